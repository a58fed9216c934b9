"""Every attention kernel under peaked, stepped and shifted softmax scores (attn_regimes.py), against the fp64 softmax
of the fp16 inputs.

Random N(0,1) inputs at scale D^-0.5 give nearly flat softmax rows, where a running maximum that misses keys, a missing
max subtraction or a wrong lazy rescale all still look right.  Here:
  R1  one-hot rows: the hot key leads by >= 60 in the exp2 domain, so P = 1 for it, P = 0 in fp16 for every other key
      and the row sum is exactly 1 - the output row IS the hot key's V row, bit for bit;
  R2  a staircase / sawtooth over key tiles (leads of 7, 9 and 24): the deferred and the taken rescale of the flash
      kernels (alpha on O and on the row sums, the per-lane running max, the wave vote) run on late tiles;
  R3  every score of a row shifted by +-150 or +-300: a kernel without max subtraction overflows, one that underflows
      returns 0 / 0, and an unmasked zero-filled pad key (score 0) would dominate the -shift rows;
  R4  R1 and R2 at scale 1.0 and 0.02 passed explicitly (every kernel folds scale * log2 e into one constant).
Bounds: rel-L2 < 1e-3 and max-abs < 4e-3 (the suite's attention bounds), every output finite.

Each case names the kernel it is meant to reach; test_attention_regimes_cpu.py checks that it does (vq_attn_fwd_route).

The row maxima of attn_fwd32d_kernel and attn_fwd64d_kernel combine the two wave halves with
__builtin_amdgcn_permlane32_swap and pass both result elements to an asm v_max_f32 (hipcc of ROCm 7.2 once read element
0 for both in the sibling form of attn_cross32_kernel).  Disassembly of the product build (-O3, gfx950) for D = 16, 32,
64 and 72: every such swap of both kernels (4 per attn_fwd32d instantiation, 8 per attn_fwd64d) feeds a v_max_f32 that
reads both swapped registers, and attn_cross32_kernel's copied-out form does the same.  The R1 cases below would fail
if one half were read twice: the hot key of every residue of the 64-key tile is swept."""
import pytest
import torch

import attn_regimes as ar
from oracle import fakequant as fq

pytestmark = pytest.mark.gpu

CASES = ar.cases()
IDS = ar.kernel_ids()


def _check(got, ref, case, what=""):
    """got, ref [r, H, D] (fp16 kernel output / fp64 reference)."""
    g = got.double()
    rel = float((g - ref).norm() / ref.norm().clamp(min=1e-30))
    mad = float((g - ref).abs().max())
    assert rel < 1e-3 and mad < 4e-3, "%s%s: rel-L2 %.3g, max-abs %.3g" % (case["id"], what, rel, mad)


def _check_one_hot(got, q, k, v, hot, case, lens, rows):
    """R1: rows (of every head) that lead by >= R1_GAP return the hot key's V row exactly.  got [n, r, H, D]."""
    gp = ar.gaps(q, k, hot, case["scale"], lens, rows)                 # [n, r, H]
    ok = gp >= ar.R1_GAP
    assert float(ok.double().mean()) >= 0.9, case["id"]
    hv = torch.stack([v[s][hot[s, rows], torch.arange(v.shape[2])[None, :]] for s in range(v.shape[0])])   # [n, r, H, D]
    bad = ok & ~(got == hv).all(-1)
    assert not bool(bad.any()), "%s: %d one-hot rows differ from the hot V row, first at %s" % (
        case["id"], int(bad.sum()), bad.nonzero()[0].tolist())
    return ok


def _run_fwd(ops, lib, dev, case):
    sh, D, scale = case["shape"], case["D"], case["scale"]
    n, Lq, lens, H = sh["n"], sh["Lq"], sh["lens"], sh["H"]
    Cc = H * D
    a = ar.fwd_layout(case)
    q, k, v, hot = ar.build(case["regime"], n, Lq, lens, H, D, scale, case["seed"])
    qd = q.reshape(n * Lq, Cc).to(dev)
    if a["offs"] is not None:
        kv = torch.cat([torch.cat([k[s, :L].reshape(L, Cc), v[s, :L].reshape(L, Cc)], 1) for s, L in enumerate(lens)])
        kvd = kv.to(dev)
        off = torch.tensor(a["offs"], dtype=torch.int32, device=dev)
    else:
        # rows kv_tok elements apart (K | V | zeros); a 2 GiB buffer for the 8-wave attn_fwd8_kernel case
        kvd = torch.zeros((a["kv_rows"], a["kv_tok"]), dtype=torch.float16, device=dev)
        kvd[:, :Cc] = k.reshape(n * lens[0], Cc).to(dev)
        kvd[:, Cc:2 * Cc] = v.reshape(n * lens[0], Cc).to(dev)
        off = None
    o = torch.full((n * Lq, Cc), float("nan"), dtype=torch.float16, device=dev)
    args = (a["n_seq"], Lq, a["Lk"], H, D, a["q_seq"], a["q_tok"], a["kv_seq"], a["kv_tok"], a["o_seq"], a["o_tok"])
    route = lib.vq_attn_fwd_route(qd.data_ptr(), kvd.data_ptr(), kvd[:, Cc:].data_ptr(), o.data_ptr(), *args,
                                  None if off is None else off.data_ptr(), scale, None)
    assert route == IDS[case["kernel"]], (case["id"], route)
    ops.attn_fwd(qd, kvd, kvd[:, Cc:], o, *args, kv_off=off, scale=scale)
    torch.cuda.synchronize()
    del kvd
    got = o.cpu().reshape(n, Lq, H, D)
    assert bool(torch.isfinite(got).all()), case["id"]
    rows = torch.arange(Lq) if Lq <= 640 else ar.sample_rows(Lq, 64)
    ref = ar.attn_ref(q, k, v, scale, lens, rows)
    _check(got[:, rows].reshape(-1, H, D), ref.reshape(-1, H, D), case)
    if hot is not None:
        _check_one_hot(got[:, rows], q, k, v, hot, case, lens, rows)


def _run_temporal(ops, dev, case):
    sh, D, scale = case["shape"], case["D"], case["scale"]
    B, T, S, H = sh["B"], sh["T"], sh["S"], sh["H"]
    Cc = H * D
    n, rows = B * S, B * T * S
    q, k, v, hot = ar.build(case["regime"], n, T, [T] * n, H, D, scale, case["seed"])

    def to_rows(x):        # [B*S, T, H, D] -> rows (b, t, s)
        return x.reshape(B, S, T, Cc).permute(0, 2, 1, 3).reshape(rows, Cc)

    qkv = torch.cat([to_rows(q), to_rows(k), to_rows(v)], 1).to(dev)
    kern = case["kernel"]
    qa = None
    if kern == "attn_temporal":
        o = torch.full((rows, Cc), float("nan"), dtype=torch.float16, device=dev)
        ops.attn_temporal(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], o, B, T, S, H, D, 3 * Cc, Cc, scale=scale)
    elif kern == "attn_temporal_long":
        # o rows ld_out = H * D + 24 apart (ops.attn_temporal_long takes dense outputs only: the C ABI directly), codes too
        from viditq_amd import _lib
        wide = torch.full((rows, Cc + 24), float("nan"), dtype=torch.float16, device=dev)
        o = wide[:, :Cc]
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        Kp = (Cc + 127) // 128 * 128
        qa = ops.QAct(torch.empty((rows, Kp), dtype=torch.int8, device=dev), torch.empty(rows, device=dev),
                      torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev), Cc, 8)
        _lib.check(_lib.load().vq_attn_temporal_long(
            qkv.data_ptr(), qkv[:, Cc:].data_ptr(), qkv[:, 2 * Cc:].data_ptr(), None, None, qa.xq.data_ptr(), qa.sx.data_ptr(),
            qa.zx.data_ptr(), qa.R.data_ptr(), st.data_ptr(), wide.data_ptr(), B, T, S, H, D, 3 * Cc, Cc + 24, Kp, scale,
            torch.cuda.current_stream().cuda_stream), "vq_attn_temporal_long")
        torch.cuda.synchronize()
        assert bool(torch.isnan(wide[:, Cc:]).all()), case["id"]                   # nothing written past H * D
    else:
        o = torch.full((rows, Cc), float("nan"), dtype=torch.float16, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        qa = ops.attn_temporal_rowquant(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], B, T, S, H, D, 3 * Cc, scale=scale, status=st,
                                        o=o)
    torch.cuda.synchronize()
    got = o.cpu().reshape(B, T, S, H, D).permute(0, 2, 1, 3, 4).reshape(n, T, H, D)
    assert bool(torch.isfinite(got).all()), case["id"]
    ref = ar.attn_ref(q, k, v, scale, [T] * n)
    _check(got.reshape(-1, H, D), ref.reshape(-1, H, D), case)
    ok = None
    if hot is not None:
        ok = _check_one_hot(got, q, k, v, hot, case, [T] * n, torch.arange(T))       # [n, T, H]
    if qa is None:
        return
    # the fused quantizer = vq_rowquant of the kernel's own fp16 output, bit for bit
    st0 = torch.zeros(1, dtype=torch.int32, device=dev)
    rq = ops.rowquant(o.contiguous().view(1, rows, Cc), status=st0)
    for f in ("xq", "sx", "zx", "R"):
        assert torch.equal(getattr(qa, f), getattr(rq, f)), (case["id"], f)
    assert int(st.item()) == int(st0.item())
    if ok is None:
        return
    # independent of the kernels: a row whose heads are all one-hot is a gathered V row, so its codes, scale and zero
    # point are the oracle's dynamic quantizer of that V row
    full = ok.all(-1)                                                                  # [n, T]
    hv = torch.stack([v[s][hot[s], torch.arange(H)[None, :]] for s in range(n)])       # [n, T, H, D]
    sel = full.reshape(B, S, T).permute(0, 2, 1).reshape(rows)                          # rows (b, t, s)
    assert float(sel.double().mean()) >= 0.9, case["id"]
    x = hv.reshape(B, S, T, Cc).permute(0, 2, 1, 3).reshape(rows, Cc)[sel]
    codes, _, delta, zp, eps = fq.dyn_act_quant(x.float()[None], 8)
    assert not eps
    idx = sel.nonzero()[:, 0]
    assert torch.equal(qa.xq.cpu()[idx, :Cc].int() + 128, codes[0].int()), case["id"]
    assert torch.equal(qa.sx.cpu()[idx], delta.reshape(-1)), case["id"]
    zx = zp.reshape(-1).int() - 128
    assert torch.equal(qa.zx.cpu()[idx], zx), case["id"]
    assert torch.equal(qa.R.cpu()[idx], (codes[0].int() - 128).sum(-1) - Cc * zx), case["id"]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_attention_kernel_under_structured_scores(ops, dev, case):
    if case["kernel"].startswith("VQ_ATTN_K_"):
        from viditq_amd import _lib
        _run_fwd(ops, _lib.load(), dev, case)
    else:
        _run_temporal(ops, dev, case)

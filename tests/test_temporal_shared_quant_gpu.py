"""vq_attn_temporal_rowquant_shared: temporal attention with attn_temp.proj's dynamic per-token quantizer fused in for a
joint cond | uncond forward (B <= 2: a token's grid is shared by its rows of both samples) at 2..8 bits - the shared-grid
forms of attn_temporal_quant2_kernel (H = 16) and attn_temporal_quant_kernel (H < 16).  Every field against vq_rowquant of
the kernel's own fp16 output, that output against the dynamic form's per sample, the grid against the oracle's shared
token grid, edge rows (exact ties, both end codes) against the CPU oracle, the eps flag per token, nothing written outside
the rows of the launch, and the block route behind its switch, eager and replayed from a graph."""
import pytest
import torch

import quant_rows as qr
from oracle import fakequant as fq
from test_kernels_gpu import h16
from test_quantizer_edges_gpu import _first_diff
from test_temporal_shared_quant_cpu import SHAPES, edge_seed

pytestmark = pytest.mark.gpu

FIELDS = ("xq", "sx", "zx", "R")


def _smooth(Cc, dev):
    return torch.exp(torch.randn(Cc, generator=torch.Generator().manual_seed(3)) * 0.6).float().to(dev)


def _same(got, ref, what):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        assert a.shape == b.shape and torch.equal(a, b), _first_diff(a.cpu().float(), b.cpu().float(), "%s %s" % (what, f))


# ----------------------------------------------------------------------------- 1. equals the two launches
@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("n_bits", [8, 6, 4])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T,S,H,D", SHAPES)
def test_shared_fused_attention_equals_two_launches(ops, dev, T, S, H, D, B, n_bits, smooth):
    Cc, n = H * D, T * S
    qkv = h16(B * n, 3 * Cc, seed=T * 31 + S + B).to(dev)
    qkv[(T - 1) * S + 1, 2 * Cc:] = 0                   # one value row zeroed (still a normal output row)
    sm = _smooth(Cc, dev) if smooth else None
    q, k, v = qkv, qkv[:, Cc:], qkv[:, 2 * Cc:]
    o = torch.full((B * n, Cc), float("nan"), dtype=torch.float16, device=dev)
    st = ops.new_status(dev)
    got = ops.attn_temporal_rowquant_shared(q, k, v, B, T, S, H, D, 3 * Cc, n_bits=n_bits, status=st, o=o, s=sm)
    assert got is not None and got.n_bits == n_bits and got.K == Cc
    st_ref = ops.new_status(dev)
    ref = ops.rowquant(o.view(B, n, Cc), n_bits=n_bits, s=sm, status=st_ref)
    _same(got, ref, "against rowquant of o:")
    assert int(st.item()) == int(st_ref.item())
    assert bool((got.xq[:, Cc:] == 0).all())
    got2 = ops.attn_temporal_rowquant_shared(q, k, v, B, T, S, H, D, 3 * Cc, n_bits=n_bits, s=sm)   # o = None
    _same(got2, got, "without o:")
    # the attention output of a sample is the dynamic form's for that sample alone, bit for bit
    for b in range(B):
        part = qkv[b * n:(b + 1) * n]
        ob = torch.full((n, Cc), float("nan"), dtype=torch.float16, device=dev)
        st1 = ops.new_status(dev)
        one = ops.attn_temporal_rowquant(part, part[:, Cc:], part[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, status=st1, o=ob, s=sm)
        a, w = o[b * n:(b + 1) * n].view(torch.int16), ob.view(torch.int16)
        assert torch.equal(a, w), _first_diff(a.cpu().int(), w.cpu().int(), "o of sample %d (bits)" % b)
        if B == 1 and n_bits == 8:                       # then the whole result is the existing entry point's
            _same(got, one, "against attn_temporal_rowquant:")
            assert int(st.item()) == int(st1.item())


# ----------------------------------------------------------------------------- 2. the grid really is shared
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("T,S,H,D", SHAPES)
def test_the_grid_is_shared_by_the_samples(ops, dev, T, S, H, D, n_bits):
    """Sample 0's V is 4 x larger on even t, sample 1's on odd t: a per-sample or per-row grid is wrong at EVERY token."""
    Cc, n = H * D, T * S
    qkv = h16(2 * n, 3 * Cc, seed=5 * T + S).to(dev)
    t_of_row = (torch.arange(2 * n, device=dev) // S) % T
    b_of_row = torch.arange(2 * n, device=dev) // n
    big = (t_of_row % 2) == b_of_row
    qkv[:, 2 * Cc:] = torch.where(big[:, None], qkv[:, 2 * Cc:] * 4, qkv[:, 2 * Cc:])
    o = torch.empty((2 * n, Cc), dtype=torch.float16, device=dev)
    got = ops.attn_temporal_rowquant_shared(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 2, T, S, H, D, 3 * Cc, n_bits=n_bits, o=o)
    assert torch.equal(got.sx[:n], got.sx[n:]) and torch.equal(got.zx[:n], got.zx[n:])
    x = o.cpu().float().view(2, n, Cc)
    delta, zp, eps = fq.token_params(x, n_bits)
    assert not eps
    cx = 128 if n_bits == 8 else 0
    assert torch.equal(got.sx.cpu()[:n], delta.reshape(-1)), _first_diff(got.sx.cpu()[:n], delta.reshape(-1), "sx")
    assert torch.equal(got.zx.cpu()[:n], zp.reshape(-1).int() - cx)
    # and the inputs do what they are for: at every token a sample's own grid is not the shared one
    own = [fq.token_params(x[b:b + 1], n_bits) for b in range(2)]
    same = [(own[b][0] == delta) & (own[b][1] == zp) for b in range(2)]
    assert not bool((same[0] & same[1]).any())


# ----------------------------------------------------------------------------- 3. edge rows against the CPU oracle
@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "q2_smooth"])
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("T,S,H,D", SHAPES)
def test_shared_fused_quantizer_edges(ops, dev, T, S, H, D, n_bits, smooth):
    """One-hot temporal attention (another seed per sample) whose V rows are Q1, Q3 and Q6 rows; sample 1's V row of a token
    is sample 0's with the channels reversed, so the two rows have the same extremes, the shared grid is the row's own and
    Q1's exact ties stay exact.  The output IS the hot V row: codes, sx, zx, R are the oracle's quantizer of x [2, n, C]."""
    import attn_regimes as ar
    Cc, scale = H * D, D ** -0.5
    s = qr.q2_smooth(Cc) if smooth else None
    q3 = qr.q3(1, Cc, qr.q3_magnitudes(97))
    pool = torch.cat([qr.q1(1, 48, Cc, n_bits, fixed=smooth), q3[:, qr.split_eps(q3, n_bits, s)[0]], qr.q6(1, Cc)], 1)
    v0 = qr.thin(pool, S * T)[0].reshape(S, T, Cc)
    vs = [v0, v0.flip(-1)]

    def to_rows(t):        # [S, T, C] -> rows (t, s)
        return t.reshape(S, T, Cc).permute(1, 0, 2).reshape(T * S, Cc)

    parts, sels, wants = [], [], []
    for b in range(2):
        q, k, hot = qr.one_hot_qk(S, T, H, D, scale, seed=edge_seed(T, D, b))
        parts.append(torch.cat([to_rows(q), to_rows(k), to_rows(vs[b])], 1))
        gp = ar.gaps(q, k, hot[:, :, None].expand(S, T, H).contiguous(), scale, [T] * S)
        sels.append((gp >= ar.R1_GAP).all(-1).permute(1, 0).reshape(T * S))
        wants.append(to_rows(torch.stack([vs[b][i][hot[i]] for i in range(S)])))
    qkv = torch.cat(parts, 0).to(dev)
    n = T * S
    o = torch.full((2 * n, Cc), float("nan"), dtype=torch.float16, device=dev)
    st = ops.new_status(dev)
    sd = None if s is None else s.to(dev)
    qa = ops.attn_temporal_rowquant_shared(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 2, T, S, H, D, 3 * Cc, n_bits=n_bits, status=st,
                                           o=o, s=sd)
    assert qa is not None
    sel = sels[0] & sels[1]                                  # (the cap: test_temporal_shared_quant_cpu)
    assert float(sel.double().mean()) >= 0.8
    idx = sel.nonzero()[:, 0]
    x = torch.stack([wants[0][idx], wants[1][idx]])          # [2, n_sel, C]
    oc = o.cpu().view(2, n, Cc)
    assert torch.equal(oc[:, idx], x), "the output is not the hot V row"
    codes, _, delta, zp, eps = fq.dyn_act_quant(qr.smoothed(x, s), n_bits)
    assert not eps
    cx = 128 if n_bits == 8 else 0
    got = qa.xq.cpu().view(2, n, -1)[:, idx, :Cc].int() + cx
    assert torch.equal(got, codes.int()), _first_diff(got, codes.int(), "fused codes")
    assert bool((qa.xq[:, Cc:] == 0).all())
    zx = zp.reshape(-1).int() - cx
    for b in range(2):
        assert torch.equal(qa.sx.cpu().view(2, n)[b, idx], delta.reshape(-1))
        assert torch.equal(qa.zx.cpu().view(2, n)[b, idx], zx)
        assert torch.equal(qa.R.cpu().view(2, n)[b, idx], (codes[b].int() - cx).sum(-1) - Cc * zx)
    if not smooth:
        assert bool((qr.tie_distance(x, n_bits) == 0).any()), "no exact tie among the compared elements"
        assert int(got.min()) == 0 and int(got.max()) == 2 ** n_bits - 1
    if bool(sel.all()):
        assert int(st.item()) == 0


# ----------------------------------------------------------------------------- 4. eps fill is a token's, not a row's
@pytest.mark.parametrize("T,S,H,D", [(5, 9, 2, 32), (3, 5, 16, 16)])
def test_eps_fill_is_per_token(ops, dev, T, S, H, D):
    """(VQ_ST_EPSFILL = 1, include/viditq.h.)"""
    Cc, n = H * D, T * S
    base = h16(2 * n, 3 * Cc, seed=9 * T + S).to(dev)

    def run(zero_both):
        qkv = base.clone()
        if zero_both:                                    # token (s = 2): V of every frame zero in both samples
            for b in range(2):
                qkv[b * n + 2:(b + 1) * n:S, 2 * Cc:] = 0
        qkv[4:n:S, 2 * Cc:] = 0                          # token (s = 4): zero in sample 0 only
        o = torch.empty((2 * n, Cc), dtype=torch.float16, device=dev)
        st, st_ref = ops.new_status(dev), ops.new_status(dev)
        got = ops.attn_temporal_rowquant_shared(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 2, T, S, H, D, 3 * Cc, n_bits=6, status=st, o=o)
        ref = ops.rowquant(o.view(2, n, Cc), n_bits=6, status=st_ref)
        _same(got, ref, "eps:")
        assert bool((o[4:n:S] == 0).all()) and not bool((o[n + 4::S] == 0).all())
        return int(st.item()), int(st_ref.item())
    assert run(True) == (1, 1)
    assert run(False) == (0, 0)


# ----------------------------------------------------------------------------- 5. guard rows
@pytest.mark.parametrize("T,S,H,D,B", [(5, 9, 2, 32, 2), (5, 3, 16, 16, 2)])
def test_shared_fused_attention_writes_only_its_rows(ops, dev, T, S, H, D, B):
    """Rows >= T of a 16-row tile exist in the kernel but not in memory: with poison rows before and after every output,
    nothing outside [0, B * T * S) changes."""
    from viditq_amd import _lib
    Cc, rows, pad, Kp = H * D, B * T * S, 16, ops.pad128(H * D)
    qkv = h16(rows, 3 * Cc, seed=7 * T + B).to(dev)
    bufs = {"xq": torch.full((rows + 2 * pad, Kp), 0x5A, dtype=torch.int8, device=dev),
            "sx": torch.full((rows + 2 * pad,), -7.0, dtype=torch.float32, device=dev),
            "zx": torch.full((rows + 2 * pad,), -77, dtype=torch.int32, device=dev),
            "R": torch.full((rows + 2 * pad,), -777, dtype=torch.int32, device=dev),
            "o": torch.full((rows + 2 * pad, Cc), 1234.0, dtype=torch.float16, device=dev)}
    before = {n: t.clone() for n, t in bufs.items()}
    p = {n: t[pad:].data_ptr() for n, t in bufs.items()}
    _lib.check(_lib.load().vq_attn_temporal_rowquant_shared(
        qkv.data_ptr(), qkv[:, Cc:].data_ptr(), qkv[:, 2 * Cc:].data_ptr(), None, None, p["xq"], p["sx"], p["zx"], p["R"], None,
        p["o"], B, T, S, H, D, 3 * Cc, Kp, 6, D ** -0.5, torch.cuda.current_stream().cuda_stream),
        "vq_attn_temporal_rowquant_shared")
    torch.cuda.synchronize()
    for n, t in bufs.items():
        assert torch.equal(t[:pad], before[n][:pad]) and torch.equal(t[pad + rows:], before[n][pad + rows:]), n
    ref = ops.rowquant(bufs["o"][pad:pad + rows].contiguous().view(B, T * S, Cc), n_bits=6)
    for f in FIELDS:
        assert torch.equal(bufs[f][pad:pad + rows], getattr(ref, f)), f


# ----------------------------------------------------------------------------- 6. the block's route
NAMES = ["rowquant", "attn_temporal", "attn_temporal_rowquant", "attn_temporal_rowquant_shared"]


def _tiny_w6a6_joint(dev):
    """The tiny W6A6 joint model of test_bench_config_gpu.test_six_bit_plans_at_model_level."""
    from helpers import load_npz, quant_params_of
    from test_parity_gpu import _cfgs, _load_qp, _stdit
    from viditq_amd.config import to_config
    g = load_npz("tiny_stdit_w6a6.npz")
    wq, aq = _cfgs(6, mixed_precision=[4, 6, 8])
    qnn = _stdit(g, dev, wq, to_config(dict(aq, n_bits=6)), cfg_split=False)
    _load_qp(qnn, quant_params_of(g, "qp"))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    x, y, mask, t = g["x"].to(dev), g["y"].half().to(dev), g["mask"].to(dev), g["t"].to(dev)
    return g, qnn, (torch.cat([x, x]), torch.cat([t, t]), y), dict(mask=mask)


def test_block_route_of_the_joint_plans(ops, dev, monkeypatch):
    from helpers import load_npz, rel_l2
    from test_model_gpu import _build
    from test_static_attn_quant_gpu import _count_block_calls
    from viditq_amd.t2v import stdit
    g, qnn, args, kw = _tiny_w6a6_joint(dev)
    unpatched = qnn(*args, **kw)                            # (the switch as the environment left it)
    monkeypatch.setattr(stdit, "_ATTN_QUANT_JOINT", False)
    parent = qnn(*args, **kw)
    per_block = _count_block_calls(ops, monkeypatch, stdit, NAMES)
    # switch off: today's launches and outputs
    off = qnn(*args, **kw)
    assert torch.equal(off, parent)
    if __import__("os").environ.get("VQ_ATTN_QUANT_JOINT", "0") == "0":
        assert torch.equal(off, unpatched)
    assert len(per_block) == 2 and per_block[0] == per_block[1]
    n_rowquant = per_block[0]["rowquant"]
    assert per_block[0] == dict(rowquant=n_rowquant, attn_temporal=1, attn_temporal_rowquant=0, attn_temporal_rowquant_shared=0)
    del per_block[:]
    # switch on: one launch instead of attention + proj's quantizer
    monkeypatch.setattr(stdit, "_ATTN_QUANT_JOINT", True)
    on = qnn(*args, **kw)
    assert per_block == [dict(rowquant=n_rowquant - 1, attn_temporal=0, attn_temporal_rowquant=0,
                              attn_temporal_rowquant_shared=1)] * 2
    assert torch.isfinite(on).all()
    ref32, ref16 = g["w6a6_joint"], g["w6a6_joint_ref_fp16"]
    assert rel_l2(on.cpu(), ref32) < 1.25 * rel_l2(ref16, ref32) + 1e-4    # test_six_bit_plans_at_model_level's own bound
    assert qnn.check_status() == 0
    # the W8A8 joint forward (8 bits, B = 2) takes it too, inside test_model_gpu's bound
    g8 = load_npz("tiny_stdit_w8a8.npz")
    q8 = _build(g8, dev, 8)
    x, y, mask, t = g8["x"].to(dev), g8["y"].half().to(dev), g8["mask"].to(dev), g8["t"].to(dev)
    del per_block[:]
    joint = q8(torch.cat([x, x]), torch.cat([t, t]), y, mask=mask)
    assert all(b["attn_temporal_rowquant_shared"] == 1 and b["attn_temporal"] == 0 for b in per_block) and len(per_block) == 2
    assert rel_l2(joint.cpu(), g8["w8a8_joint"]) < 1.95e-3
    # a B = 1 W8A8 forward never does: today's fused call, switch on or off
    for sw in (True, False):
        monkeypatch.setattr(stdit, "_ATTN_QUANT_JOINT", sw)
        del per_block[:]
        q8(x, t, y[:1], mask=mask)
        assert per_block == [dict(rowquant=per_block[0]["rowquant"], attn_temporal=0, attn_temporal_rowquant=1,
                                  attn_temporal_rowquant_shared=0)] * 2, sw


# ----------------------------------------------------------------------------- 7. graph replay
def test_switched_on_joint_forward_replays_from_a_graph(ops, dev, monkeypatch):
    """Nothing synchronises: the switched-on joint forward is capturable and its replay is the eager result bit for bit."""
    from viditq_amd.graph import ForwardGraph
    from viditq_amd.t2v import stdit
    monkeypatch.setattr(stdit, "_ATTN_QUANT_JOINT", True)
    _, qnn, args, kw = _tiny_w6a6_joint(dev)
    kw = dict(kw, timestep_id=int(args[1][0]))             # (known on the host: no t[0].item() under capture)
    calls = []
    real = ops.attn_temporal_rowquant_shared
    monkeypatch.setattr(ops, "attn_temporal_rowquant_shared", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        eager = qnn(*args, **kw).clone()
    assert len(calls) == 2
    fg = ForwardGraph(qnn, *args, kw)
    out = fg.run(*args)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)

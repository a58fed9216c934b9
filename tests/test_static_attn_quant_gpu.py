"""vq_attn_temporal_rowquant_static: temporal attention with attn_temp.proj's static tensor-wise quantizer fused in - the
static-grid forms of attn_temporal_quant2_kernel (H = 16), attn_temporal_quant_kernel (H < 16) and
attn_temporal_long_kernel (17 <= T <= 64).  Codes, sx, zx and R against vq_rowquant's static case on the kernel's own
fp16 output and against the CPU oracle (oracle/fakequant.py: static_act_quant) on exact ties, both clamps and fp16's
largest value; nothing written outside the rows of the launch; and the block route behind its switch."""
import pytest
import torch

import quant_rows as qr
from oracle import fakequant as fq
from test_kernels_gpu import h16
from test_quantizer_edges_gpu import _first_diff
from test_static_attn_quant_cpu import EDGE_CASES

pytestmark = pytest.mark.gpu

# (T, S, H, D): trimmed kernel | generic T <= 16 kernel | long kernel
TWO_KERNELS = [(16, 8, 16, 72), (5, 9, 2, 32), (16, 8, 8, 64), (17, 6, 4, 16), (64, 5, 16, 72)]


def _plain(ops, qkv, B, T, S, H, D):
    """The un-fused attention output: attn_temporal (T <= 16) / attn_temporal_long without the quantizer."""
    Cc = H * D
    o = torch.empty((B * T * S, Cc), dtype=torch.float16, device=qkv.device)
    if T <= 16:
        ops.attn_temporal(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], o, B, T, S, H, D, 3 * Cc, Cc)
    else:
        ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], B, T, S, H, D, 3 * Cc, o=o)
    return o


@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T,S,H,D", TWO_KERNELS)
def test_static_fused_attention_equals_two_kernels(ops, dev, T, S, H, D, B, n_bits, smooth):
    Cc, rows = H * D, B * T * S
    qkv = h16(rows, 3 * Cc, seed=T * 31 + S + B).to(dev)
    qkv[(T - 1) * S + 1, 2 * Cc:] = 0                   # one value row zeroed (still a normal output row)
    o_ref = _plain(ops, qkv, B, T, S, H, D)
    sm = torch.exp(torch.randn(Cc, generator=torch.Generator().manual_seed(3)) * 0.6).float().to(dev) if smooth else None
    # the grid from the 2nd and 98th percentile of what the quantizer sees: both clamps act
    xin = o_ref.float() if sm is None else o_ref.float() / sm
    lo, hi = [float(v) for v in torch.quantile(xin.flatten()[:: max(1, xin.numel() // 200000)], torch.tensor([0.02, 0.98], device=dev))]
    qmax = 2 ** n_bits - 1
    delta = torch.tensor([(hi - lo) / qmax], dtype=torch.float32, device=dev)
    zp = torch.round(-lo / delta)
    o = torch.zeros_like(o_ref)
    q, k, v = qkv, qkv[:, Cc:], qkv[:, 2 * Cc:]
    got = ops.attn_temporal_rowquant_static(q, k, v, B, T, S, H, D, 3 * Cc, delta, zp, n_bits=n_bits, o=o, s=sm)
    assert got is not None and got.n_bits == n_bits and got.K == Cc
    ref = ops.rowquant(o.view(B, T * S, Cc), n_bits=n_bits, delta=delta, zp=zp, s=sm, fast_div=False)
    for f in ("xq", "sx", "zx", "R"):
        a, b = getattr(got, f), getattr(ref, f)
        assert a.shape == b.shape and torch.equal(a, b), _first_diff(a.cpu().int(), b.cpu().int(), f)
    cx = 128 if n_bits == 8 else 0
    raw = got.xq[:, :Cc].int() + cx
    assert int(raw.min()) == 0 and int(raw.max()) == qmax, "both clamps must act"
    assert bool((got.xq[:, Cc:] == 0).all())
    got2 = ops.attn_temporal_rowquant_static(q, k, v, B, T, S, H, D, 3 * Cc, delta, zp, n_bits=n_bits, s=sm)   # o = None
    for f in ("xq", "sx", "zx", "R"):
        assert torch.equal(getattr(got2, f), getattr(got, f)), f
    diff = (o.float() - o_ref.float()).abs()
    assert float((diff > 0).float().mean()) < 2e-3
    assert bool((diff <= 2.0 ** -10 * o_ref.float().abs().clamp(min=2.0 ** -14)).all())     # one fp16 ulp


@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "q2_smooth"])
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("T,S,H,D", EDGE_CASES)
def test_static_fused_attention_edge_rows_against_the_oracle(ops, dev, T, S, H, D, n_bits, smooth):
    """One-hot temporal attention whose V rows are quant_rows.static_rows (ties of both parities, values beyond both grid
    ends, +-65504): the output IS the hot V row, so codes, sx, zx and R must be the oracle's static quantizer of it."""
    import attn_regimes as ar
    Cc, scale = H * D, D ** -0.5
    s = qr.q2_smooth(Cc) if smooth else None
    vrows, delta, zp = qr.static_rows(1, S * T, Cc, n_bits, per_token=False)
    q, k, hot = qr.one_hot_qk(S, T, H, D, scale, seed=100 * T + D)
    v = vrows[0].reshape(S, T, H, D)

    def to_rows(t):        # [S, T, H, D] -> rows (t, s)
        return t.reshape(S, T, Cc).permute(1, 0, 2).reshape(T * S, Cc)

    qkv = torch.cat([to_rows(q), to_rows(k), to_rows(v)], 1).to(dev)
    o = torch.full((T * S, Cc), float("nan"), dtype=torch.float16, device=dev)
    sd = None if s is None else s.to(dev)
    qa = ops.attn_temporal_rowquant_static(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, delta.to(dev), zp.to(dev),
                                           n_bits=n_bits, o=o, s=sd)
    assert qa is not None
    torch.cuda.synchronize()
    gp = ar.gaps(q, k, hot[:, :, None].expand(S, T, H).contiguous(), scale, [T] * S)
    sel = (gp >= ar.R1_GAP).all(-1).permute(1, 0).reshape(T * S)
    assert float(sel.double().mean()) >= 0.9
    want = to_rows(torch.stack([v[i][hot[i]] for i in range(S)]))
    idx = sel.nonzero()[:, 0]
    assert torch.equal(o.cpu()[idx], want[idx]), "the output is not the hot V row"
    codes, _ = fq.static_act_quant(qr.smoothed(want[idx][None], s), delta, zp, n_bits)
    cx = 128 if n_bits == 8 else 0
    got = qa.xq.cpu()[idx, :Cc].int() + cx
    assert torch.equal(got, codes[0].int()), _first_diff(got, codes[0].int(), "fused static codes")
    assert int(got.min()) == 0 and int(got.max()) == 2 ** n_bits - 1
    assert bool((qa.xq[:, Cc:] == 0).all())
    assert torch.equal(qa.sx.cpu(), delta.expand(T * S))
    zx = int(zp) - cx
    assert torch.equal(qa.zx.cpu(), torch.full((T * S,), zx, dtype=torch.int32))
    assert torch.equal(qa.R.cpu()[idx], ((codes[0].int() - cx).sum(-1) - Cc * zx).int())


@pytest.mark.parametrize("T,S,H,D,B", [(5, 9, 2, 32, 2), (5, 3, 16, 16, 1), (17, 6, 4, 16, 2)])
def test_static_fused_attention_writes_only_its_rows(ops, dev, T, S, H, D, B):
    """Rows >= T of a 16-row tile exist in the kernel but not in memory: with poison rows before and after every output,
    nothing outside [0, B * T * S) changes."""
    from viditq_amd import _lib
    Cc, rows, pad, Kp = H * D, B * T * S, 16, ops.pad128(H * D)
    qkv = h16(rows, 3 * Cc, seed=7 * T + B).to(dev)
    delta = torch.tensor([0.01], device=dev)
    zp = torch.tensor([100.0], device=dev)
    bufs = {"xq": torch.full((rows + 2 * pad, Kp), 0x5A, dtype=torch.int8, device=dev),
            "sx": torch.full((rows + 2 * pad,), -7.0, dtype=torch.float32, device=dev),
            "zx": torch.full((rows + 2 * pad,), -77, dtype=torch.int32, device=dev),
            "R": torch.full((rows + 2 * pad,), -777, dtype=torch.int32, device=dev),
            "o": torch.full((rows + 2 * pad, Cc), 1234.0, dtype=torch.float16, device=dev)}
    before = {n: t.clone() for n, t in bufs.items()}
    p = {n: t[pad:].data_ptr() for n, t in bufs.items()}
    _lib.check(_lib.load().vq_attn_temporal_rowquant_static(
        qkv.data_ptr(), qkv[:, Cc:].data_ptr(), qkv[:, 2 * Cc:].data_ptr(), None, None, delta.data_ptr(), zp.data_ptr(),
        p["xq"], p["sx"], p["zx"], p["R"], p["o"], B, T, S, H, D, 3 * Cc, Cc, Kp, 8, D ** -0.5,
        torch.cuda.current_stream().cuda_stream), "vq_attn_temporal_rowquant_static")
    torch.cuda.synchronize()
    for n, t in bufs.items():
        assert torch.equal(t[:pad], before[n][:pad]) and torch.equal(t[pad + rows:], before[n][pad + rows:]), n
    assert bool((bufs["sx"][pad:pad + rows] == 0.01).all()) and bool((bufs["zx"][pad:pad + rows] == -28).all())
    ref = ops.rowquant(bufs["o"][pad:pad + rows].contiguous().view(B, T * S, Cc), delta=delta, zp=zp)
    assert torch.equal(bufs["xq"][pad:pad + rows], ref.xq) and torch.equal(bufs["R"][pad:pad + rows], ref.R)


# ----------------------------------------------------------------------------- the block's route
def _count_block_calls(ops, monkeypatch, stdit, names):
    count = dict.fromkeys(names, 0)
    for name in names:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            count[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    per_block = []
    inner = stdit.STDiTBlock.forward_fused

    def forward_fused(self, x2, y2, t0, y_lens, tpe, B, kv_ready=None, mod=None):
        if kv_ready is None:
            kv_ready = self.prompt_kv(y2)
        before = dict(count)
        out = inner(self, x2, y2, t0, y_lens, tpe, B, kv_ready=kv_ready, mod=mod)
        per_block.append({k: count[k] - before[k] for k in count})
        return out
    monkeypatch.setattr(stdit.STDiTBlock, "forward_fused", forward_fused)
    return per_block


def test_block_route_of_the_static_plan(ops, dev, monkeypatch):
    from helpers import load_npz, rel_l2
    from test_static_quant_gpu import _tiny_static_stdit
    from viditq_amd.t2v import stdit
    qnn, args, kw = _tiny_static_stdit(dev)
    g = load_npz("tiny_stdit_static.npz")
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", False)
    parent = qnn(*args, **kw)
    names = ["rowquant_static", "rowquant", "attn_temporal_rowquant_static", "attn_temporal"]
    per_block = _count_block_calls(ops, monkeypatch, stdit, names)
    # switch off: today's launches and outputs
    off = qnn(*args, **kw)
    assert torch.equal(off, parent)
    assert per_block == [dict(rowquant_static=3, rowquant=5, attn_temporal_rowquant_static=0, attn_temporal=1)] * 2
    del per_block[:]
    # switch on
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", True)
    on = qnn(*args, **kw)
    assert per_block == [dict(rowquant_static=3, rowquant=4, attn_temporal_rowquant_static=1, attn_temporal=0)] * 2
    assert torch.isfinite(on).all()
    # the bound test_parity_gpu.test_static_activation_plans_match_reference applies to this golden with qp_tw
    ref32, ref16 = g["tw_joint_t721"], g["tw_joint_t721_ref_fp16"]
    assert rel_l2(on.cpu(), ref32) < 1.25 * rel_l2(ref16, ref32) + 1e-4
    # without the one-pass static route the switch does nothing: the layerwise route, as before
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    del per_block[:]
    layerwise = qnn(*args, **kw)
    assert torch.equal(layerwise, parent)
    assert all(b["attn_temporal_rowquant_static"] == 0 and b["attn_temporal"] == 1 for b in per_block)


def test_switched_on_forward_replays_from_a_graph(ops, dev, monkeypatch):
    """The grid is read on the device: nothing synchronises, so the switched-on forward is capturable and its replay
    returns the eager result bit for bit."""
    from test_static_quant_gpu import _tiny_static_stdit
    from viditq_amd.t2v import stdit
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", True)
    qnn, args, kw = _tiny_static_stdit(dev)
    kw = dict(kw, timestep_id=int(args[1][0]))             # (known on the host: no t[0].item() under capture)
    from viditq_amd.graph import ForwardGraph
    with torch.no_grad():
        eager = qnn(*args, **kw).clone()
    fg = ForwardGraph(qnn, *args, kw)
    out = fg.run(*args)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)

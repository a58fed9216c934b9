"""Long videos (17 <= T <= 64 frames, OpenSORA 64x512x512): the temporal attention kernel with the fused per-token
quantizer of attn_temp.proj, its dispatch from the fused STDiT block, and the 64-frame model against the CPU oracle."""
import pytest
import torch

from oracle import stdit_ref as sr

pytestmark = pytest.mark.gpu


def h16(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def rel_l2(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp(min=1e-30))


def _attn_ref(q, k, v, scale):
    # q, k, v [n, T, H, D]; fp32 softmax (blocks.py:179-187)
    a = torch.einsum("nqhd,nkhd->nhqk", q.float() * scale, k.float()).softmax(-1)
    return torch.einsum("nhqk,nkhd->nqhd", a, v.float())


def _temporal_ref(qkv, B, T, S, H, D):
    Cc = H * D
    q, k, v = [t.cpu().reshape(B, T, S, H, D).permute(0, 2, 1, 3, 4).reshape(B * S, T, H, D) for t in qkv.split(Cc, dim=1)]
    return _attn_ref(q, k, v, D ** -0.5).reshape(B, S, T, Cc).permute(0, 2, 1, 3).reshape(B * T * S, Cc)


SHAPES = [(64, 16, 72), (37, 16, 72), (9, 4, 16), (16, 8, 64), (5, 2, 32)]


@pytest.mark.parametrize("T", [17, 32, 33, 48, 63, 64])
@pytest.mark.parametrize("S,H,D", SHAPES)
def test_attn_temporal_long_matches_fp32(ops, dev, T, S, H, D):
    B = 2 if S < 16 else 1
    Cc = H * D
    qkv = h16(B * T * S, 3 * Cc, seed=T * 7 + S + D).to(dev)
    o = torch.full((B * T * S, Cc), float("nan"), dtype=torch.float16, device=dev)
    ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], B, T, S, H, D, 3 * Cc, o=o)
    assert rel_l2(o.cpu(), _temporal_ref(qkv, B, T, S, H, D)) < 1e-3


def test_attn_temporal_long_full_size(ops, dev):
    """64 frames x 1024 positions x 16 heads of 72 (STDiT-XL/2 at 64x512x512), codes mode with the fp16 copy."""
    T, S, H, D = 64, 1024, 16, 72
    Cc = H * D
    qkv = h16(T * S, 3 * Cc, seed=5).to(dev)
    o = torch.empty((T * S, Cc), dtype=torch.float16, device=dev)
    qa = ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, o=o, quant=True)
    assert rel_l2(o.cpu(), _temporal_ref(qkv, 1, T, S, H, D)) < 1e-3
    ref = ops.rowquant(o.view(1, T * S, Cc))
    for f in ("xq", "sx", "zx", "R"):
        assert torch.equal(getattr(qa, f), getattr(ref, f)), f


@pytest.mark.parametrize("T", [17, 33, 64])
@pytest.mark.parametrize("S,H,D", SHAPES)
def test_attn_temporal_long_codes_equal_rowquant(ops, dev, T, S, H, D):
    """Codes, scales, zero points, row sums and the status word of the fused mode = vq_rowquant of the kernel's own fp16
    output, with and without the consuming Linear's smoothing vector; the codes-only call gives the same codes."""
    Cc = H * D
    qkv = h16(T * S, 3 * Cc, seed=T * 31 + S).to(dev)
    qkv[(T - 1) * S + 1, 2 * Cc:] = 0                   # one value row zeroed
    o_plain = torch.empty((T * S, Cc), dtype=torch.float16, device=dev)
    ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, o=o_plain)
    st1 = torch.zeros(1, dtype=torch.int32, device=dev)
    o = torch.zeros_like(o_plain)
    got = ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, o=o, quant=True, status=st1)
    assert torch.equal(o, o_plain)                      # the quantizer does not change the fp16 output
    st0 = torch.zeros(1, dtype=torch.int32, device=dev)
    ref = ops.rowquant(o.view(1, T * S, Cc), status=st0)
    assert got.K == ref.K and got.xq.shape == ref.xq.shape
    for f in ("xq", "sx", "zx", "R"):
        assert torch.equal(getattr(got, f), getattr(ref, f)), f
    assert int(st0.item()) == int(st1.item())
    got2 = ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, quant=True)
    for f in ("xq", "sx", "zx", "R"):
        assert torch.equal(getattr(got2, f), getattr(got, f)), f
    sm = torch.exp(torch.randn(Cc, generator=torch.Generator().manual_seed(3)) * 0.6).float().to(dev)
    got3 = ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, quant=True, s=sm)
    ref3 = ops.rowquant(o.view(1, T * S, Cc), s=sm, fast_div=False)
    for f in ("xq", "sx", "zx", "R"):
        assert torch.equal(getattr(got3, f), getattr(ref3, f)), f


def test_attn_temporal_long_status_on_constant_rows(ops, dev):
    """All value rows zero -> every output row is zero -> delta < 1e-6 -> VQ_ST_EPSFILL, as vq_rowquant sets it."""
    T, S, H, D = 40, 3, 4, 16
    Cc = H * D
    qkv = h16(T * S, 3 * Cc, seed=9).to(dev)
    qkv[:, 2 * Cc:] = 0
    st1 = torch.zeros(1, dtype=torch.int32, device=dev)
    o = torch.empty((T * S, Cc), dtype=torch.float16, device=dev)
    got = ops.attn_temporal_long(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 1, T, S, H, D, 3 * Cc, o=o, quant=True, status=st1)
    st0 = torch.zeros(1, dtype=torch.int32, device=dev)
    ref = ops.rowquant(o.view(1, T * S, Cc), status=st0)
    assert int(st0.item()) != 0 and int(st1.item()) == int(st0.item())
    assert torch.equal(got.xq, ref.xq) and torch.equal(got.R, ref.R)


# ----------------------------------------------------------------------------- the tiny 64-frame model
def _plan(bits):
    from viditq_amd import synth
    from viditq_amd.config import loads_yaml
    txt = synth.W8A8_DYNAMIC if bits == 8 else synth.W8A8_DYNAMIC.replace("n_bits: 8", "n_bits: %d" % bits)
    return loads_yaml(txt)


def _tiny(dev, bits, T=64, depth=2):
    from viditq_amd import synth
    m = synth.build_stdit(dev, depth=depth, hidden_size=64, num_heads=4, input_size=(T, 8, 8), model_max_length=12,
                          caption_channels=32, seed=0, time_scale=2 / 3)
    qnn = synth.quantize_model(m, _plan(bits))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    return m, qnn


def _inputs(dev, T):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 4, T, 8, 8, generator=g).to(dev)
    y = (torch.randn(2, 1, 12, 32, generator=g) * 0.3).half().to(dev)
    mask = torch.ones(1, 12, dtype=torch.int64, device=dev)
    mask[0, 9:] = 0
    return x, y, mask


def _sd_of(m):
    return {k: v.detach().cpu().float() for k, v in m.state_dict().items()
            if "weight_quantizer" not in k and "act_quantizer" not in k}


@pytest.mark.parametrize("bits", [8, 6])
def test_tiny_64_frame_dispatch(dev, ops, monkeypatch, bits):
    """forward_fused launches the long temporal kernel once per block (codes mode at 8 bits, plain output + the layer's
    quantizer at 6) and never reaches the generic flash kernel for temporal attention; 16 frames never call it."""
    from viditq_amd import ops as vops
    calls = {"long": [], "fwd": []}
    orig_long, orig_fwd = vops.attn_temporal_long, vops.attn_fwd

    def long_spy(*a, **k):
        calls["long"].append(bool(k.get("quant", False)))
        return orig_long(*a, **k)

    def fwd_spy(q, k, v, o, n_seq, Lq, Lk, *a, **kw):
        calls["fwd"].append((n_seq, Lq, Lk))
        return orig_fwd(q, k, v, o, n_seq, Lq, Lk, *a, **kw)
    monkeypatch.setattr(vops, "attn_temporal_long", long_spy)
    monkeypatch.setattr(vops, "attn_fwd", fwd_spy)
    for T in (64, 16):
        _, qnn = _tiny(dev, bits, T=T)
        x, y, mask = _inputs(dev, T)
        calls["long"].clear()
        calls["fwd"].clear()
        out = qnn(x, torch.tensor([500], device=dev), y[:1], mask=mask)
        assert torch.isfinite(out).all()
        if T == 64:
            assert calls["long"] == [bits == 8] * 2, calls["long"]
            # spatial (Lq = Lk = 16 positions) and cross (Lq = 1024 tokens) only: no strided 64-frame sequences
            assert calls["fwd"] and not any(lq == T and lk == T for _, lq, lk in calls["fwd"]), calls["fwd"]
        else:
            assert calls["long"] == []
        assert qnn.check_status() == 0


@pytest.mark.parametrize("bits", [8, 6])
def test_tiny_64_frame_model_matches_reference_fixture(dev, ops, bits):
    """The reference's own QuantModel(STDiT) at 64 frames (tiny_stdit_t64.npz, time_scale 2/3): the HIP path from the
    fixture's weights (weight grids min-max, as the reference initialises them) is not further from the reference's
    fp32 output than 1.25 x the reference's own fp16 mode is, + 1e-4 (the bound of the 16-frame tiny goldens).  W8A8
    runs the fused attention + quantizer, W6A6 the plain long-kernel output + the layer's quantizer."""
    import viditq_amd  # noqa: F401
    from helpers import load_npz, state_dict_of
    from viditq_amd import synth
    from viditq_amd.t2v import STDiT
    g = load_npz("tiny_stdit_t64.npz")
    m = STDiT(dtype=torch.float16, input_size=(64, 8, 8), depth=2, hidden_size=64, num_heads=4, model_max_length=12,
              caption_channels=32, time_scale=2 / 3)
    m.load_state_dict(state_dict_of(g), strict=True)
    m = m.half().to(dev).eval()
    qnn = synth.quantize_model(m, _plan(bits))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    x, y, mask, t = g["x"].to(dev), g["y"].half().to(dev), g["mask"].to(dev), g["t"].to(dev)
    out = qnn(x, t, y[:1], mask=mask).cpu()
    tag = "w%da%d_cond" % (bits, bits)
    ref32, ref16 = g[tag], g[tag + "_ref_fp16"]
    e, drift = rel_l2(out, ref32), rel_l2(ref16, ref32)
    print("tiny 64-frame %s: HIP vs reference fp32 %.3e, reference fp16 mode vs fp32 %.3e" % (tag, e, drift))
    assert e < 1.25 * drift + 1e-4, (e, drift)
    assert qnn.check_status() == 0


def test_tiny_64_frame_graph_two_stream_step_equals_eager(dev, ops):
    """The captured 64-frame step (cond and uncond as parallel branches on two HIP streams) reproduces the eager
    forwards bit for bit, also after replay with new latent contents."""
    from viditq_amd.graph import GraphedSampler
    _, qnn = _tiny(dev, 8)
    _, y, mask = _inputs(dev, 64)
    gs = GraphedSampler(qnn, y[:1], y[1:], mask, two_streams=True)
    for seed, t_id in ((1, 721), (2, 300), (3, 721)):
        x = torch.randn(1, 4, 64, 8, 8, generator=torch.Generator().manual_seed(seed)).to(dev)
        t = torch.full((1,), t_id, device=dev, dtype=torch.long)
        cond_e = qnn(x, t, y[:1], mask=mask, timestep_id=t_id).clone()
        unc_e = qnn(x, t, y[1:], mask=mask, timestep_id=t_id).clone()
        cond_g, unc_g = gs.forward_pair(x, t_id)
        torch.cuda.synchronize()
        assert torch.equal(cond_g, cond_e) and torch.equal(unc_g, unc_e)
    assert len(gs.graphs) == 1


def test_full_size_64_frame_stdit_block_matches_oracle(dev, ops):
    """ONE STDiT-XL/2 block at 64 x 1024 tokens (64x512x512, time_scale 2/3), W8A8, through the fused HIP route vs the
    CPU oracle on identical weights."""
    import viditq_amd.t2v.stdit as st
    from viditq_amd import synth
    from viditq_amd.config import loads_yaml
    m = synth.build_stdit(dev, depth=1, input_size=(64, 64, 64), caption_channels=64, seed=11, time_scale=2 / 3)
    qnn = synth.quantize_model(m, loads_yaml(synth.W8A8_DYNAMIC))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    gx = torch.Generator().manual_seed(12)
    x = torch.randn(1, 4, 64, 64, 64, generator=gx).to(dev)
    y = (torch.randn(1, 1, 120, 64, generator=gx) * 0.3).half().to(dev)
    mask = torch.zeros(1, 120, dtype=torch.int64)
    mask[0, :97] = 1
    blocks = []
    orig = st.STDiTBlock.forward_fused

    def spy(self, x2, *a, **k):
        r = orig(self, x2, *a, **k)
        blocks.append(x2.clone())
        return r
    t = torch.tensor([721], device=dev)
    st.STDiTBlock.forward_fused = spy
    try:
        out = qnn(x, t, y, mask=mask.to(dev)).cpu()
    finally:
        st.STDiTBlock.forward_fused = orig
    cfgd = dict(T=64, S=1024, H=16, depth=1, patch=(1, 2, 2), in_ch=4, out_ch=8, input_size=(64, 64, 64))
    ref, rblocks = sr.stdit_forward(_sd_of(m), cfgd, x.cpu().half().float(), t.cpu(), y.cpu().float(), mask,
                                    sr.QSpec(w_bits=8), return_blocks=True)
    eb = rel_l2(blocks[0].cpu().float().reshape(1, 65536, 1152), rblocks[0])
    eo = rel_l2(out, ref)
    print("64-frame full-size block rel-L2 %.3e, depth-1 model %.3e" % (eb, eo))
    assert eb < 1e-3, eb
    assert eo < 1.25e-3, eo
    assert qnn.check_status() == 0

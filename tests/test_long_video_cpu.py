"""CPU-side checks of the long-video temporal attention entry point (17 <= T <= 64 frames): exported, bound, declared,
and its argument rules enforced before any device call."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vq_attn_temporal_long"


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L, L.load()


def test_long_temporal_entry_point_is_exported_bound_and_declared():
    L, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, src)
    assert hasattr(lib, NAME)
    assert NAME in L.SIGNATURES
    from viditq_amd import ops
    assert callable(ops.attn_temporal_long)


def _call(lib, B=1, T=64, S=4, H=4, D=16, Kp=128, xq=True, sx=True, o=True, ld_in=192, ld_out=64):
    one = ctypes.c_void_p(256)      # non-null, 16-byte aligned dummy: the checks must reject before any dereference
    p = lambda on: one if on else None  # noqa: E731
    return getattr(lib, NAME)(one, one, one, None, None, p(xq), p(sx), one, one, None, p(o), B, T, S, H, D, ld_in, ld_out,
                              Kp, 1.0, None)


def test_long_temporal_argument_rules_without_gpu():
    _, lib = _lib()
    nul = [None] * 11
    assert getattr(lib, NAME)(*nul, 1, 64, 4, 4, 16, 192, 64, 128, 1.0, None) == -1        # all pointers null
    assert _call(lib, T=65) == -2                       # more frames than the kernel holds
    assert _call(lib, H=17, D=16, ld_in=3 * 17 * 16, ld_out=17 * 16, Kp=384) == -2           # more than 16 heads
    assert _call(lib, sx=False) == -1                   # codes without their scales
    assert _call(lib, B=2) == -2                        # per-token grids are shared over the batch
    assert _call(lib, xq=False, o=False) == -1          # neither output
    assert _call(lib, Kp=100) == -2                     # Kp % 128
    assert _call(lib, ld_in=190) == -2                  # misaligned rows
    assert _call(lib, D=48, ld_in=3 * 4 * 48, ld_out=4 * 48, Kp=256) == -2                   # head dim without a kernel
    assert _call(lib, T=0) == -1
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)   # odd: a float view at an offset; s / s_rcp are read as float4
    assert getattr(lib, NAME)(one, one, one, odd, odd, one, one, one, one, None, one, 1, 64, 4, 4, 16, 192, 64, 128, 1.0,
                              None) == -2
    # the 16-frame entry point keeps its limit
    one = ctypes.c_void_p(16)
    assert lib.vq_attn_temporal(one, one, one, one, 1, 17, 4, 4, 72, 8, 8, 1.0, None) == -2


T64_CFG = dict(T=64, S=16, H=4, depth=2, patch=(1, 2, 2), in_ch=4, out_ch=8, input_size=(64, 8, 8))


def test_oracle_reproduces_the_64_frame_reference_fixture():
    """The CPU oracle at 64 frames (time_scale 2/3 in the reference's own pos_embed_temporal) against the reference's
    QuantModel(STDiT) outputs of tiny_stdit_t64.npz: W8A8 and W6A6 forwards, the W8A8 weight grids, and 2 DDIM steps."""
    import torch
    from helpers import load_npz, quant_params_of, rel_l2, state_dict_of
    from oracle import stdit_ref as sr
    g = load_npz("tiny_stdit_t64.npz")
    sd = state_dict_of(g)
    assert sd["pos_embed_temporal"].shape == (1, 64, 64)
    # the product's STDiT builds the reference's 2/3-scaled temporal embedding (the fixture stores it fp16-rounded)
    import viditq_amd  # noqa: F401
    from viditq_amd.t2v import STDiT
    m = STDiT(input_size=(64, 8, 8), depth=1, hidden_size=64, num_heads=4, model_max_length=12, caption_channels=32,
              time_scale=2 / 3)
    assert torch.equal(m.pos_embed_temporal.half().float(), sd["pos_embed_temporal"])
    m1 = STDiT(input_size=(64, 8, 8), depth=1, hidden_size=64, num_heads=4, model_max_length=12, caption_channels=32)
    assert not torch.equal(m1.pos_embed_temporal.half().float(), sd["pos_embed_temporal"])
    x, y, mask, t = g["x"], g["y"], g["mask"], g["t"]
    for bits in (8, 6):
        spec = sr.QSpec(w_bits=bits, a_bits=bits)
        assert rel_l2(sr.stdit_forward(sd, T64_CFG, x, t, y[:1], mask, spec), g["w%da%d_cond" % (bits, bits)]) < 1e-4
        qp = quant_params_of(g, "qp_w%da%d" % (bits, bits))
        for name, (d, z) in spec.w_grid.items():
            assert torch.equal(d, qp[name + ".weight_quantizer"]["delta"].reshape(d.shape)), name
    tmap, acp = sr.spaced_schedule(2)
    spec = sr.QSpec(w_bits=8)
    z = g["ddim_z"]
    for i in (1, 0):
        tt = torch.tensor([tmap[i]])
        cond = sr.stdit_forward(sd, T64_CFG, z, tt, y[:1], mask, spec)
        unc = sr.stdit_forward(sd, T64_CFG, z, tt, y[1:], mask, spec)
        z = sr.cfg_ddim_step(z, cond, unc, acp, i, 4.0)
    assert rel_l2(z, g["w8a8_ddim2_final"]) < 1e-4

"""CPU-side checks of vq_attn_temporal_rowquant_static (temporal attention + attn_temp.proj's static tensor-wise
quantizer): exported, bound and declared; its argument rules enforced before any device call; ops.attn_temporal_static_ok
agreeing with them; the block's route predicate; and the one-hot inputs of the GPU edge-row test staying inside their cap."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vq_attn_temporal_rowquant_static"
EINVAL, ESHAPE, EUNSUP = -1, -2, -4

# (T, S, H, D) of test_quantizer_edges_gpu.TEMPORAL: the trimmed, the generic and the long kernel
EDGE_CASES = [(16, 8, 8, 64), (5, 9, 2, 32), (16, 8, 16, 72), (17, 6, 4, 16), (64, 4, 8, 64), (64, 5, 16, 72)]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L, L.load()


def test_static_attention_entry_point_is_exported_bound_and_declared():
    L, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m, "not declared in include/viditq.h"
    assert hasattr(lib, NAME)
    assert NAME in L.SIGNATURES
    assert len(L.SIGNATURES[NAME][1]) == len(m.group(1).split(",")) == 23
    from viditq_amd import ops
    assert callable(ops.attn_temporal_rowquant_static) and callable(ops.attn_temporal_static_ok)


ONE = 256           # non-null, 16-byte aligned dummy address: the checks must reject before any dereference


def _call(lib, q=ONE, k=ONE, v=ONE, s=None, s_rcp=None, delta=ONE, zp=ONE, xq=ONE, sx=ONE, zx=ONE, R=ONE, o=None, B=1,
          T=16, S=4, H=4, D=16, ld_in=None, ld_out=None, Kp=None, n_bits=8):
    C = H * D
    ld_in = 3 * C if ld_in is None else ld_in
    ld_out = C if ld_out is None else ld_out
    Kp = (C + 127) // 128 * 128 if Kp is None else Kp
    p = lambda a: None if a is None else ctypes.c_void_p(a)  # noqa: E731
    return getattr(lib, NAME)(p(q), p(k), p(v), p(s), p(s_rcp), p(delta), p(zp), p(xq), p(sx), p(zx), p(R), p(o), B, T, S, H,
                              D, ld_in, ld_out, Kp, n_bits, 1.0, None)


@pytest.mark.parametrize("kw,want", [
    (dict(q=None), EINVAL), (dict(k=None), EINVAL), (dict(v=None), EINVAL), (dict(delta=None), EINVAL),
    (dict(zp=None), EINVAL), (dict(xq=None), EINVAL), (dict(sx=None), EINVAL), (dict(zx=None), EINVAL),
    (dict(R=None), EINVAL), (dict(s=ONE), EINVAL), (dict(s_rcp=ONE), EINVAL),
    (dict(B=0), EINVAL), (dict(T=0), EINVAL), (dict(S=0), EINVAL), (dict(H=0), EINVAL), (dict(T=65), EINVAL),
    (dict(H=17), ESHAPE), (dict(H=3, D=72, Kp=256), ESHAPE),         # H * D % 16
    (dict(Kp=100), ESHAPE), (dict(H=16, D=16, Kp=128), ESHAPE),      # Kp % 128, Kp < H * D
    (dict(D=48), ESHAPE), (dict(ld_in=190), ESHAPE),
    (dict(q=260), ESHAPE), (dict(k=264), ESHAPE), (dict(v=258), ESHAPE), (dict(xq=272 + 8), ESHAPE),
    (dict(s=260, s_rcp=ONE), ESHAPE), (dict(s=ONE, s_rcp=260), ESHAPE), (dict(o=264), ESHAPE),
    (dict(o=ONE, ld_out=72), ESHAPE),                                # T <= 16: o is dense
    (dict(o=ONE, T=17, ld_out=60), ESHAPE), (dict(o=ONE, T=17, ld_out=68), ESHAPE),   # long: ld_out >= H * D, % 8
    (dict(n_bits=1), EUNSUP), (dict(n_bits=9), EUNSUP), (dict(T=64, n_bits=0), EUNSUP),
])
def test_static_attention_argument_rules_without_gpu(kw, want):
    """Every refusal returns its code before any HIP call or dereference (the pointers are dummies, no GPU is present)."""
    _, lib = _lib()
    assert _call(lib, **kw) == want


def test_static_ok_agrees_with_the_entry_point():
    """ops.attn_temporal_static_ok mirrors the entry point's refusals over (T, H, D, Kp, n_bits).  (Only refusals are
    compared where no GPU is present: an accepted call would launch.)"""
    _, lib = _lib()
    from viditq_amd import ops
    n_ok = 0
    for T in (0, 1, 16, 17, 64, 65):
        for H in (0, 2, 3, 16, 17):
            for D in (16, 48, 72):
                for Kp in (0, 100, 128, H * D, (H * D + 127) // 128 * 128, 2048):
                    for n_bits in (1, 2, 6, 8, 9):
                        ok = ops.attn_temporal_static_ok(T, H, D, Kp, n_bits)
                        n_ok += ok
                        if not ok:
                            assert _call(lib, T=T, H=H, D=D, Kp=Kp, n_bits=n_bits) < 0, (T, H, D, Kp, n_bits)
                        else:       # what the entry point checks, restated
                            assert 1 <= T <= 64 and 1 <= H <= 16 and D in (16, 72) and (H * D) % 16 == 0
                            assert Kp % 128 == 0 and Kp >= H * D and 2 <= n_bits <= 8
    assert n_ok > 50
    assert ops.attn_temporal_static_ok(16, 16, 72, 1152, 6) and ops.attn_temporal_static_ok(64, 16, 72, 1152, 8)


def test_block_route_predicate(monkeypatch):
    _lib()
    from viditq_amd.qdiff.quantizer.dynamic_quantizer import DynamicActQuantizer
    from viditq_amd.t2v import stdit
    tw = types.SimpleNamespace(act_quantizer=types.SimpleNamespace(delta=torch.ones(1), zero_point=torch.zeros(1), n_bits=6))
    tok = types.SimpleNamespace(act_quantizer=types.SimpleNamespace(delta=torch.ones(32, 1), zero_point=torch.zeros(32, 1),
                                                                     n_bits=8))
    dyn = types.SimpleNamespace(act_quantizer=object.__new__(DynamicActQuantizer))
    if "VQ_STATIC_ATTN_QUANT" not in os.environ:
        assert stdit._STATIC_ATTN_QUANT is False                   # the default is off
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", False)
    assert not stdit._static_attn_quant(tw, 16, 16, 72)
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", True)
    assert stdit._static_attn_quant(tw, 16, 16, 72) and stdit._static_attn_quant(tw, 64, 4, 16)
    assert not stdit._static_attn_quant(dyn, 16, 16, 72)           # dynamic: today's dynamic route
    assert not stdit._static_attn_quant(tok, 16, 16, 72)           # static per-token grids: today's route
    assert not stdit._static_attn_quant(tw, 65, 16, 72) and not stdit._static_attn_quant(tw, 16, 16, 48)
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    assert not stdit._static_attn_quant(tw, 16, 16, 72)


@pytest.mark.parametrize("T,S,H,D", EDGE_CASES)
def test_edge_row_inputs_stay_inside_their_cap(T, S, H, D):
    """The one-hot q / k of the GPU edge-row test: at least 0.9 of the rows have every head's lead >= R1_GAP."""
    import attn_regimes as ar
    import quant_rows as qr
    scale = D ** -0.5
    q, k, hot = qr.one_hot_qk(S, T, H, D, scale, seed=100 * T + D)
    gp = ar.gaps(q, k, hot[:, :, None].expand(S, T, H).contiguous(), scale, [T] * S)
    sel = (gp >= ar.R1_GAP).all(-1)
    assert float(sel.double().mean()) >= 0.9

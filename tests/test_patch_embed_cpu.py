"""vq_patch_embed_f16's refusals, in their order, before any device call (dummy addresses), and ops.patch_embed_f16_ok beside them."""
import ctypes
import os

import pytest
import torch

EINVAL, ESHAPE, EUNSUP, ONE = -1, -2, -4, 1 << 20      # ONE: a non-null, 16-byte aligned dummy DEVICE address
BASE = dict(B=2, Cin=4, D=1, H=6, W=10, pt=1, ph=2, pw=2, C=96, rows=15, ldw=16)
PTRS = ("x", "w", "bias", "pos", "out")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L.load()


def _call(lib, f32=1, **kw):
    a = {**BASE, **dict.fromkeys(PTRS, ONE), **kw}
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    return lib.vq_patch_embed_f16(p(a["x"]), f32, p(a["w"]), p(a["bias"]), p(a["pos"]), p(a["out"]), a["B"], a["Cin"], a["D"],
                                  a["H"], a["W"], a["pt"], a["ph"], a["pw"], a["C"], a["rows"], a["ldw"], None)


CASES = [   # in the entry point's order; the last two rows: pairs that show which of two refusals comes first
    (dict(x=None), EINVAL), (dict(w=None), EINVAL), (dict(out=None), EINVAL),
    (dict(B=0), EINVAL), (dict(Cin=-4), EINVAL), (dict(D=0), EINVAL), (dict(H=0), EINVAL), (dict(W=-10), EINVAL),
    (dict(pt=0), EINVAL), (dict(ph=0), EINVAL), (dict(pw=-2), EINVAL), (dict(C=0), EINVAL), (dict(ldw=0), EINVAL),
    (dict(rows=0), EINVAL), (dict(rows=-15), EINVAL),
    (dict(D=3, pt=2, Cin=2), ESHAPE), (dict(H=7), ESHAPE), (dict(W=11), ESHAPE),                       # padding needed
    (dict(Cin=3), ESHAPE), (dict(Cin=16), ESHAPE), (dict(Cin=1 << 30, ph=1 << 15, pw=1 << 15, H=1 << 15, W=1 << 15), ESHAPE),
    (dict(C=88), ESHAPE), (dict(C=1552), ESHAPE), (dict(rows=4), ESHAPE), (dict(rows=30), ESHAPE),
    (dict(B=1 << 20, H=64, W=64, rows=1024), ESHAPE),                                                  # 2^32 elements
    (dict(ldw=20), ESHAPE), (dict(ldw=8), ESHAPE),
    (dict(x=ONE + 8), ESHAPE), (dict(w=ONE + 2), ESHAPE), (dict(bias=ONE + 8), ESHAPE), (dict(pos=ONE + 4), ESHAPE),
    (dict(out=ONE + 8), ESHAPE), (dict(f32=2), EUNSUP), (dict(f32=-1), EUNSUP),
    (dict(x=None, H=7), EINVAL), (dict(B=0, C=88), EINVAL), (dict(rows=0, W=11), EINVAL),
    (dict(C=88, f32=2), ESHAPE), (dict(ldw=20, f32=2), ESHAPE), (dict(out=ONE + 8, f32=2), ESHAPE),
]


@pytest.mark.parametrize("kw,want", CASES)
def test_refusals_and_their_order_without_gpu(kw, want):
    lib = _lib()
    assert _call(lib, **kw) == want
    from viditq_amd import ops
    if not any(k in kw for k in PTRS + ("f32",)):                    # (pointers and the type flag stay with the entry point)
        a = dict(BASE, **kw)
        assert not ops.patch_embed_f16_ok(a["B"], a["Cin"], a["D"], a["H"], a["W"], (a["pt"], a["ph"], a["pw"]), a["C"], a["rows"],
                                          a["ldw"])


def test_wrapper_refuses_cpu_tensors_and_the_switch_is_off_by_default():
    lib = _lib()
    assert _call(lib, pos=None, rows=0, H=7) == ESHAPE and _call(lib, x=None, B=0, f32=7) == EINVAL     # pos_rows without pos
    from viditq_amd import ops
    from viditq_amd.t2v import stdit
    with pytest.raises(ops.VQError):
        ops.patch_embed_f16(torch.zeros(1, 4, 4, 4), torch.zeros(32, 16, dtype=torch.float16), patch=(2, 2))
    ok = ops.patch_embed_f16_ok
    assert ok(2, 4, 1, 6, 10, (1, 2, 2), 96, 15, 16) and ok(1, 4, 4, 4, 4, (2, 2, 2), 1536, None, 40) and ok(1, 2, 1, 2, 2, (1, 2, 2), 16, 1, 8)
    if "VQ_PATCH_EMBED_FUSED" not in os.environ:
        assert stdit._PATCH_EMBED_FUSED is False

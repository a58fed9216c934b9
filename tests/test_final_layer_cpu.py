"""CPU-side checks of vq_final_layer_f16 (csrc/final_layer.hip): its refusals, in their order, before any device call -
the addresses are dummies that are never dereferenced - and ops.final_layer_f16_ok agreeing with them."""
import ctypes

import pytest
import torch

EINVAL, ESHAPE, ONE = -1, -2, 1 << 20      # ONE: a non-null, 16-byte aligned dummy DEVICE address


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L.load()


def _call(lib, x=ONE, shift=ONE, scale=ONE, w=ONE, bias=ONE, out=ONE, M=30, R=15, C=1152, N=32, ldx=None, ldw=None):
    p = lambda a: None if a is None else ctypes.c_void_p(a)  # noqa: E731
    return lib.vq_final_layer_f16(p(x), p(shift), p(scale), 1e-6, p(w), p(bias), p(out), M, R, C, N, C if ldx is None else ldx,
                                  C if ldw is None else ldw, None)


CASES = [   # in the entry point's order: null pointers (a null bias falls through to the LAST check), extents, M % R,
    # the shapes served, the pitches, a pointer off 16 bytes; then pairs that show which of two refusals comes first
    (dict(x=None), EINVAL), (dict(shift=None), EINVAL), (dict(scale=None), EINVAL), (dict(w=None), EINVAL),
    (dict(out=None), EINVAL), (dict(bias=None, out=ONE + 8), ESHAPE),
    (dict(M=0), EINVAL), (dict(M=-16), EINVAL), (dict(R=0), EINVAL), (dict(C=0), EINVAL), (dict(N=0), EINVAL),
    (dict(N=-16), EINVAL), (dict(ldx=0), EINVAL), (dict(ldw=-8), EINVAL), (dict(M=31), EINVAL), (dict(M=15, R=30), EINVAL),
    (dict(C=1144), ESHAPE), (dict(C=16), ESHAPE), (dict(C=1568), ESHAPE), (dict(N=24), ESHAPE), (dict(N=80), ESHAPE),
    (dict(ldx=1156), ESHAPE), (dict(ldw=1156), ESHAPE), (dict(ldx=1144), ESHAPE), (dict(ldw=1024), ESHAPE),
    (dict(x=ONE + 8), ESHAPE), (dict(shift=ONE + 4), ESHAPE), (dict(scale=ONE + 8), ESHAPE), (dict(w=ONE + 2), ESHAPE),
    (dict(bias=ONE + 8), ESHAPE), (dict(out=ONE + 8), ESHAPE),
    (dict(x=None, C=1144), EINVAL), (dict(w=None, M=0), EINVAL), (dict(M=0, N=24), EINVAL), (dict(R=0, x=ONE + 8), EINVAL),
    (dict(M=31, C=1144), EINVAL), (dict(M=31, ldx=1156), EINVAL), (dict(M=31, out=ONE + 8), EINVAL),
]


@pytest.mark.parametrize("kw,want", CASES)
def test_refusals_and_their_order_without_gpu(kw, want):
    lib = _lib()
    assert _call(lib, **kw) == want
    from viditq_amd import ops
    if not any(k in kw for k in ("x", "shift", "scale", "w", "bias", "out")):         # (pointers stay with the entry point)
        a = dict(dict(M=30, R=15, C=1152, N=32), **kw)
        assert not ops.final_layer_f16_ok(a["M"], a["R"], a["C"], a["N"], a.get("ldx", a["C"]), a.get("ldw", a["C"]))


def test_wrapper_refuses_cpu_tensors_and_the_switch_is_off_by_default():
    _lib()
    import os
    from viditq_amd import ops
    from viditq_amd.t2v import stdit
    with pytest.raises(ops.VQError):
        ops.final_layer_f16(torch.zeros(1, 4, 64, dtype=torch.float16), torch.zeros(1, 64), torch.zeros(1, 64), 1e-6,
                            torch.zeros(32, 64, dtype=torch.float16))
    assert ops.final_layer_f16_ok(30, 15, 1152, 32, 1152, 1152) and ops.final_layer_f16_ok(1, 1, 32, 16, 40, 32)
    if "VQ_FINAL_FUSED" not in os.environ:
        assert stdit._FINAL_FUSED is False

"""CPU-side checks of vq_final_layer_i8 (csrc/final_layer_i8.hip): its refusals, in their order, before any device call -
the addresses are dummies that are never dereferenced - and ops.final_layer_i8_ok agreeing with them."""
import ctypes

import pytest
import torch

EINVAL, ESHAPE, EUNSUP, ONE = -1, -2, -4, 1 << 20      # ONE: a non-null, 16-byte aligned dummy DEVICE address
PTRS = ("x", "shift", "scale", "s", "s_rcp", "wq", "sw", "zw", "cs", "bias", "out", "status")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L.load()


def _call(lib, M=30, R=15, C=1152, Kp=None, N=32, ldx=None, nb=8, wb=8, **ptr):
    p = lambda a: None if a is None else ctypes.c_void_p(a)  # noqa: E731
    a = [p(ptr.get(k, ONE)) for k in PTRS]
    return lib.vq_final_layer_i8(*a[:3], 1e-6, *a[3:], M, R, C, (C + 127) // 128 * 128 if Kp is None else Kp, N,
                                 C if ldx is None else ldx, nb, wb, None)


CASES = [   # in the entry point's order: null pointers (the optional ones fall through to the LAST check), extents, M % R,
    # the shapes served with the batch, the pitch, the widths, a pointer off 16 bytes; then pairs that show which comes first
    (dict(x=None), EINVAL), (dict(shift=None), EINVAL), (dict(scale=None), EINVAL), (dict(wq=None), EINVAL),
    (dict(sw=None), EINVAL), (dict(zw=None), EINVAL), (dict(cs=None), EINVAL), (dict(out=None), EINVAL),
    (dict(s=None), EINVAL), (dict(s=None, s_rcp=None, bias=None, status=None, out=ONE + 8), ESHAPE),
    (dict(M=0), EINVAL), (dict(M=-16), EINVAL), (dict(R=0), EINVAL), (dict(C=0), EINVAL), (dict(Kp=0), EINVAL),
    (dict(N=0), EINVAL), (dict(ldx=0), EINVAL), (dict(M=31), EINVAL), (dict(M=15, R=30), EINVAL),
    (dict(C=1144), ESHAPE), (dict(C=16), ESHAPE), (dict(C=1568), ESHAPE), (dict(Kp=1280), ESHAPE), (dict(C=96, Kp=96), ESHAPE),
    (dict(N=24), ESHAPE), (dict(N=80), ESHAPE), (dict(M=45), ESHAPE), (dict(M=480, R=15), ESHAPE),
    (dict(ldx=1156), ESHAPE), (dict(ldx=1144), ESHAPE),
    (dict(nb=1), EUNSUP), (dict(nb=9), EUNSUP), (dict(wb=1), EUNSUP), (dict(wb=9), EUNSUP),
    (dict(x=ONE + 8), ESHAPE), (dict(shift=ONE + 4), ESHAPE), (dict(scale=ONE + 8), ESHAPE), (dict(s=ONE + 4), ESHAPE),
    (dict(s_rcp=ONE + 8), ESHAPE), (dict(wq=ONE + 2), ESHAPE), (dict(sw=ONE + 4), ESHAPE), (dict(zw=ONE + 8), ESHAPE),
    (dict(cs=ONE + 4), ESHAPE), (dict(bias=ONE + 8), ESHAPE), (dict(out=ONE + 8), ESHAPE), (dict(status=ONE + 4), ESHAPE),
    (dict(x=None, C=1144), EINVAL), (dict(s=None, M=45), EINVAL), (dict(M=0, N=24), EINVAL), (dict(R=0, x=ONE + 8), EINVAL),
    (dict(M=31, C=1144), EINVAL), (dict(M=31, nb=9), EINVAL), (dict(M=45, ldx=1156), ESHAPE), (dict(M=45, nb=9), ESHAPE),
    (dict(ldx=1156, wb=9), ESHAPE), (dict(nb=9, out=ONE + 8), EUNSUP), (dict(wb=1, C=1144), ESHAPE),
]


@pytest.mark.parametrize("kw,want", CASES)
def test_refusals_and_their_order_without_gpu(kw, want):
    lib = _lib()
    assert _call(lib, **kw) == want
    from viditq_amd import ops
    if not any(k in kw for k in PTRS):                                                 # (pointers stay with the entry point)
        a = dict(dict(M=30, R=15, C=1152, N=32, nb=8, wb=8), **kw)
        Kp = a.get("Kp", (a["C"] + 127) // 128 * 128)
        assert not ops.final_layer_i8_ok(a["M"], a["R"], a["C"], Kp, a["N"], a.get("ldx", a["C"]), a["nb"], a["wb"])


def test_wrapper_refuses_cpu_tensors_and_the_switch_is_off_by_default():
    _lib()
    import os
    from viditq_amd import ops
    from viditq_amd.t2v import stdit
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    pw = ops.PackedWeight(torch.zeros(32, 128, dtype=torch.int8), torch.ones(32), i32(32), i32(32), 32, 64, 128, 8)
    with pytest.raises(ops.VQError):
        ops.final_layer_i8(torch.zeros(1, 4, 64, dtype=torch.float16), torch.zeros(1, 64), torch.zeros(1, 64), 1e-6, pw)
    assert ops.final_layer_i8_ok(30, 15, 1152, 1152, 32, 1152, 8, 4) and ops.final_layer_i8_ok(16, 1, 32, 128, 16, 40, 2, 2)
    if "VQ_FINAL_QUANT_FUSED" not in os.environ:
        assert stdit._FINAL_QUANT_FUSED is False

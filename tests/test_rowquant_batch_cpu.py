"""CPU-side checks of vq_rowquant_batch (one-pass per-token quantizers of a batched forward, 3 <= B <= 16): declared, exported
and bound; its refusals, in their order, before any device call; ops.rowquant_batch_ok agreeing with them; the wrappers
refusing CPU tensors; and the LayerNorm references of the GPU test staying inside the checker's caps."""
import ctypes
import functools

import pytest
import torch

import ln_cases as lc

NAME = "vq_rowquant_batch"
EINVAL, ESHAPE, EUNSUP = -1, -2, -4
ONE = 1 << 20       # non-null, 16-byte aligned dummy DEVICE address: the checks must reject before any dereference
LN_SHAPES = [(3, 1152), (4, 768), (5, 1280), (8, 1152), (16, 64), (16, 1024), (16, 1152)]


@functools.lru_cache(maxsize=None)
def ln_reference(B, n, C, eps=1e-6):
    """(x, shift, scale, smooth, Reference at 8 bits) of one LayerNorm launch of the GPU test: mixed rows, no vector + two."""
    x, shift, scale, names = lc.mixed(B, n, C)
    smooth = [None] + lc.smooth_vectors(C, 2)
    return x, shift, scale, smooth, lc.Reference(x, shift, scale, eps, 8, smooth, names)


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L, L.load()


def _call(lib, x=ONE, shift=None, scale=None, act=0, n_out=1, xm=None, B=4, n_tok=5, C=1152, Kp=None, n_bits=8, **arrays):
    keep = []
    for name in ("s", "s_rcp", "xq", "sx", "zx", "R"):
        vals = arrays.get(name, None if name in ("s", "s_rcp") else [ONE] * 3)
        keep.append(None if vals is None else ctypes.cast((ctypes.c_void_p * 3)(*vals), ctypes.c_void_p))
    return getattr(lib, NAME)(x, shift, scale, 1e-6, act, n_out, *keep, xm, B, n_tok, C, C if Kp is None else Kp, n_bits, None,
                              None)


CASES = [
    # 1. VQ_EINVAL
    (dict(x=None), EINVAL), (dict(xq=None), EINVAL), (dict(R=[None, ONE, ONE]), EINVAL), (dict(shift=ONE), EINVAL),
    (dict(act=1, shift=ONE, scale=ONE), EINVAL), (dict(act=2), EINVAL), (dict(xm=ONE), EINVAL), (dict(n_out=0), EINVAL),
    (dict(B=0), EINVAL), (dict(n_tok=0), EINVAL), (dict(C=0, Kp=128), EINVAL),
    # 2. the shape, the code width, then 16-byte alignment
    (dict(C=1150, Kp=1152), ESHAPE), (dict(Kp=1100), ESHAPE), (dict(n_bits=9), EUNSUP), (dict(x=ONE + 8), ESHAPE),
    (dict(s=[ONE + 4, None, None]), ESHAPE), (dict(s=[ONE] * 3, s_rcp=[ONE + 8, ONE, ONE]), ESHAPE), (dict(xq=[ONE + 8, ONE, ONE]), ESHAPE),
    # 3. B > 16, 4. what the kernels do not hold
    (dict(B=17), ESHAPE), (dict(B=2), EUNSUP), (dict(B=1), EUNSUP), (dict(C=4736), EUNSUP), (dict(n_out=4), EUNSUP),
    (dict(act=1, n_out=2), EUNSUP), (dict(shift=ONE, scale=ONE, C=4608), EUNSUP),
    # the order
    (dict(x=None, C=1150), EINVAL), (dict(B=0, x=ONE + 8), EINVAL), (dict(C=1150, Kp=1152, B=17), ESHAPE),
    (dict(x=ONE + 8, B=17), ESHAPE), (dict(x=ONE + 8, B=2), ESHAPE), (dict(B=17, C=4736), ESHAPE), (dict(n_bits=9, B=17), EUNSUP),
]


@pytest.mark.parametrize("kw,want", CASES)
def test_refusals_in_their_order_without_gpu(kw, want):
    L, lib = _lib()
    assert NAME in L.SIGNATURES and len(L.SIGNATURES[NAME][1]) == 20 and hasattr(lib, NAME)
    assert _call(lib, **kw) == want


def test_batch_ok_agrees_with_the_entry_point():
    """Where the predicate refuses, the entry point refuses (aligned dummies: nothing may be launched); where it accepts,
    the same call with x off 16 bytes comes back VQ_ESHAPE - the second group of checks, so the first passed - and the
    table above holds the third and fourth."""
    _, lib = _lib()
    from viditq_amd import ops
    n_ok, codes = 0, set()
    for B in (1, 2, 3, 16, 17):
        for C, Kp in ((64, 128), (1152, 1152), (1150, 1152), (4608, 4608), (4736, 4736)):
            for n_bits in (1, 4, 8):
                for n_out, act, ln in ((1, 0, False), (3, 0, False), (4, 0, False), (1, 1, False), (2, 1, False), (3, 0, True)):
                    kw = dict(B=B, C=C, Kp=Kp, n_bits=n_bits, n_out=n_out, act=act, **(dict(shift=ONE, scale=ONE) if ln else {}))
                    if ops.rowquant_batch_ok(B, C, Kp, n_bits, n_out, act, ln):
                        n_ok += 1
                        assert _call(lib, x=ONE + 8, **kw) == ESHAPE, kw
                    else:
                        codes.add(_call(lib, **kw))
    assert n_ok == 2 * 2 * (3 * 3 + 2) and codes == {ESHAPE, EUNSUP}, (n_ok, codes)   # B 3 / 16, 4 / 8 bits; C 4608: no LN arm


def test_wrappers_refuse_cpu_tensors(monkeypatch):
    _lib()
    from viditq_amd import _lib as L, ops
    monkeypatch.setattr(L, "load", lambda *a, **k: pytest.fail("a CPU tensor got as far as the library"))
    x, v = torch.zeros(4, 5, 64, dtype=torch.float16), torch.ones(4, 64)
    for call in (lambda: ops.rowquant_batch(x, 8, [v[0]]), lambda: ops.gelu_rowquant_batch(x, 8, None),
                 lambda: ops.ln_modulate_rowquant_batch(x, v, v)):
        with pytest.raises(ops.VQError):
            call()
    from viditq_amd.t2v import stdit
    assert stdit._BATCH_QUANT is False or "VQ_BATCH_QUANT" in __import__("os").environ


@pytest.mark.parametrize("B,C", LN_SHAPES)
def test_ln_references_stay_inside_the_caps(B, C):
    """The references alone: finite, small margins and shares of two-valued elements under the checker's caps, at both code
    widths of the GPU test."""
    for n, eps in ((9, 1e-6), (1, 1e-6)) + (((9, 1e-5),) if (B, C) == (8, 1152) else ()):
        ref8 = ln_reference(B, n, C, eps)[4]
        for ref in (ref8, ref8.rebits(4)):
            assert ref.finite_and_small()
            assert ref.xm_share() <= lc._cap(ref.u64.numel()) and ref.xm_share(True) <= lc.XM_ILL_CAP
            assert all(ref.code_share(j) <= lc._cap(ref.u64.numel()) for j in range(3))

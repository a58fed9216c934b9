"""CPU-side checks of vq_rowquant_smooth_multi_shared (the smoothed q | k | v quantizers of a joint cond | uncond forward
from one pass over the rows, plain or behind LayerNorm + modulate): declared, exported and bound alike; its argument rules
enforced, in their order, before any device call; ops.rowquant_multi_shared_ok agreeing with them; the block's switch off
by default and its route predicate; and the edge rows of the GPU test staying clean behind each of its three vectors."""
import ctypes
import os
import re
import types

import pytest
import torch

import quant_rows as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vq_rowquant_smooth_multi_shared"
EINVAL, ESHAPE, EUNSUP = -1, -2, -4
WIDTHS = (768, 1024, 1152, 1280)


def vectors(C):
    """The three smoothing vectors of the GPU test, as test_smoothed_outputs_of_one_pass_edges builds them: the Q2 vector
    (near ties), the same with its perturbations mirrored, and a wide one."""
    s0 = qr.q2_smooth(C)
    return [s0, (2.0 - s0.double()).float(), torch.exp(torch.randn(C, generator=torch.Generator().manual_seed(3)) * 0.7).float()]


def edge_rows(C, n_bits):
    """(exact, flagged) of the GPU test at B = 2: launch_sets behind the Q2 vector, the exact rows then filtered behind
    each of the three vectors in turn."""
    exact, flagged, _ = qr.launch_sets(2, C, n_bits, s=qr.q2_smooth(C), q3_stride=49, fixed=True)
    n0 = exact.shape[1]
    for v in vectors(C):
        exact = exact[:, qr.split_eps(exact, n_bits, v)[0]]
    return exact.contiguous(), flagged, n0


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L, L.load()


def test_entry_point_is_declared_exported_and_bound_alike():
    L, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m, "not declared in include/viditq.h"
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    res, kinds = L.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(kinds) == len(params) == 18

    def kind(decl):
        if "*" in decl:
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}[decl.split()[0]]
    assert [kind(p) for p in params] == list(kinds)
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "x", "shift", "scale", "ln_eps", "n_out", "s", "s_rcp", "xq", "sx", "zx", "R", "B", "n_tok", "C", "Kp", "n_bits",
        "status", "stream"]
    from viditq_amd import ops
    assert callable(ops.rowquant_multi_shared) and callable(ops.rowquant_multi_shared_ok)
    # the header comment cites the reference lines the entry replaces
    doc = re.findall(r"/\*(.*?)\*/\s*int\s+%s\s*\(" % NAME, open(os.path.join(ROOT, "include", "viditq.h")).read(), re.S)
    assert doc and "base_quantizer.py" in doc[-1].split("/*")[-1] and "stdit.py" in doc[-1].split("/*")[-1]


ONE = 1 << 20       # non-null, 16-byte aligned dummy DEVICE address: the checks must reject before any dereference
ARRAYS = ("s", "s_rcp", "xq", "sx", "zx", "R")


def _call(lib, x=ONE, shift=None, scale=None, n_out=3, B=2, n_tok=4, C=1152, Kp=None, n_bits=8, **arrays):
    """The entry point with dummy device addresses.  ``arrays``: name -> None (a null HOST array) or a list of addresses."""
    Kp = C if Kp is None else Kp
    keep = []
    for name in ARRAYS:
        vals = arrays.get(name, [ONE] * 3)
        keep.append(None if vals is None else (ctypes.c_void_p * 3)(*[None if v is None else ctypes.c_void_p(v) for v in vals]))
    p = lambda a: None if a is None else ctypes.c_void_p(a)  # noqa: E731
    return getattr(lib, NAME)(p(x), p(shift), p(scale), 1e-6, n_out, *[None if k is None else ctypes.cast(k, ctypes.c_void_p)
                                                                     for k in keep], B, n_tok, C, Kp, n_bits, None, None)


CASES = [
    # 1. VQ_EINVAL: a null required pointer or array, a null entry below n_out, one of shift / scale, a count or extent
    (dict(x=None), EINVAL), (dict(s=None), EINVAL), (dict(s_rcp=None), EINVAL), (dict(xq=None), EINVAL),
    (dict(sx=None), EINVAL), (dict(zx=None), EINVAL), (dict(R=None), EINVAL),
    (dict(s=[ONE, None, ONE]), EINVAL), (dict(s_rcp=[ONE, ONE, None]), EINVAL), (dict(xq=[None, ONE, ONE]), EINVAL),
    (dict(sx=[ONE, None, ONE]), EINVAL), (dict(zx=[ONE, ONE, None]), EINVAL), (dict(R=[None, ONE, ONE]), EINVAL),
    (dict(shift=ONE), EINVAL), (dict(scale=ONE), EINVAL),
    (dict(n_out=0), EINVAL), (dict(n_out=4), EINVAL), (dict(n_out=-1), EINVAL),
    (dict(B=0), EINVAL), (dict(B=-2), EINVAL), (dict(n_tok=0), EINVAL), (dict(C=0, Kp=128), EINVAL), (dict(C=-8, Kp=128), EINVAL),
    # 2. the shape and the code width, as rq_check_shape returns them
    (dict(C=1150, Kp=1152), ESHAPE), (dict(Kp=1100), ESHAPE), (dict(Kp=1024), ESHAPE), (dict(Kp=0), ESHAPE),
    (dict(n_bits=1), EUNSUP), (dict(n_bits=9), EUNSUP), (dict(n_bits=0), EUNSUP),
    # 3. VQ_ESHAPE: a pointer off 16 bytes
    (dict(x=ONE + 8), ESHAPE), (dict(x=ONE + 2), ESHAPE), (dict(s=[ONE, ONE + 4, ONE]), ESHAPE),
    (dict(s_rcp=[ONE + 8, ONE, ONE]), ESHAPE), (dict(xq=[ONE, ONE, ONE + 8]), ESHAPE),
    # 4. VQ_EUNSUP: what the pair kernel does not cover
    (dict(B=1), EUNSUP), (dict(B=3), EUNSUP), (dict(C=896), EUNSUP), (dict(C=64, Kp=128), EUNSUP), (dict(C=1408), EUNSUP),
    (dict(Kp=1280), EUNSUP), (dict(C=4608), EUNSUP),
    # an entry at or above n_out is not read
    (dict(n_out=1, s=[ONE, None, None], xq=[ONE, None, ONE + 8], B=1), EUNSUP),
    # the order: 1 before 2 before 3 before 4
    (dict(x=None, C=1150), EINVAL), (dict(s=[None, ONE, ONE], n_bits=9), EINVAL), (dict(shift=ONE, Kp=1100), EINVAL),
    (dict(n_out=4, B=3), EINVAL), (dict(B=0, x=ONE + 8), EINVAL),
    (dict(n_bits=9, x=ONE + 8), EUNSUP), (dict(C=1150, Kp=1152, B=3), ESHAPE), (dict(n_bits=9, C=1150, Kp=1152), ESHAPE),
    (dict(x=ONE + 8, B=1), ESHAPE), (dict(xq=[ONE + 8, ONE, ONE], C=896), ESHAPE), (dict(s=[ONE, ONE, ONE + 4], Kp=1280), ESHAPE),
    (dict(n_bits=9, B=1), EUNSUP),
]


@pytest.mark.parametrize("kw,want", CASES)
def test_argument_rules_without_gpu(kw, want):
    """Every refusal returns its code before any HIP call or dereference of a device pointer (the addresses are dummies,
    no GPU is needed), and the four groups of checks run in their order."""
    _, lib = _lib()
    assert _call(lib, **kw) == want


def _spec(B, n_tok, C, Kp, n_bits, n_out):
    """What include/viditq.h says of these six arguments (aligned non-null pointers, no LayerNorm): a code, or None = taken."""
    if not 1 <= n_out <= 3 or B <= 0 or n_tok <= 0 or C <= 0:
        return EINVAL
    if C % 8 or Kp % 128 or Kp < C:
        return ESHAPE
    if not 2 <= n_bits <= 8:
        return EUNSUP
    if B != 2 or C not in WIDTHS or Kp != C:
        return EUNSUP
    return None


def test_shared_ok_agrees_with_the_entry_point():
    """ops.rowquant_multi_shared_ok is true exactly where the header's rules take the launch, and the entry point returns
    the header's code wherever they refuse.  A taken launch is not made on dummy addresses: there the same arguments with x
    off 16 bytes must come back VQ_ESHAPE - the third group of checks, so the first two passed."""
    _, lib = _lib()
    from viditq_amd import ops
    n_ok, codes = 0, {EINVAL: 0, ESHAPE: 0, EUNSUP: 0}
    for B in (1, 2, 3):
        for C in (64, 768, 896, 1152, 1280, 1408):
            for Kp in (C, C + 128):
                for n_bits in (1, 2, 6, 8, 9):
                    for n_out in (0, 1, 3, 4):
                        want = _spec(B, 5, C, Kp, n_bits, n_out)
                        assert ops.rowquant_multi_shared_ok(B, 5, C, Kp, n_bits, n_out) == (want is None), (B, C, Kp, n_bits, n_out)
                        if want is None:
                            n_ok += 1
                            assert _call(lib, x=ONE + 8, B=B, n_tok=5, C=C, Kp=Kp, n_bits=n_bits, n_out=n_out) == ESHAPE
                        else:
                            codes[want] += 1
                            assert _call(lib, B=B, n_tok=5, C=C, Kp=Kp, n_bits=n_bits, n_out=n_out) == want, (B, C, Kp, n_bits, n_out)
    assert n_ok == 3 * 3 * 2 and all(codes.values()), (n_ok, codes)      # three widths of the sweep, bits 2 / 6 / 8, one or three outputs
    good = dict(B=2, n_tok=1, Cc=1152, Kp=1152, n_bits=6, n_out=3)
    assert ops.rowquant_multi_shared_ok(**good) and ops.rowquant_multi_shared_ok(**dict(good, Cc=1024, Kp=1024, n_out=2))
    for bad in (dict(B=1), dict(B=3), dict(B=0), dict(n_tok=0), dict(Cc=896, Kp=896), dict(Cc=1150), dict(Kp=1280), dict(Kp=1100),
                dict(n_bits=1), dict(n_bits=9), dict(n_out=0), dict(n_out=4), dict(Cc=4608, Kp=4608), dict(Cc=0)):
        assert not ops.rowquant_multi_shared_ok(**dict(good, **bad)), bad


def test_wrapper_refuses_cpu_tensors():
    """No CPU / eager fallback: ops.rowquant_multi_shared raises on a CPU tensor, as every wrapper of the operator layer."""
    _lib()
    from viditq_amd import ops
    for C in (896, 1152):
        with pytest.raises(ops.VQError):
            ops.rowquant_multi_shared(torch.zeros(2, 4, C, dtype=torch.float16), [torch.ones(C)])


def _layer(n_bits=8, dynamic=True):
    from viditq_amd.qdiff.quantizer import ActQuantizer, DynamicActQuantizer
    aq = object.__new__(DynamicActQuantizer if dynamic else ActQuantizer)     # (the predicate reads the class and n_bits only)
    object.__setattr__(aq, "__dict__", {"n_bits": n_bits})
    return types.SimpleNamespace(act_quantizer=aq)


def test_switch_is_off_by_default_and_the_route_predicate(monkeypatch):
    _lib()
    from viditq_amd.t2v import stdit
    if "VQ_SMOOTH_JOINT" not in os.environ:
        assert stdit._SMOOTH_JOINT is False
    assert isinstance(stdit._SMOOTH_JOINT, bool)
    s = torch.ones(8)
    three = [_layer(), _layer(), _layer()]
    monkeypatch.setattr(stdit, "_SMOOTH_JOINT", False)
    assert not stdit._smooth_joint(three, [s, s, s], 2)
    monkeypatch.setattr(stdit, "_SMOOTH_JOINT", True)
    assert stdit._smooth_joint(three, [s, s, s], 2)
    assert stdit._smooth_joint([_layer(6), _layer(6), _layer(6)], [s, s, s], 2)
    assert not stdit._smooth_joint(three, [s, s, s], 1)                                  # B = 1: rowquant_multi's
    assert not stdit._smooth_joint(three, [s, s, s], 3)
    assert not stdit._smooth_joint([_layer(8), _layer(6), _layer(8)], [s, s, s], 2)      # mixed bit widths
    assert not stdit._smooth_joint(three, [s, None, s], 2)                               # a missing vector
    assert not stdit._smooth_joint(three, [None, None, None], 2)
    assert not stdit._smooth_joint([_layer(), _layer(dynamic=False), _layer()], [s, s, s], 2)   # a static quantizer
    assert not stdit._smooth_joint(three, [s, s, s], 2, add_rows=True)                   # block 0's x + tpe


@pytest.mark.parametrize("n_bits,n_rows", [(8, 781), (6, 821)])
@pytest.mark.parametrize("C", [1152, 768])
def test_edge_rows_stay_clean_behind_every_vector(C, n_bits, n_rows):
    """Every exact row of launch_sets(B = 2) behind the Q2 vector is also clean (delta >= 1e-6 by the oracle's own fp32
    delta) behind the mirrored and the wide vector - none is left out of the GPU test - and every flagged launch stays
    flagged behind the Q2 vector, which every launch of the GPU test holds."""
    from oracle import fakequant as fq
    exact, flagged, n0 = edge_rows(C, n_bits)
    assert exact.shape[1] == n0 == n_rows, (exact.shape[1], n0)
    assert len(flagged) >= 3
    s0 = qr.q2_smooth(C)
    for x in flagged:
        assert x.shape[1] == 65 and fq.dyn_act_quant(qr.smoothed(x, s0), n_bits)[4]

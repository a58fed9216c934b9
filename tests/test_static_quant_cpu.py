"""vq_rowquant_static at the boundary, without a GPU: the symbol and its binding, every error code of its contract
(include/viditq.h) returned before anything is dereferenced or launched, and the host's refusal mirror
(ops.rowquant_static_ok) against the entry point's own answer.

No call here can reach a launch: each either violates the contract, or carries a null OUTPUT pointer in the host array
of output 0 - the entry point looks at those last, after every refusal a shape can earn, and returns VQ_EINVAL."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE, EUNSUP = -1, -2, -4
GOOD, BAD = 1 << 20, (1 << 20) + 8          # a 16-byte aligned dummy device address, and one 8 bytes off


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    return _lib.load()


def _arr(*vals):
    vals = list(vals) + [None] * (3 - len(vals))
    return (C.c_void_p * 3)(*[None if v is None else C.c_void_p(v) for v in vals])


def _call(lib, keep=None, **kw):
    """One call with consistent defaults (B 1, n_tok 4, C 64, Kp 128, 8 bits, one output, no arm, dummy pointers) and the
    overrides of ``kw``; host arrays are real arrays of dummy device addresses."""
    a = dict(x=GOOD, add_rows=None, n_add=0, add_div=1, shift=None, scale=None, ln_eps=1e-6, n_out=1, s=None, s_rcp=None,
             delta=_arr(GOOD, GOOD, GOOD), zp=_arr(GOOD, GOOD, GOOD), n_param=1, xq=_arr(GOOD, GOOD, GOOD),
             sx=_arr(GOOD, GOOD, GOOD), zx=_arr(GOOD, GOOD, GOOD), R=_arr(GOOD, GOOD, GOOD), xm_out=None, B=1, n_tok=4, C=64,
             Kp=128, n_bits=8, stream=None)
    a.update(kw)

    def ptr(v):
        if v is None or isinstance(v, int):
            return None if v is None else C.c_void_p(v)
        return C.cast(v, C.c_void_p)
    order = ["x", "add_rows", "n_add", "add_div", "shift", "scale", "ln_eps", "n_out", "s", "s_rcp", "delta", "zp", "n_param",
             "xq", "sx", "zx", "R", "xm_out", "B", "n_tok", "C", "Kp", "n_bits", "stream"]
    pointers = {"x", "add_rows", "shift", "scale", "s", "s_rcp", "delta", "zp", "xq", "sx", "zx", "R", "xm_out", "stream"}
    return lib.vq_rowquant_static(*[ptr(a[k]) if k in pointers else a[k] for k in order])


def test_the_entry_point_is_exported_and_bound_with_the_headers_arity(lib):
    from viditq_amd import _lib
    assert hasattr(lib, "vq_rowquant_static")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bvq_rowquant_static\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert m, "vq_rowquant_static is not declared in include/viditq.h"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    res, args = _lib.SIGNATURES["vq_rowquant_static"]
    assert res is C.c_int and len(args) == len(params) == 24
    for decl, ct in zip(params, args):
        kind = C.c_void_p if "*" in decl else C.c_float if re.match(r"^(const\s+)?float\b", decl) else C.c_int
        assert ct is kind, decl


NULL_OUT = dict(xq=_arr(None, GOOD, GOOD))      # reaches the per-output checks and stops there: VQ_EINVAL

CODES = [
    # (what, overrides, code)
    ("add_rows together with LayerNorm", dict(add_rows=GOOD, n_add=4, shift=GOOD, scale=GOOD), EUNSUP),
    ("n_bits 1", dict(n_bits=1), EUNSUP),
    ("n_bits 9", dict(n_bits=9), EUNSUP),
    ("Kp > 4608", dict(C=4616, Kp=4736), EUNSUP),
    ("C % 8", dict(C=60), ESHAPE),
    ("Kp % 128", dict(Kp=100), ESHAPE),
    ("Kp < C", dict(C=256, Kp=128), ESHAPE),
    ("x off 16 bytes", dict(x=BAD), ESHAPE),
    ("add_rows off 16 bytes", dict(add_rows=BAD, n_add=4), ESHAPE),
    ("shift off 16 bytes", dict(shift=BAD, scale=GOOD), ESHAPE),
    ("xm_out off 16 bytes", dict(shift=GOOD, scale=GOOD, xm_out=BAD), ESHAPE),
    ("xq[1] off 16 bytes", dict(n_out=2, xq=_arr(GOOD, BAD, GOOD)), ESHAPE),
    ("s[0] off 16 bytes", dict(s=_arr(BAD), s_rcp=_arr(GOOD)), ESHAPE),
    ("s_rcp[0] off 16 bytes", dict(s=_arr(GOOD), s_rcp=_arr(BAD)), ESHAPE),
    ("null x", dict(x=None), EINVAL),
    ("null delta array", dict(delta=None), EINVAL),
    ("null R array", dict(R=None), EINVAL),
    ("scale without shift", dict(scale=GOOD), EINVAL),
    ("null zp[1]", dict(n_out=2, zp=_arr(GOOD, None, GOOD)), EINVAL),
    ("null xq[0]", NULL_OUT, EINVAL),
    ("B 0", dict(B=0), EINVAL),
    ("n_tok 0", dict(n_tok=0, n_param=0), EINVAL),
    ("C 0", dict(C=0), EINVAL),
    ("n_out 0", dict(n_out=0), EINVAL),
    ("n_out 4", dict(n_out=4), EINVAL),
    ("n_param 2 of 4 tokens", dict(n_param=2), EINVAL),
    ("add_rows too short", dict(add_rows=GOOD, n_add=1, add_div=2), EINVAL),
]


@pytest.mark.parametrize("what,kw,code", CODES, ids=[c[0] for c in CODES])
def test_each_refusal_has_its_code_and_comes_before_any_launch(lib, what, kw, code):
    assert _call(lib, **kw) == code, what


def test_n_param_may_be_one_or_n_tok(lib):
    assert _call(lib, n_param=1, **NULL_OUT) == EINVAL          # (the null output: past every shape check)
    assert _call(lib, n_param=4, **NULL_OUT) == EINVAL
    assert _call(lib, n_param=4, C=60, **NULL_OUT) == ESHAPE    # ... which a bad shape does not reach


MIRROR = [
    # C, Kp, n_bits, n_out, add_rows, LN
    (1152, 1152, 8, 3, False, True),
    (1152, 1152, 8, 3, True, False),
    (4608, 4608, 8, 1, False, False),
    (64, 128, 4, 2, False, False),
    (200, 256, 6, 1, True, False),
    (200, 384, 2, 1, False, True),
    (4600, 4608, 8, 3, False, True),
    (4616, 4736, 8, 1, False, False),      # Kp > 4608
    (6144, 6144, 8, 1, False, False),
    (1152, 1152, 9, 1, False, False),      # width
    (1152, 1152, 1, 1, False, False),
    (1152, 1152, 8, 1, True, True),        # both arms
    (60, 128, 8, 1, False, False),         # C % 8
    (64, 100, 8, 1, False, False),         # Kp % 128
    (256, 128, 8, 1, False, False),        # Kp < C
    (1152, 1152, 8, 4, False, False),      # n_out
    (1152, 1152, 8, 0, False, False),
]


@pytest.mark.parametrize("Cc,Kp,n_bits,n_out,add,ln", MIRROR)
def test_the_hosts_mirror_agrees_with_the_entry_point(lib, Cc, Kp, n_bits, n_out, add, ln):
    """ops.rowquant_static_ok says yes exactly where the entry point finds nothing to refuse in the shape (it then
    stops at the null output pointer this call carries, VQ_EINVAL's last cause; a bad n_out earns VQ_EINVAL earlier and
    is told apart by a second call that differs in n_out alone)."""
    from viditq_amd import ops
    kw = dict(C=Cc, Kp=Kp, n_bits=n_bits, n_out=n_out, **NULL_OUT)
    if add:
        kw.update(add_rows=GOOD, n_add=4)
    if ln:
        kw.update(shift=GOOD, scale=GOOD)
    code = _call(lib, **kw)
    accepted = code == EINVAL and 1 <= n_out <= 3
    assert code in (EINVAL, ESHAPE, EUNSUP)
    assert ops.rowquant_static_ok(Cc, Kp, n_bits, n_out, add_rows=add, ln=ln) == accepted, code


def test_rowquant_static_refuses_cpu_tensors():
    import torch
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    one = torch.ones(1)
    with pytest.raises(ops.VQError):
        ops.rowquant_static(torch.zeros(1, 4, 64, dtype=torch.float16), [one], [one])

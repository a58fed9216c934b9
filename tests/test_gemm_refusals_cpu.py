"""Refusals of the six int8 GEMM entry points, without a GPU: every clause of their argument checks violated alone, and
pairs of violations that fix which clause wins.  Pointers are non-null dummies that the checks must not dereference; every
case is refused before any HIP call, so nothing here reaches a device."""
import ctypes as C

import pytest

EINVAL, ESHAPE, EUNSUP = -1, -2, -4
P = 16                                        # dummy pointer: non-null, 16-byte aligned
_PTRS = ["xq", "sx", "zx", "R", "wq", "sw", "zw", "cs", "bias"]

# parameter names in the order of include/viditq.h
PARAMS = {
    "vq_gemm_i8": _PTRS + ["out", "ldo", "resid", "gate", "rows_per_gate", "M", "N", "K", "Kp", "w_bits", "epilogue",
                           "variant", "stream"],
    "vq_gemm_i8_batched": _PTRS + ["out", "nbatch", "M", "N", "K", "Kp", "w_bits", "stream"],
    "vq_gemm_i8_grouped": ["ngroups"] + _PTRS + ["out", "ldo", "M", "N", "K", "Kp", "w_bits", "stream"],
    "vq_gemm_i8_cross_attn": _PTRS + ["k", "v", "o", "M", "N", "K", "Kp", "w_bits", "n_seq", "Lq", "Lk", "H", "D",
                                      "kv_seq_stride", "kv_tok_stride", "o_seq_stride", "o_tok_stride", "kv_off", "scale",
                                      "stream"],
    "vq_gemm_i8_rowquant_static": _PTRS + ["s", "s_rcp", "delta", "zp", "xq_out", "sx_out", "zx_out", "R_out", "M", "N", "K",
                                           "Kp", "Kp_out", "w_bits", "n_bits", "variant", "stream"],
    "vq_gemm_i8_stamped": _PTRS + ["out", "ldo", "M", "N", "K", "Kp", "stamps", "n_stamps", "stream"],
}
# one interior 256 x 288 tile, K = Kp = 128, 8-bit weights: every case below differs from it in what its row names
_SHAPE = dict(M=256, N=288, K=128, Kp=128)
BASE = {
    "vq_gemm_i8": dict(_SHAPE, ldo=288, rows_per_gate=1, w_bits=8, epilogue=0, variant=-1),
    "vq_gemm_i8_batched": dict(_SHAPE, nbatch=2, w_bits=8),
    "vq_gemm_i8_grouped": dict(_SHAPE, ngroups=3, ldo=864, w_bits=8),
    "vq_gemm_i8_cross_attn": dict(_SHAPE, w_bits=8, n_seq=1, Lq=256, Lk=120, H=4, D=72, kv_seq_stride=120 * 288,
                                  kv_tok_stride=288, o_seq_stride=256 * 288, o_tok_stride=288, scale=1.0),
    "vq_gemm_i8_rowquant_static": dict(_SHAPE, Kp_out=384, w_bits=8, n_bits=8, variant=-1),
    "vq_gemm_i8_stamped": dict(_SHAPE, ldo=288, n_stamps=80),
}
NULL = None
BIG = 1 << 25                                 # BIG * 128 = 2^32: one byte past what a 32-bit operand offset reaches
GATE_RESID, RESID = 2, 3

# (entry point, what is violated, {parameter: value}, expected code)
ALONE = [
    ("vq_gemm_i8", "Kp % 128", dict(K=64, Kp=64), ESHAPE),
    ("vq_gemm_i8", "Kp < K", dict(K=200), ESHAPE),
    ("vq_gemm_i8", "K = 16385", dict(K=16385, Kp=16512), ESHAPE),
    ("vq_gemm_i8", "M * Kp = 2^32", dict(M=BIG), ESHAPE),
    ("vq_gemm_i8", "N * Kp = 2^32", dict(N=BIG, ldo=BIG), ESHAPE),
    ("vq_gemm_i8", "N % 4", dict(N=290, ldo=292), ESHAPE),
    ("vq_gemm_i8", "ldo % 4", dict(ldo=290), ESHAPE),
    ("vq_gemm_i8", "ldo < N", dict(ldo=284), ESHAPE),
    ("vq_gemm_i8", "w_bits = 1", dict(w_bits=1), EUNSUP),
    ("vq_gemm_i8", "w_bits = 9", dict(w_bits=9), EUNSUP),
    ("vq_gemm_i8", "epilogue = -1", dict(epilogue=-1), EUNSUP),
    ("vq_gemm_i8", "epilogue = 4", dict(epilogue=4), EUNSUP),
    ("vq_gemm_i8", "unknown variant", dict(variant=7), EUNSUP),
    ("vq_gemm_i8", "unknown variant, nibble weights", dict(variant=12, w_bits=4), EUNSUP),
    ("vq_gemm_i8", "variant 19, M % 256", dict(variant=19, M=300), ESHAPE),
    ("vq_gemm_i8", "variant 19, N % 288", dict(variant=19, N=292, ldo=296), ESHAPE),
    ("vq_gemm_i8", "variant 19, a half-tile shape", dict(variant=19, M=128), ESHAPE),
    ("vq_gemm_i8", "variant 19, ldo % 8", dict(variant=19, ldo=292), ESHAPE),
    ("vq_gemm_i8", "variant 19, rows_per_gate % 256", dict(variant=19, epilogue=GATE_RESID, rows_per_gate=128), ESHAPE),
    ("vq_gemm_i8", "variant 19, nibble weights, M % 256", dict(variant=19, w_bits=4, M=384), ESHAPE),
    ("vq_gemm_i8", "rows_per_gate = 0", dict(epilogue=GATE_RESID, rows_per_gate=0), EINVAL),
    ("vq_gemm_i8", "gate epilogue without resid", dict(epilogue=GATE_RESID, resid=NULL), EINVAL),
    ("vq_gemm_i8", "gate epilogue without gate", dict(epilogue=GATE_RESID, gate=NULL), EINVAL),
    ("vq_gemm_i8", "residual epilogue without resid", dict(epilogue=RESID, resid=NULL), EINVAL),
    ("vq_gemm_i8", "M = 0", dict(M=0), EINVAL),

    ("vq_gemm_i8_batched", "Kp % 128", dict(K=64, Kp=64), ESHAPE),
    ("vq_gemm_i8_batched", "Kp < K", dict(K=200), ESHAPE),
    ("vq_gemm_i8_batched", "K = 16385", dict(K=16385, Kp=16512), ESHAPE),
    ("vq_gemm_i8_batched", "M * Kp = 2^32", dict(M=BIG), ESHAPE),
    ("vq_gemm_i8_batched", "N * Kp = 2^32", dict(N=BIG), ESHAPE),
    ("vq_gemm_i8_batched", "N % 4", dict(N=290), ESHAPE),
    ("vq_gemm_i8_batched", "w_bits = 4", dict(w_bits=4), EUNSUP),
    ("vq_gemm_i8_batched", "w_bits = 9", dict(w_bits=9), EUNSUP),
    ("vq_gemm_i8_batched", "nbatch = 0", dict(nbatch=0), EINVAL),

    ("vq_gemm_i8_grouped", "Kp % 128", dict(K=64, Kp=64), ESHAPE),
    ("vq_gemm_i8_grouped", "Kp < K", dict(K=200), ESHAPE),
    ("vq_gemm_i8_grouped", "K = 16385", dict(K=16385, Kp=16512), ESHAPE),
    ("vq_gemm_i8_grouped", "M * Kp = 2^32", dict(M=BIG), ESHAPE),
    ("vq_gemm_i8_grouped", "N * Kp = 2^32", dict(N=BIG, ngroups=1, ldo=BIG), ESHAPE),
    ("vq_gemm_i8_grouped", "N % 4", dict(N=290, ldo=872), ESHAPE),
    ("vq_gemm_i8_grouped", "ldo % 4", dict(ldo=866), ESHAPE),
    ("vq_gemm_i8_grouped", "ldo < ngroups * N", dict(ldo=860), ESHAPE),
    ("vq_gemm_i8_grouped", "w_bits = 1", dict(w_bits=1), EUNSUP),
    ("vq_gemm_i8_grouped", "w_bits = 9", dict(w_bits=9), EUNSUP),
    ("vq_gemm_i8_grouped", "ngroups = 4", dict(ngroups=4, ldo=1152), EINVAL),
    ("vq_gemm_i8_grouped", "a null pointer inside a group", dict(sw=[P, NULL, P]), EINVAL),

    ("vq_gemm_i8_cross_attn", "Kp % 128", dict(K=64, Kp=64), ESHAPE),
    ("vq_gemm_i8_cross_attn", "Kp < K", dict(K=200), ESHAPE),
    ("vq_gemm_i8_cross_attn", "K = 16385", dict(K=16385, Kp=16512), ESHAPE),
    ("vq_gemm_i8_cross_attn", "M * Kp = 2^32", dict(M=BIG, Lq=BIG), ESHAPE),
    ("vq_gemm_i8_cross_attn", "N * Kp = 2^32", dict(N=BIG), ESHAPE),
    ("vq_gemm_i8_cross_attn", "w_bits = 1", dict(w_bits=1), EUNSUP),
    ("vq_gemm_i8_cross_attn", "w_bits = 9", dict(w_bits=9), EUNSUP),
    ("vq_gemm_i8_cross_attn", "D = 64", dict(D=64), EUNSUP),
    ("vq_gemm_i8_cross_attn", "M % 256", dict(M=384, Lq=384), ESHAPE),
    ("vq_gemm_i8_cross_attn", "N % 288", dict(N=144, H=2), ESHAPE),
    ("vq_gemm_i8_cross_attn", "N != H * D", dict(H=3), ESHAPE),
    ("vq_gemm_i8_cross_attn", "Lq % 256", dict(M=512, n_seq=4, Lq=128), ESHAPE),
    ("vq_gemm_i8_cross_attn", "Lk = 129", dict(Lk=129), ESHAPE),
    ("vq_gemm_i8_cross_attn", "o_tok_stride < N", dict(o_tok_stride=280), ESHAPE),
    ("vq_gemm_i8_cross_attn", "a pointer off 16 bytes", dict(k=P + 8), ESHAPE),

    ("vq_gemm_i8_rowquant_static", "Kp % 128", dict(K=64, Kp=64), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "Kp < K", dict(K=200), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "K = 16385", dict(K=16385, Kp=16512), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "M * Kp = 2^32", dict(M=BIG), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "N * Kp = 2^32", dict(N=BIG, Kp_out=BIG), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "N % 8", dict(N=292), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "Kp_out % 128", dict(Kp_out=320), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "Kp_out < N", dict(Kp_out=256), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "a pointer off 16 bytes", dict(xq_out=P + 8), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "w_bits = 4", dict(w_bits=4), EUNSUP),
    ("vq_gemm_i8_rowquant_static", "w_bits = 9", dict(w_bits=9), EUNSUP),
    ("vq_gemm_i8_rowquant_static", "n_bits = 1", dict(n_bits=1), EUNSUP),
    ("vq_gemm_i8_rowquant_static", "n_bits = 9", dict(n_bits=9), EUNSUP),
    ("vq_gemm_i8_rowquant_static", "s without s_rcp", dict(s_rcp=NULL), EUNSUP),
    ("vq_gemm_i8_rowquant_static", "unknown variant", dict(variant=7), EUNSUP),
    ("vq_gemm_i8_rowquant_static", "variant 19, M % 256", dict(variant=19, M=304), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "variant 19, N % 288", dict(variant=19, N=296), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "variant 19, a half-tile shape", dict(variant=19, M=128), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "Kp_out = 0", dict(Kp_out=0), EINVAL),

    ("vq_gemm_i8_stamped", "Kp % 128", dict(K=64, Kp=64), ESHAPE),
    ("vq_gemm_i8_stamped", "Kp < K", dict(K=200), ESHAPE),
    ("vq_gemm_i8_stamped", "K = 16385", dict(K=16385, Kp=16512), ESHAPE),
    ("vq_gemm_i8_stamped", "M * Kp = 2^32", dict(M=BIG, n_stamps=1 << 40), ESHAPE),
    ("vq_gemm_i8_stamped", "N * Kp = 2^32", dict(N=BIG, ldo=BIG, n_stamps=1 << 40), ESHAPE),
    ("vq_gemm_i8_stamped", "N % 4", dict(N=290, ldo=292, n_stamps=160), ESHAPE),
    ("vq_gemm_i8_stamped", "ldo % 4", dict(ldo=290), ESHAPE),
    ("vq_gemm_i8_stamped", "ldo < N", dict(ldo=284), ESHAPE),
    ("vq_gemm_i8_stamped", "one stamp short", dict(n_stamps=79), ESHAPE),
    ("vq_gemm_i8_stamped", "no stamp buffer", dict(stamps=NULL), EINVAL),
]

# two clauses violated at once: the code of the one that is checked first
PAIRS = [
    ("vq_gemm_i8", "null pointer + Kp % 128", dict(sx=NULL, K=64, Kp=64), EINVAL),
    ("vq_gemm_i8", "M = 0 + Kp % 128", dict(M=0, K=64, Kp=64), EINVAL),
    ("vq_gemm_i8", "Kp % 128 + w_bits = 9", dict(K=64, Kp=64, w_bits=9), ESHAPE),
    ("vq_gemm_i8", "ldo < N + unknown epilogue", dict(ldo=284, epilogue=7), ESHAPE),
    ("vq_gemm_i8", "w_bits = 9 + K = 16385", dict(w_bits=9, K=16385, Kp=16512), EUNSUP),
    ("vq_gemm_i8", "unknown epilogue + M * Kp = 2^32", dict(epilogue=7, M=BIG), EUNSUP),
    ("vq_gemm_i8", "w_bits = 9 + missing resid", dict(w_bits=9, epilogue=RESID, resid=NULL), EUNSUP),
    ("vq_gemm_i8", "missing resid + K = 16385", dict(epilogue=RESID, resid=NULL, K=16385, Kp=16512), EINVAL),
    ("vq_gemm_i8", "rows_per_gate = 0 + N * Kp = 2^32", dict(epilogue=GATE_RESID, rows_per_gate=0, N=BIG, ldo=BIG), EINVAL),
    ("vq_gemm_i8", "K = 16385 + unknown variant", dict(K=16385, Kp=16512, variant=7), ESHAPE),
    ("vq_gemm_i8", "M * Kp = 2^32 + variant 19 on M % 256", dict(M=BIG + 4, variant=19), ESHAPE),
    ("vq_gemm_i8_batched", "null pointer + Kp % 128", dict(wq=NULL, K=64, Kp=64), EINVAL),
    ("vq_gemm_i8_batched", "N % 4 + w_bits = 4", dict(N=290, w_bits=4), ESHAPE),
    ("vq_gemm_i8_batched", "w_bits = 4 + K = 16385", dict(w_bits=4, K=16385, Kp=16512), EUNSUP),
    ("vq_gemm_i8_batched", "w_bits = 9 + M * Kp = 2^32", dict(w_bits=9, M=BIG), EUNSUP),
    ("vq_gemm_i8_grouped", "ngroups = 0 + Kp < K", dict(ngroups=0, K=200), EINVAL),
    ("vq_gemm_i8_grouped", "ldo < ngroups * N + w_bits = 9", dict(ldo=860, w_bits=9), ESHAPE),
    ("vq_gemm_i8_grouped", "w_bits = 9 + K = 16385", dict(w_bits=9, K=16385, Kp=16512), EUNSUP),
    ("vq_gemm_i8_grouped", "K = 16385 + a null pointer inside a group", dict(K=16385, Kp=16512, cs=[P, P, NULL]), ESHAPE),
    ("vq_gemm_i8_grouped", "w_bits = 1 + a null pointer inside a group", dict(w_bits=1, xq=[NULL, P, P]), EUNSUP),
    ("vq_gemm_i8_cross_attn", "null pointer + Kp % 128", dict(v=NULL, K=64, Kp=64), EINVAL),
    ("vq_gemm_i8_cross_attn", "Lk = 0 + K = 16385", dict(Lk=0, K=16385, Kp=16512), EINVAL),
    ("vq_gemm_i8_cross_attn", "K = 16385 + w_bits = 9", dict(K=16385, Kp=16512, w_bits=9), ESHAPE),
    ("vq_gemm_i8_cross_attn", "N * Kp = 2^32 + D = 64", dict(N=BIG, D=64), ESHAPE),
    ("vq_gemm_i8_cross_attn", "w_bits = 9 + M % 256", dict(w_bits=9, M=384, Lq=384), EUNSUP),
    ("vq_gemm_i8_cross_attn", "D = 64 + Lk = 129", dict(D=64, Lk=129), EUNSUP),
    ("vq_gemm_i8_rowquant_static", "null pointer + Kp % 128", dict(delta=NULL, K=64, Kp=64), EINVAL),
    ("vq_gemm_i8_rowquant_static", "Kp < K + w_bits = 4", dict(K=200, w_bits=4), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "N % 8 + n_bits = 9", dict(N=292, n_bits=9), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "variant 19 on M % 256 + w_bits = 4", dict(variant=19, M=304, w_bits=4), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "variant 19 on N % 288 + unknown variant's neighbour n_bits = 1",
     dict(variant=19, N=296, n_bits=1), ESHAPE),
    ("vq_gemm_i8_rowquant_static", "w_bits = 9 + unknown variant", dict(w_bits=9, variant=7), EUNSUP),
    ("vq_gemm_i8_rowquant_static", "M * Kp = 2^32 + s without s_rcp", dict(M=BIG, s_rcp=NULL), ESHAPE),
    ("vq_gemm_i8_stamped", "null pointer + Kp % 128", dict(out=NULL, K=64, Kp=64), EINVAL),
    ("vq_gemm_i8_stamped", "K = 0 + ldo < N", dict(K=0, ldo=284), EINVAL),
    ("vq_gemm_i8_stamped", "K = 16385 + one stamp short", dict(K=16385, Kp=16512, n_stamps=79), ESHAPE),
]


@pytest.fixture(scope="module")
def lib():
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    return _lib.load()


def _call(lib, name, over):
    from viditq_amd import _lib
    argtypes = _lib.SIGNATURES[name][1]
    names = PARAMS[name]
    assert len(names) == len(argtypes), name
    assert set(over) <= set(names), (name, sorted(set(over) - set(names)))
    vals = dict(BASE[name], **over)
    grouped = name == "vq_gemm_i8_grouped"
    keep = []                                  # the groups' pointer arrays stay alive over the call
    args = []
    for pn, ct in zip(names, argtypes):
        if pn == "stream":
            args.append(None)
        elif ct is C.c_void_p:
            v = vals.get(pn, P)
            if grouped and pn in _PTRS:        # one pointer per group
                v = v if isinstance(v, list) else [v] * 3
                arr = (C.c_void_p * 3)(*[C.c_void_p(x) if x is not None else None for x in v])
                keep.append(arr)
                v = C.cast(arr, C.c_void_p)
            args.append(v)
        else:
            args.append(vals[pn])
    return getattr(lib, name)(*args)


def _id(case):
    return "%s-%s" % (case[0][3:], case[1].replace(" ", "_"))


@pytest.mark.parametrize("case", ALONE, ids=_id)
def test_gemm_entry_point_refuses_each_clause_alone(lib, case):
    name, _, over, code = case
    assert _call(lib, name, over) == code


@pytest.mark.parametrize("case", PAIRS, ids=_id)
def test_gemm_entry_point_refusal_precedence(lib, case):
    name, _, over, code = case
    assert _call(lib, name, over) == code


def test_the_table_covers_all_six_entry_points():
    assert {c[0] for c in ALONE} == set(PARAMS) == {c[0] for c in PAIRS}

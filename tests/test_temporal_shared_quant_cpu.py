"""CPU-side checks of vq_attn_temporal_rowquant_shared (temporal attention + attn_temp.proj's dynamic per-token quantizer
for a joint cond | uncond forward, 2..8 bits): declared, exported and bound alike; its argument rules enforced, in their
order, before any device call; ops.attn_temporal_shared_ok agreeing with them; the model's switch off by default; and the
one-hot inputs of the GPU edge-row test staying inside their cap in both samples."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vq_attn_temporal_rowquant_shared"
EINVAL, ESHAPE, EUNSUP = -1, -2, -4

# (T, S, H, D) of the GPU tests: trimmed kernel with the D = 72 tail | generic kernel, rows >= T masked, odd S | generic
# kernel, 8 waves | trimmed kernel, T < 16, smallest D
SHAPES = [(16, 8, 16, 72), (5, 9, 2, 32), (16, 8, 8, 64), (3, 5, 16, 16)]


def edge_seed(T, D, b):
    """Seed of sample b's one-hot keys in the GPU edge-row test (sample 0: the seed of the existing families)."""
    return 100 * T + D + 7 * b


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L, L.load()


def test_shared_entry_point_is_declared_exported_and_bound_alike():
    L, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m, "not declared in include/viditq.h"
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    res, kinds = L.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(kinds) == len(params) == 21

    def kind(decl):
        if "*" in decl:
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}[decl.split()[0]]
    assert [kind(p) for p in params] == list(kinds)
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "q", "k", "v", "s", "s_rcp", "xq", "sx", "zx", "R", "status", "o", "B", "T", "S", "H", "D", "ld_in", "Kp", "n_bits",
        "scale", "stream"]
    from viditq_amd import ops
    from viditq_amd.qdiff.models.quant_block import QuantAttention
    assert callable(ops.attn_temporal_rowquant_shared) and callable(ops.attn_temporal_shared_ok)
    assert callable(QuantAttention.temporal_quantized_shared)
    # the existing entry point says where shared grids are
    doc = re.findall(r"/\*(.*?)\*/\s*int\s+vq_attn_temporal_rowquant\s*\(", open(os.path.join(ROOT, "include", "viditq.h")).read(), re.S)
    assert doc and NAME in doc[-1].split("/*")[-1]


ONE = 16            # non-null, 16-byte aligned dummy address: the checks must reject before any dereference


def _call(lib, q=ONE, k=ONE, v=ONE, s=None, s_rcp=None, xq=ONE, sx=ONE, zx=ONE, R=ONE, status=None, o=None, B=2, T=16, S=4,
          H=4, D=16, ld_in=None, Kp=None, n_bits=8):
    C = H * D
    ld_in = 3 * C if ld_in is None else ld_in
    Kp = (C + 127) // 128 * 128 if Kp is None else Kp
    p = lambda a: None if a is None else ctypes.c_void_p(a)  # noqa: E731
    return getattr(lib, NAME)(p(q), p(k), p(v), p(s), p(s_rcp), p(xq), p(sx), p(zx), p(R), p(status), p(o), B, T, S, H, D,
                              ld_in, Kp, n_bits, 1.0, None)


@pytest.mark.parametrize("kw,want", [
    # VQ_EINVAL: a null required pointer; s without s_rcp or the reverse; a non-positive extent
    (dict(q=None), EINVAL), (dict(k=None), EINVAL), (dict(v=None), EINVAL), (dict(xq=None), EINVAL),
    (dict(sx=None), EINVAL), (dict(zx=None), EINVAL), (dict(R=None), EINVAL),
    (dict(s=ONE), EINVAL), (dict(s_rcp=ONE), EINVAL),
    (dict(B=0), EINVAL), (dict(T=0), EINVAL), (dict(S=0), EINVAL), (dict(H=0), EINVAL), (dict(D=0, Kp=128), EINVAL),
    (dict(Kp=0), EINVAL), (dict(B=-1), EINVAL), (dict(Kp=-128), EINVAL),
    # VQ_ESHAPE: what the T <= 16 kernels refuse ...
    (dict(T=17), ESHAPE), (dict(H=17, Kp=384), ESHAPE), (dict(ld_in=196), ESHAPE),
    (dict(H=3, D=72, Kp=256), ESHAPE),                               # H * D % 16
    (dict(Kp=100), ESHAPE), (dict(H=16, D=16, Kp=128), ESHAPE),      # Kp % 128, Kp < H * D
    (dict(H=4, D=100, Kp=512), ESHAPE),                              # the V staging limit: 16 * (H * D / 8) > 192 * H
    (dict(q=20), ESHAPE), (dict(k=24), ESHAPE), (dict(v=18), ESHAPE), (dict(xq=32 + 8), ESHAPE),
    (dict(s=20, s_rcp=ONE), ESHAPE), (dict(s=ONE, s_rcp=20), ESHAPE), (dict(o=24), ESHAPE),
    # ... a head dim without a kernel, and more samples than a workgroup holds
    (dict(D=48, Kp=256), ESHAPE), (dict(B=3), ESHAPE),
    # VQ_EUNSUP: the code width
    (dict(n_bits=1), EUNSUP), (dict(n_bits=9), EUNSUP), (dict(n_bits=0), EUNSUP), (dict(B=1, n_bits=16), EUNSUP),
    # the order: null before shape before width
    (dict(q=None, T=17), EINVAL), (dict(R=None, B=3, n_bits=9), EINVAL), (dict(s=ONE, D=48, Kp=256), EINVAL),
    (dict(B=0, Kp=100), EINVAL), (dict(T=17, n_bits=9), ESHAPE), (dict(B=3, n_bits=1), ESHAPE), (dict(D=48, Kp=256, n_bits=9), ESHAPE),
    (dict(o=24, n_bits=9), ESHAPE),
])
def test_shared_argument_rules_without_gpu(kw, want):
    """Every refusal returns its code before any HIP call or dereference (the pointers are dummies, no GPU is needed)."""
    _, lib = _lib()
    assert _call(lib, **kw) == want


def test_shared_ok_agrees_with_the_entry_point():
    """ops.attn_temporal_shared_ok is true exactly when the entry point does not refuse, over a grid of its six arguments
    (S = 1, ld_in = 3 H D, aligned dummy pointers, s = s_rcp = o = NULL: the answer depends on the six only).
    An accepted call would launch on dummy pointers, so acceptance is read without one: the width check is the entry
    point's LAST, and no earlier check reads n_bits, so 'returns VQ_EUNSUP at width 9' is 'nothing but the width can
    refuse these arguments'.  The call is accepted exactly when that holds and 2 <= n_bits <= 8."""
    _, lib = _lib()
    from viditq_amd import ops
    n_ok, kernels, codes = 0, set(), {EINVAL: 0, ESHAPE: 0, EUNSUP: 0}
    for B in (0, 1, 2, 3):
        for T in (0, 1, 16, 17):
            for H in (0, 2, 3, 8, 16, 17):
                for D in (0, 16, 48, 64, 72, 100):
                    C = H * D
                    for Kp in sorted({0, 100, 128, C, (C + 127) // 128 * 128, 2048, 2176}):
                        at9 = _call(lib, B=B, T=T, S=1, H=H, D=D, Kp=Kp, n_bits=9)
                        assert at9 in codes, (B, T, H, D, Kp, at9)
                        for n_bits in (1, 2, 6, 8, 9):
                            accepted = at9 == EUNSUP and 2 <= n_bits <= 8
                            ok = ops.attn_temporal_shared_ok(B, T, H, D, Kp, n_bits)
                            assert ok == accepted, (B, T, H, D, Kp, n_bits, at9)
                            if not accepted:
                                rc = at9 if at9 != EUNSUP else _call(lib, B=B, T=T, S=1, H=H, D=D, Kp=Kp, n_bits=n_bits)
                                codes[rc] += 1
                            else:
                                n_ok += 1
                                kernels.add("trimmed" if H == 16 and Kp <= 2048 else "generic")
    assert n_ok > 100 and kernels == {"trimmed", "generic"} and all(codes.values()), (n_ok, kernels, codes)
    # every refusal the predicate can see, once by name
    good = dict(B=2, T=16, H=16, D=72, Kp=1152, n_bits=6)
    assert ops.attn_temporal_shared_ok(**good) and ops.attn_temporal_shared_ok(**dict(good, B=1, H=2, D=32, Kp=128, n_bits=2))
    for bad in (dict(n_bits=1), dict(n_bits=9), dict(B=3), dict(T=17), dict(H=17, Kp=1280), dict(D=48, Kp=768),
                dict(H=3, Kp=256), dict(Kp=1100), dict(Kp=1024), dict(H=4, D=100, Kp=512), dict(B=0), dict(T=0), dict(H=0),
                dict(D=0), dict(Kp=0)):
        assert not ops.attn_temporal_shared_ok(**dict(good, **bad)), bad


def test_joint_switch_is_off_by_default():
    _lib()
    from viditq_amd.t2v import stdit
    if "VQ_ATTN_QUANT_JOINT" not in os.environ:
        assert stdit._ATTN_QUANT_JOINT is False
    assert isinstance(stdit._ATTN_QUANT_JOINT, bool)


@pytest.mark.parametrize("T,S,H,D", SHAPES)
def test_edge_row_inputs_stay_inside_their_cap_in_both_samples(T, S, H, D):
    """The one-hot q / k of the GPU edge-row test, one seed per sample: in each sample at least 0.9 of the tokens have every
    head's lead >= R1_GAP, and at least 0.8 of the tokens have it in BOTH samples (only those are compared)."""
    import attn_regimes as ar
    import quant_rows as qr
    scale = D ** -0.5
    sel = []
    for b in range(2):
        q, k, hot = qr.one_hot_qk(S, T, H, D, scale, seed=edge_seed(T, D, b))
        gp = ar.gaps(q, k, hot[:, :, None].expand(S, T, H).contiguous(), scale, [T] * S)
        sel.append((gp >= ar.R1_GAP).all(-1))
        assert float(sel[-1].double().mean()) >= 0.9, b
    assert float((sel[0] & sel[1]).double().mean()) >= 0.8

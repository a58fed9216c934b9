"""CPU-side checks of vq_attn_fwd_rowquant_static (spatial / cross attention + proj's static tensor-wise quantizer):
exported, bound and declared; its argument rules enforced before any device call; the routes without a static-grid form
refused; ops.attn_fwd_static_ok agreeing with the entry point; no new VQ_ATTN_K_* id; the blocks' route predicate; and the
shapes and one-hot inputs of the GPU tests (SHAPES) reaching the kernel they name and staying inside their cap."""
import ctypes
import functools
import os
import re
import types

import pytest
import torch

import attn_regimes as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vq_attn_fwd_rowquant_static"
EINVAL, ESHAPE, EUNSUP = -1, -2, -4

# (kernel, D, n, Lq, lens, H, kv_off); kv_off: False | True (Lk = the longest sequence) | "unbound" (Lk = 0: no bound known).
# Shape i uses seed 500 + i.  H * D >= 64: quant_rows.static_rows places two of its out-of-grid values on one column at
# C = 32.
SHAPES = [
    ("VQ_ATTN_K_FWD", 16, 2, 300, [150, 77], 4, "unbound"),
    ("VQ_ATTN_K_FWD", 72, 2, 64, [200, 200], 4, False),
    ("VQ_ATTN_K_FWD", 32, 2, 80, [333, 333], 2, False),
    ("VQ_ATTN_K_FWD32D", 72, 2, 300, [333, 333], 2, False),
    ("VQ_ATTN_K_FWD32D", 32, 2, 513, [191, 191], 2, False),
    ("VQ_ATTN_K_FWD32D", 64, 1, 192, [700], 2, False),
    ("VQ_ATTN_K_FWD32D", 72, 1, 256, [256], 16, False),          # the real row width: Kp = C = 1152
    ("VQ_ATTN_K_FWD64D", 72, 1, 2048, [2100], 2, False),
    ("VQ_ATTN_K_FWD64D", 64, 1, 2100, [2077], 1, False),
    ("VQ_ATTN_K_CROSS32_2", 72, 2, 300, [120, 37], 2, True),
    ("VQ_ATTN_K_CROSS32_2", 32, 2, 300, [128, 128], 2, False),
    ("VQ_ATTN_K_CROSS32_3", 72, 2, 256, [192, 17], 2, True),
    ("VQ_ATTN_K_CROSS32_4", 64, 2, 260, [256, 200], 2, True),
    ("VQ_ATTN_K_CROSS32_5", 72, 2, 290, [300, 1], 2, True),
]
SHAPE_IDS = ["%d-%s-D%d-%dx%dx%s-H%d" % (i, s[0].replace("VQ_ATTN_K_", ""), s[1], s[2], s[3], "+".join(map(str, s[4])), s[5])
             for i, s in enumerate(SHAPES)]


def shape_case(i):
    """SHAPES[i] as an attn_regimes case (for fwd_layout) and its seed."""
    kern, D, n, Lq, lens, H, kv_off = SHAPES[i]
    sh = dict(n=n, Lq=Lq, lens=lens, H=H, kv_off=bool(kv_off))
    if kv_off == "unbound":
        sh["bound"] = 0
    return dict(id=SHAPE_IDS[i], kernel=kern, D=D, shape=sh, scale=D ** -0.5, seed=500 + i)


@functools.lru_cache(maxsize=None)
def one_hot(i):
    """attn_regimes.r1 of SHAPES[i]: q, k, v, hot (computed once, shared; callers do not modify them)."""
    kern, D, n, Lq, lens, H, kv_off = SHAPES[i]
    return ar.r1(n, Lq, lens, H, D, D ** -0.5, 500 + i)


@functools.lru_cache(maxsize=None)
def one_hot_selected(i):
    """[n, Lq] bool: query rows of SHAPES[i] whose every head leads by >= R1_GAP."""
    kern, D, n, Lq, lens, H, kv_off = SHAPES[i]
    q, k, v, hot = one_hot(i)
    return (ar.gaps(q, k, hot, D ** -0.5, lens) >= ar.R1_GAP).all(-1)


def static_v(i, n_bits):
    """V [n, max(lens), H, D] of quant_rows.static_rows for SHAPES[i], with its grid."""
    import quant_rows as qr
    kern, D, n, Lq, lens, H, kv_off = SHAPES[i]
    rows, delta, zp = qr.static_rows(1, n * max(lens), H * D, n_bits, per_token=False)
    return rows[0].reshape(n, max(lens), H, D), delta, zp


def hot_rows(v, hot):
    """[n, Lq, H, D]: the hot key's V row of every (query, head)."""
    return torch.stack([v[s][hot[s], torch.arange(v.shape[2])[None, :]] for s in range(v.shape[0])])


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L, L.load()


def test_static_fwd_attention_entry_point_is_exported_bound_and_declared():
    L, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m, "not declared in include/viditq.h"
    assert hasattr(lib, NAME)
    assert NAME in L.SIGNATURES
    assert len(L.SIGNATURES[NAME][1]) == len(m.group(1).split(",")) == 28
    from viditq_amd import ops
    assert callable(ops.attn_fwd_rowquant_static) and callable(ops.attn_fwd_static_ok)


def test_no_attention_kernel_id_was_added():
    assert sorted(ar.kernel_ids()) == sorted(ar.FWD_KERNELS)
    assert sorted(ar.kernel_ids().values()) == [0, 1, 2, 3, 5, 6, 7, 8, 9, 10]


ONE = 1 << 20       # non-null, 16-byte aligned dummy address: the checks must reject before any dereference


def _call(lib, q=ONE, k=ONE, v=ONE, s=None, s_rcp=None, delta=ONE, zp=ONE, xq=ONE, sx=ONE, zx=ONE, R=ONE, o=None, n_seq=2,
          Lq=300, Lk=333, H=2, D=72, q_seq=None, q_tok=None, kv_seq=None, kv_tok=None, o_seq=None, o_tok=None, kv_off=None,
          Kp=None, n_bits=8, fn=NAME):
    C = H * D
    q_tok = C if q_tok is None else q_tok
    kv_tok = 2 * C if kv_tok is None else kv_tok
    o_tok = C if o_tok is None else o_tok
    q_seq = Lq * q_tok if q_seq is None else q_seq
    kv_seq = (0 if kv_off else Lk * kv_tok) if kv_seq is None else kv_seq
    o_seq = Lq * o_tok if o_seq is None else o_seq
    Kp = (C + 127) // 128 * 128 if Kp is None else Kp
    p = lambda a: None if a is None else ctypes.c_void_p(a)  # noqa: E731
    if fn == "vq_attn_fwd_route":
        return lib.vq_attn_fwd_route(p(q), p(k), p(v), p(ONE), n_seq, Lq, Lk, H, D, q_seq, q_tok, kv_seq, kv_tok, o_seq,
                                     o_tok, p(kv_off), 1.0, None)
    return getattr(lib, NAME)(p(q), p(k), p(v), p(s), p(s_rcp), p(delta), p(zp), p(xq), p(sx), p(zx), p(R), p(o), n_seq, Lq,
                              Lk, H, D, q_seq, q_tok, kv_seq, kv_tok, o_seq, o_tok, p(kv_off), Kp, n_bits, 1.0, None)


@pytest.mark.parametrize("kw,want", [
    (dict(q=None), EINVAL), (dict(k=None), EINVAL), (dict(v=None), EINVAL), (dict(delta=None), EINVAL),
    (dict(zp=None), EINVAL), (dict(xq=None), EINVAL), (dict(sx=None), EINVAL), (dict(zx=None), EINVAL),
    (dict(R=None), EINVAL), (dict(s=ONE), EINVAL), (dict(s_rcp=ONE), EINVAL),
    (dict(n_seq=0), EINVAL), (dict(Lq=0), EINVAL), (dict(Lk=0), EINVAL), (dict(H=0), EINVAL), (dict(D=0), EINVAL),
    (dict(Kp=0), EINVAL), (dict(Lq=-4), EINVAL),
    # the rules of vq_attn_fwd (o optional)
    (dict(q_tok=148), ESHAPE), (dict(kv_tok=292), ESHAPE), (dict(o=ONE, o_tok=150), ESHAPE), (dict(q_seq=300 * 144 + 4), ESHAPE),
    (dict(q=ONE + 8), ESHAPE), (dict(k=ONE + 4), ESHAPE), (dict(v=ONE + 2), ESHAPE), (dict(o=ONE + 8), ESHAPE),
    (dict(n_seq=65536), ESHAPE), (dict(H=65536, D=16), ESHAPE),
    # the quantizer's
    (dict(Kp=200), ESHAPE), (dict(Kp=128), ESHAPE),                     # Kp % 128, Kp < H * D = 144
    (dict(D=50, Kp=128, q_tok=104, kv_tok=208, o_tok=104), ESHAPE),              # D % 4
    (dict(xq=ONE + 8), ESHAPE), (dict(s=ONE + 8, s_rcp=ONE), ESHAPE), (dict(s=ONE, s_rcp=ONE + 4), ESHAPE),
    (dict(n_seq=40000, Lq=60000), ESHAPE),                              # n_seq * Lq beyond int32
    (dict(n_bits=1), EUNSUP), (dict(n_bits=9), EUNSUP), (dict(n_bits=0), EUNSUP),
    (dict(D=48, Kp=128), EUNSUP), (dict(D=128), EUNSUP),                # head dims without a kernel
])
def test_static_fwd_attention_argument_rules_without_gpu(kw, want):
    """Every refusal returns its code before any HIP call or dereference (the pointers are dummies, no GPU is present)."""
    _, lib = _lib()
    assert _call(lib, **kw) == want


def _regime_shapes(kernel):
    return [(D, sh) for kern, D, sh in ar._SHAPES if kern == kernel]


@pytest.mark.parametrize("kernel", ["VQ_ATTN_K_FWD8_NW4", "VQ_ATTN_K_CROSS_REG"])
def test_routes_without_a_static_form_are_refused(kernel):
    """attn_fwd8_kernel and attn_cross_reg_kernel have no static-grid form: VQ_EUNSUP (the caller keeps two launches),
    and ops.attn_fwd_static_ok says so beforehand."""
    _, lib = _lib()
    from viditq_amd import ops
    ids = ar.kernel_ids()
    shapes = _regime_shapes(kernel)
    assert shapes
    for D, sh in shapes:
        a = ar.fwd_layout(dict(shape=sh, D=D))
        kw = dict(n_seq=a["n_seq"], Lq=a["Lq"], Lk=a["Lk"], H=a["H"], D=D, kv_tok=a["kv_tok"], kv_seq=a["kv_seq"],
                  kv_off=ONE if a["offs"] is not None else None)
        assert _call(lib, fn="vq_attn_fwd_route", **kw) == ids[kernel], (kernel, D, sh)
        assert _call(lib, **kw) == EUNSUP, (kernel, D, sh)
        assert not ops.attn_fwd_static_ok(a["n_seq"], a["Lq"], a["Lk"], a["H"], D, a["q_tok"], a["kv_tok"],
                                          ops.pad128(a["H"] * D), 8, kv_off=a["offs"] is not None)


def test_static_ok_agrees_with_the_entry_point():
    """ops.attn_fwd_static_ok mirrors the entry point's refusals.  (Only refusals are compared where no GPU is present:
    an accepted call would launch.)"""
    _, lib = _lib()
    from viditq_amd import ops
    n_ok = n_no = 0
    for Lq, Lk, kv_off in ((0, 300, False), (300, 0, False), (300, 0, True), (300, 333, False), (150, 333, False),
                           (300, 120, True), (100, 120, False), (2048, 2048, False)):
        for H in (0, 2, 8):
            for D in (16, 48, 50, 72):
                C = H * D
                for Kp in (0, 100, 128, (C + 127) // 128 * 128, 2048):
                    for n_bits in (1, 6, 8, 9):
                        ok = ops.attn_fwd_static_ok(2, Lq, Lk, H, D, C, 2 * C, Kp, n_bits, kv_off=kv_off)
                        if not ok:
                            n_no += 1
                            rc = _call(lib, n_seq=2, Lq=Lq, Lk=Lk, H=H, D=D, Kp=Kp, n_bits=n_bits, q_tok=C, kv_tok=2 * C,
                                       kv_off=ONE if kv_off else None)
                            assert rc < 0, (Lq, Lk, kv_off, H, D, Kp, n_bits)
                        else:       # what the entry point checks, restated
                            n_ok += 1
                            assert Lq > 0 and H > 0 and D in (16, 72) and (Lk > 0 or kv_off)
                            assert Kp % 128 == 0 and Kp >= C and 2 <= n_bits <= 8
                            route = _call(lib, fn="vq_attn_fwd_route", n_seq=2, Lq=Lq, Lk=Lk, H=H, D=D,
                                          kv_off=ONE if kv_off else None)
                            assert route in ops.ATTN_FWD_STATIC_ROUTES
    assert n_ok > 50 and n_no > 50
    # the product launches: spatial 16 x 1024, cross 16384 over <= 120 prompt tokens, PixArt-alpha 512^2
    assert ops.attn_fwd_static_ok(16, 1024, 1024, 16, 72, 3456, 3456, 1152, 8)
    assert ops.attn_fwd_static_ok(1, 16384, 120, 16, 72, 1152, 2304, 1152, 6, kv_off=True)
    assert ops.attn_fwd_static_ok(2, 1024, 120, 16, 72, 1152, 2304, 1152, 8, kv_off=True)
    assert not ops.attn_fwd_static_ok(2, 100, 120, 16, 72, 1152, 2304, 1152, 8, kv_off=True)      # CROSS_REG


def test_block_route_predicate(monkeypatch):
    _lib()
    from viditq_amd.qdiff.quantizer.dynamic_quantizer import DynamicActQuantizer
    from viditq_amd.t2v import stdit
    tw = types.SimpleNamespace(act_quantizer=types.SimpleNamespace(delta=torch.ones(1), zero_point=torch.zeros(1), n_bits=6))
    tok = types.SimpleNamespace(act_quantizer=types.SimpleNamespace(delta=torch.ones(32, 1), zero_point=torch.zeros(32, 1),
                                                                     n_bits=8))
    dyn = types.SimpleNamespace(act_quantizer=object.__new__(DynamicActQuantizer))
    if "VQ_STATIC_FWD_ATTN_QUANT" not in os.environ:
        assert stdit._STATIC_FWD_ATTN_QUANT is False               # the default is off
    calls = []
    fused = lambda d, z, nb, s: calls.append((d, z, nb, s)) or "qa"  # noqa: E731
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", False)
    assert not stdit._static_fwd_attn_quant(tw)
    assert stdit.fwd_attn_quantized_static(tw, None, fused) is None and not calls
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", True)
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", False)        # independent of the temporal switch
    assert stdit._static_fwd_attn_quant(tw)
    assert stdit.fwd_attn_quantized_static(tw, "sv", fused) == "qa"
    assert len(calls) == 1 and calls[0][2] == 6 and calls[0][3] == "sv" and calls[0][0].dtype == torch.float32
    assert not stdit._static_fwd_attn_quant(dyn)                   # dynamic: today's route
    assert not stdit._static_fwd_attn_quant(tok)                   # static per-token grids: today's route
    assert stdit.fwd_attn_quantized_static(dyn, None, fused) is None and stdit.fwd_attn_quantized_static(tok, None, fused) is None
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    assert not stdit._static_fwd_attn_quant(tw)
    assert len(calls) == 1


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_shapes_reach_the_kernel_they_name(i):
    _, lib = _lib()
    from viditq_amd import ops
    case = shape_case(i)
    a = ar.fwd_layout(case)
    kw = dict(n_seq=a["n_seq"], Lq=a["Lq"], Lk=a["Lk"], H=a["H"], D=a["D"], kv_tok=a["kv_tok"], kv_seq=a["kv_seq"],
              kv_off=ONE if a["offs"] is not None else None)
    assert _call(lib, fn="vq_attn_fwd_route", **kw) == ar.kernel_ids()[case["kernel"]]
    assert a["H"] * a["D"] >= 64
    assert ops.attn_fwd_static_ok(a["n_seq"], a["Lq"], a["Lk"], a["H"], a["D"], a["q_tok"], a["kv_tok"],
                                  ops.pad128(a["H"] * a["D"]), 6, kv_off=a["offs"] is not None)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_edge_row_inputs_stay_inside_their_cap(i):
    """The one-hot q / k of the GPU edge-row test: at least 0.9 of the query rows have every head's lead >= R1_GAP, and
    with V = quant_rows.static_rows the oracle's codes of those rows reach both ends of the grid at 8 and 6 bits."""
    from oracle import fakequant as fq
    kern, D, n, Lq, lens, H, kv_off = SHAPES[i]
    sel = one_hot_selected(i)
    assert float(sel.double().mean()) >= 0.9
    hot = one_hot(i)[3]
    for n_bits in (8, 6):
        v, delta, zp = static_v(i, n_bits)
        want = hot_rows(v, hot).reshape(n, Lq, H * D)[sel]
        codes, _ = fq.static_act_quant(want[None].float(), delta, zp, n_bits)
        assert int(codes.min()) == 0 and int(codes.max()) == 2 ** n_bits - 1

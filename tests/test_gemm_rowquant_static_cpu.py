"""CPU-side checks of vq_gemm_i8_rowquant_static (mlp.fc1's GEMM with GELU and fc2's static tensor-wise quantizer in its
epilogue): declared, exported and bound; its refusal table enforced before any device call; ops.gemm_rowquant_static_ok
agreeing with the entry point; the wrapper refusing CPU tensors; the block switch off by default and its predicate."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vq_gemm_i8_rowquant_static"
EINVAL, ESHAPE, EUNSUP = -1, -2, -4
ONE = 1 << 20       # non-null, 16-byte aligned dummy address: the checks must reject before any dereference

# (M, N, K) and variants of the GPU tests: the smallest shapes that reach every form and edge
SHAPES = [((256, 1152, 128), (19, 11)), ((128, 1152, 128), (-1,)), ((300, 1160, 200), (11, 16, -1)), ((64, 256, 64), (-1,))]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L, L.load()


POINTERS = ("xq", "sx", "zx", "R", "wq", "sw", "zw", "cs", "bias", "s", "s_rcp", "delta", "zp", "xq_out", "sx_out", "zx_out",
            "R_out")
REQUIRED = tuple(p for p in POINTERS if p not in ("bias", "s", "s_rcp"))


def _call(lib, M=256, N=1152, K=128, Kp=None, Kp_out=None, w_bits=8, n_bits=8, variant=-1, **ptr):
    Kp = (K + 127) // 128 * 128 if Kp is None else Kp
    Kp_out = (N + 127) // 128 * 128 if Kp_out is None else Kp_out
    vals = dict.fromkeys(POINTERS, ONE)
    vals.update(s=None, s_rcp=None)
    vals.update(ptr)
    p = [None if vals[n] is None else ctypes.c_void_p(vals[n]) for n in POINTERS]
    return getattr(lib, NAME)(*p, M, N, K, Kp, Kp_out, w_bits, n_bits, variant, None)


def test_entry_point_is_declared_exported_and_bound():
    L, lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m, "not declared in include/viditq.h"
    assert hasattr(lib, NAME)
    assert NAME in L.SIGNATURES
    params = [q.strip() for q in m.group(1).split(",")]
    assert len(L.SIGNATURES[NAME][1]) == len(params) == 26
    assert [("*" in q) for q in params] == [True] * 17 + [False] * 8 + [True]     # pointers, extents, stream
    from viditq_amd import ops
    assert callable(ops.gemm_i8_rowquant_static) and callable(ops.gemm_rowquant_static_ok)


@pytest.mark.parametrize("kw,want", [(dict([(p, None)]), EINVAL) for p in REQUIRED] + [
    (dict(M=0), EINVAL), (dict(N=0), EINVAL), (dict(K=0), EINVAL), (dict(Kp=0), EINVAL), (dict(Kp_out=0), EINVAL),
    (dict(M=-256), EINVAL),
    # null pointers come first: a null pointer together with a bad shape or width is VQ_EINVAL
    (dict(xq_out=None, N=1150), EINVAL), (dict(delta=None, n_bits=9), EINVAL),
    # what vq_gemm_i8 refuses
    (dict(Kp=200), ESHAPE), (dict(K=200, Kp=128), ESHAPE), (dict(K=16512), ESHAPE),
    (dict(M=1 << 22, K=1024), ESHAPE), (dict(N=(1 << 22) + 8, K=1024), ESHAPE),          # an operand image of 2^32 bytes
    # the quantizer's
    (dict(N=1156), ESHAPE), (dict(N=1150), ESHAPE), (dict(Kp_out=1200), ESHAPE), (dict(Kp_out=1024), ESHAPE),
    (dict(xq_out=ONE + 8), ESHAPE), (dict(s=ONE + 4, s_rcp=ONE), ESHAPE), (dict(s=ONE, s_rcp=ONE + 8), ESHAPE),
    # variant 19: interior tiles of the 256-row form only
    (dict(variant=19, M=128), ESHAPE), (dict(variant=19, M=300), ESHAPE), (dict(variant=19, N=1160, Kp_out=1280), ESHAPE),
    # a shape error is reported in front of an unsupported width
    (dict(N=1150, n_bits=9), ESHAPE),
    (dict(w_bits=4), EUNSUP), (dict(w_bits=2), EUNSUP), (dict(w_bits=9), EUNSUP), (dict(n_bits=1), EUNSUP),
    (dict(n_bits=9), EUNSUP), (dict(n_bits=0), EUNSUP), (dict(s=ONE), EUNSUP),
    (dict(variant=12), EUNSUP), (dict(variant=0), EUNSUP), (dict(variant=-2), EUNSUP),
])
def test_refusal_table_without_gpu(kw, want):
    """Every refusal returns its code before any HIP call or dereference (the pointers are dummies, no GPU is present)."""
    _, lib = _lib()
    assert _call(lib, **kw) == want


def test_all_null_call_is_einval():
    L, lib = _lib()
    args = [None if ct is ctypes.c_void_p else 1 for ct in L.SIGNATURES[NAME][1]]
    assert getattr(lib, NAME)(*args) == EINVAL


def test_static_ok_agrees_with_the_entry_point():
    """ops.gemm_rowquant_static_ok mirrors the entry point's refusals.  (Only refusals are compared where no GPU is present:
    an accepted call would launch.)"""
    _, lib = _lib()
    from viditq_amd import ops
    n_ok = n_no = 0
    for M in (0, 64, 256, 300, 1 << 22):
        for N in (0, 256, 1150, 1152, 1156, 1160, 4608):
            for K in (0, 64, 1024, 1152, 16384, 16512):
                for w_bits in (2, 4, 6, 8, 9):
                    for n_bits in (1, 2, 6, 8, 9):
                        for variant in (-1, 11, 16, 19, 12):
                            ok = ops.gemm_rowquant_static_ok(M, N, K, w_bits, n_bits, variant=variant)
                            if not ok:
                                n_no += 1
                                assert _call(lib, M=M, N=N, K=K, w_bits=w_bits, n_bits=n_bits, variant=variant) < 0, \
                                    (M, N, K, w_bits, n_bits, variant)
                            else:       # what the entry point checks, restated
                                n_ok += 1
                                assert M > 0 and N > 0 and 0 < K <= 16384 and N % 8 == 0
                                assert M * ops.pad128(K) < 1 << 32 and N * ops.pad128(K) < 1 << 32
                                assert 4 < w_bits <= 8 and 2 <= n_bits <= 8 and variant in (-1, 11, 16, 19)
                                assert variant != 19 or (M % 256 == 0 and N % 288 == 0)
    assert n_ok > 200 and n_no > 200
    # the product launches (fc1 of STDiT 16x512x512 and of PixArt at 512 / 1024 px), and the GPU tests' shapes
    for M in (16384, 32768, 2048, 8192):
        assert ops.gemm_rowquant_static_ok(M, 4608, 1152, 8, 8) and ops.gemm_rowquant_static_ok(M, 4608, 1152, 6, 6)
    for (M, N, K), variants in SHAPES:
        for v in variants:
            assert ops.gemm_rowquant_static_ok(M, N, K, 8, 8, variant=v), (M, N, K, v)
    assert not ops.gemm_rowquant_static_ok(16384, 4608, 1152, 4, 8)          # nibble weights: out of scope


def test_wrapper_refuses_cpu_tensors():
    _lib()
    from viditq_amd import ops
    a = ops.QAct(torch.zeros(4, 128, dtype=torch.int8), torch.ones(4), torch.zeros(4, dtype=torch.int32),
                 torch.zeros(4, dtype=torch.int32), 64)
    w = ops.PackedWeight(torch.zeros(8, 128, dtype=torch.int8), torch.ones(8), torch.zeros(8, dtype=torch.int32),
                         torch.zeros(8, dtype=torch.int32), 8, 64, 128, 8)
    with pytest.raises(ops.VQError):
        ops.gemm_i8_rowquant_static(a, w, None, torch.ones(1), torch.zeros(1), 8)


def test_switch_is_off_by_default_and_the_block_predicate(monkeypatch):
    _lib()
    from viditq_amd import ops
    from viditq_amd.qdiff.quantizer.dynamic_quantizer import DynamicActQuantizer
    from viditq_amd.t2v import stdit
    if "VQ_STATIC_GEMM_QUANT" not in os.environ:
        assert stdit._STATIC_GEMM_QUANT is False                   # the default is off
    fc1 = types.SimpleNamespace(bias_f32=lambda: "bias")
    pw = types.SimpleNamespace(N=256, K=64, n_bits=8)
    pw_w4 = types.SimpleNamespace(N=256, K=64, n_bits=4)
    tw = types.SimpleNamespace(act_quantizer=types.SimpleNamespace(delta=torch.ones(1), zero_point=torch.zeros(1), n_bits=6))
    run = types.SimpleNamespace(act_quantizer=tw.act_quantizer, smooth_quant_running_stat=True)
    tok = types.SimpleNamespace(act_quantizer=types.SimpleNamespace(delta=torch.ones(32, 1), zero_point=torch.zeros(32, 1),
                                                                     n_bits=8))
    dyn = types.SimpleNamespace(act_quantizer=object.__new__(DynamicActQuantizer))
    calls = []
    monkeypatch.setattr(ops, "gemm_i8_rowquant_static", lambda *a, **k: calls.append((a, k)) or "qa")
    qa = types.SimpleNamespace(rows=64)
    monkeypatch.setattr(stdit, "_STATIC_GEMM_QUANT", False)
    assert not stdit._static_gemm_quant(pw, tw, 64)
    assert stdit.mlp_quantized_static(fc1, tw, qa, pw, None) is None and not calls
    monkeypatch.setattr(stdit, "_STATIC_GEMM_QUANT", True)
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", False)        # independent of the attention switches
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", False)
    assert stdit._static_gemm_quant(pw, tw, 64)
    assert stdit.mlp_quantized_static(fc1, tw, qa, pw, "s2") == "qa"
    (a, k), = calls
    assert a[0] is qa and a[1] is pw and a[2] == "bias" and a[5] == 6 and k == dict(s="s2") and a[3].dtype == torch.float32
    assert not stdit._static_gemm_quant(pw, dyn, 64)               # dynamic: today's route
    assert not stdit._static_gemm_quant(pw, tok, 64)               # static per-token grids: today's route
    assert not stdit._static_gemm_quant(pw, run, 64)               # a running statistic on fc2: today's route
    assert not stdit._static_gemm_quant(pw_w4, tw, 64)             # nibble weights: the predicate refuses
    assert stdit.mlp_quantized_static(fc1, tw, qa, pw_w4, None) is None
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    assert not stdit._static_gemm_quant(pw, tw, 64)
    assert len(calls) == 1

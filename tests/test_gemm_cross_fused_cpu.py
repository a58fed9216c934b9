"""The route predicate of the fused q_linear + cross attention launch (viditq_amd.t2v.stdit._cross_q_fused): pure host
arithmetic.  It must refuse the tiny models whose ordered launch lists tests/test_block_trace_gpu.py pins - before any
call into ``ops``, an ``*_ok`` query included - and accept the shapes of the benchmark."""
import types

import pytest
import torch

import block_trace_cases as btc


def _models_of(fn, seen=None):
    """The QuantModel(s) a case's run function closes over (directly or through the helper functions it closes over)."""
    seen = set() if seen is None else seen
    out = []
    for cell in fn.__closure__ or ():
        try:
            v = cell.cell_contents
        except ValueError:
            continue
        if id(v) in seen:
            continue
        seen.add(id(v))
        if isinstance(v, torch.nn.Module) and hasattr(v, "model") and hasattr(v.model, "blocks"):
            out.append(v)
        elif isinstance(v, types.FunctionType):
            out += _models_of(v, seen)
    return out


def _ops_raise(monkeypatch):
    """Every public function of ``ops`` raises: the predicate must not get that far."""
    import viditq_amd  # noqa: F401
    from viditq_amd import ops

    def boom(*a, **k):
        raise AssertionError("the route predicate called into ops")
    for name, fn in list(vars(ops).items()):
        if not name.startswith("_") and isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__:
            monkeypatch.setattr(ops, name, boom)
    return ops


@pytest.fixture
def ops_raise(monkeypatch):
    return _ops_raise(monkeypatch)


def _tiny_cross_attn():
    """The geometry every traced model shares (block_trace_cases: hidden 64, 4 heads), for the cases whose builders quantize
    their weights with the library's kernels and so cannot be built without a GPU."""
    return types.SimpleNamespace(core=types.SimpleNamespace(num_heads=4, head_dim=16),
                                 q_linear=types.SimpleNamespace(in_features=64), proj=object())


@pytest.mark.parametrize("name", btc.NAMES)
def test_predicate_refuses_the_traced_tiny_models(name, monkeypatch):
    """Every cross-attention stage of every traced case, for one and for two samples, at the token counts of the tiny models
    and at multiples of 256 (the refusal must come from the models' heads of 16, not from a token count), with the switch
    on and the static fused arm out of the way."""
    from viditq_amd.t2v import stdit
    monkeypatch.setattr(stdit, "_CROSS_Q_FUSED", True)
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", False)
    _, build, _ = btc.CASES[btc.NAMES.index(name)]
    try:
        with torch.no_grad():
            stages = [blk.cross_attn for qnn in _models_of(build(torch.device("cpu"))) for blk in qnn.model.blocks]
    except Exception as e:  # noqa: BLE001  (a builder that needs the GPU)
        print("%s: not buildable on the CPU (%s: %s) - the shared geometry of the tiny models" % (name, type(e).__name__, e))
        stages = []
    stages = stages or [_tiny_cross_attn()]
    _ops_raise(monkeypatch)
    n = 0
    monkeypatch.setattr(stdit, "_CROSS_Q_FUSED_ROUND", 1)            # (nor from the tile count)
    for ca in stages:
        assert ca.core.num_heads == 4 and ca.core.num_heads * ca.core.head_dim == 64
        for B in (1, 2):
            for N in (16, 64, 128, 256, 512, 1024):
                assert not stdit._cross_q_fused(ca, B, N)
                n += 1
    assert n > 0


def test_shape_predicate_clause_by_clause(ops_raise):
    from viditq_amd.t2v.stdit import _cross_q_fused_shape as ok
    assert ok(16, 72, 1152, 1, 16384) and ok(16, 72, 1152, 1, 16384, 120)      # the benchmark: STDiT-XL/2 16 x 512 x 512, one sample
    assert ok(16, 72, 1152, 2, 16384, 120) and ok(16, 72, 1152, 2, 256, 128)    # a joint forward; PixArt-alpha 256 x 256
    assert ok(16, 72, 1152, 2, 4096) and ok(4, 72, 288, 1, 256, 1)
    assert not ok(16, 72, 1152, 1, 16384, 129) and not ok(16, 72, 1152, 2, 4096, 300)   # PixArt-Sigma's prompts
    assert not ok(16, 72, 1152, 1, 16384, 0)
    assert not ok(4, 16, 64, 1, 256) and not ok(18, 64, 1152, 1, 256)           # heads of 72 only
    assert not ok(5, 72, 360, 1, 256) and not ok(2, 72, 144, 1, 256)            # whole 288-column tiles
    assert not ok(16, 72, 1152, 1, 255) and not ok(16, 72, 1152, 2, 384) and not ok(16, 72, 1152, 1, 0)
    assert not ok(16, 72, 20000, 1, 256)                                        # K <= 16384
    assert not ok(16, 72, 16384, 1, 1 << 18)                                    # the token image stays below 2^32 bytes


def test_switch_and_static_arm(ops_raise, monkeypatch):
    """On and off with the switch; out of the way where the static fused attention launch serves proj; and only at tile
    counts where the launch was measured faster than the pair."""
    from viditq_amd.t2v import stdit

    class _Core:
        num_heads, head_dim = 16, 72

    class _Lin:
        in_features = 1152

    ca = types.SimpleNamespace(core=_Core(), q_linear=_Lin(), proj=object())
    monkeypatch.setattr(stdit, "_static_fwd_attn_quant", lambda proj: False)
    monkeypatch.setattr(stdit, "_CROSS_Q_FUSED", True)
    assert stdit._cross_q_fused(ca, 1, 16384)
    monkeypatch.setattr(stdit, "_CROSS_Q_FUSED", False)
    assert not stdit._cross_q_fused(ca, 1, 16384)
    monkeypatch.setattr(stdit, "_CROSS_Q_FUSED", True)
    monkeypatch.setattr(stdit, "_static_fwd_attn_quant", lambda proj: True)
    assert not stdit._cross_q_fused(ca, 1, 16384)
    # whole rounds of 256 tiles only: the benchmark's one and the joint forward's two; not PixArt's 32 or 128 tiles
    monkeypatch.setattr(stdit, "_static_fwd_attn_quant", lambda proj: False)
    assert stdit._cross_q_fused(ca, 1, 16384) and stdit._cross_q_fused(ca, 2, 16384)
    assert not stdit._cross_q_fused(ca, 2, 1024) and not stdit._cross_q_fused(ca, 2, 4096) and not stdit._cross_q_fused(ca, 1, 16640)

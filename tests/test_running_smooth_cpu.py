"""CPU checks behind test_running_smooth_gpu.py: the expectations of running_stat_cases.py ARE the reference's running
statistic (QuantLayer._update_running_act_scale + the zero patch of QuantLayer.channel_wise_scale, run on the CPU), the
entry point's refusals come before any HIP call, and the opt-in route predicate of the block classes."""
import ctypes
import os
import types

import pytest
import torch

import running_stat_cases as rc

EINVAL, ESHAPE = -1, -2
ONE = 256           # non-null, 16-byte aligned dummy address: the checks must reject before any dereference


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L
    return L, L.load()


# ------------------------------------------------------------------------------------------------ the model is the reference
def _reference_layer(C):
    """What the two reference methods read of a QuantLayer, as a stub they are called on unbound."""
    from viditq_amd.qdiff.models.quant_layer import QuantLayer
    stub = types.SimpleNamespace(act_quantizer=types.SimpleNamespace(act_scale=None), timerange_num=1,
                                 smooth_quant_momentum=rc.MOMENTUM, channel_wise_scale_type="momentum_act_max",
                                 _master_weight=lambda: torch.ones(1, C))
    return QuantLayer, stub


def reference_step(QL, stub, x):
    """One forward's worth of the statistic on the device of x: the update, then the zero patch (in place)."""
    QL._update_running_act_scale(stub, x, 0)
    QL.channel_wise_scale(stub, 0, 0.5)
    return stub.act_quantizer.act_scale[0].reshape(-1)


@pytest.mark.parametrize("name", rc.NAMES)
def test_cases_equal_the_reference_statistic_on_the_cpu(name):
    xs, init = rc.inputs(name)
    C = init.numel()
    QL, stub = _reference_layer(C)
    if (init != 0).any():
        stub.act_quantizer.act_scale = init.clone().reshape(1, 1, C)
    exp = rc.expected(name, xs, init)
    for j, x in enumerate(xs):
        x0 = x.clone()
        got = reference_step(QL, stub, x)
        assert torch.equal(got, exp[j][0]), (name, j, float((got - exp[j][0]).abs().max()))
        assert torch.equal(x.abs().amax(dim=-2).float().mean(dim=0), exp[j][1]), (name, j)
        assert torch.equal(x.view(torch.int16), x0.view(torch.int16))
    assert all(torch.isfinite(e[0]).all() and (e[0] != 0).all() for e in exp)


def test_case_families_are_what_their_names_say():
    exp = rc.expected("zero_column/B2_n37_C72")
    assert exp[0][0][3] == 1.0e-5 and exp[0][0][71] == 1.0e-5 and exp[0][0][5] == 1.0e-5          # the patch fired
    assert 0 < exp[1][0][3] < 1.0e-5 and 0 < exp[2][0][3] < exp[1][0][3]                          # ... and then persists, decaying
    assert exp[1][0][5] > 1e-2                                                                    # (zero in the first call only)
    exp = rc.expected("extremes/B2_n37_C72")
    assert exp[0][1][0] == 65504.0 / 2 and exp[0][1][1] == 0 and exp[0][0][1] == 1.0e-5
    assert exp[0][1][2] == (0x200 + 0x3ff) * 2.0 ** -24 / 2 and exp[0][1][3] == 2.0 ** -24 / 2 and exp[0][1][4] == 65504.0
    for fam in ("peak_first_row", "peak_last_row", "peak_last_row_of_sample0"):
        exp = rc.expected(fam + "/B2_n300_C1152")
        assert exp[0][1][0] > 500 and exp[0][1][1] > 500                                          # (1000 + <= 8) / 2
    xs, init = rc.inputs("one_nonzero_entry/B2_n37_C72")
    exp = rc.expected("one_nonzero_entry/B2_n37_C72", xs, init)
    cur = exp[0][1]
    assert not torch.equal(exp[0][0], cur) and torch.allclose(exp[0][0][:36], cur[:36] * 0.05, rtol=1e-6)   # momentum, not init
    # several workgroups meet in one column: more rows than one workgroup's slab at every width
    assert sum(1 for n in rc.NAMES if "_n300_" in n or "_n1025_" in n) >= 24


# ------------------------------------------------------------------------------------------------ ABI without a GPU
def _call(lib, x=ONE, act=ONE, cur=None, scratch=ONE, mom=0.95, B=2, n_tok=16, C=64):
    p = lambda a: None if a is None else ctypes.c_void_p(a)  # noqa: E731
    return lib.vq_act_scale_momentum(p(x), p(act), p(cur), p(scratch), mom, 1.0 - mom, B, n_tok, C, None)


@pytest.mark.parametrize("kw,want", [
    (dict(x=None, act=None, scratch=None), EINVAL), (dict(x=None), EINVAL), (dict(act=None), EINVAL),
    (dict(scratch=None), EINVAL), (dict(x=None, C=12), EINVAL),                                   # null pointers first
    (dict(B=0), EINVAL), (dict(n_tok=0), EINVAL), (dict(C=0), EINVAL), (dict(C=-8), EINVAL),
    (dict(mom=-0.01), EINVAL), (dict(mom=1.5), EINVAL), (dict(mom=float("nan")), EINVAL),
    (dict(C=12), ESHAPE), (dict(C=4604), ESHAPE), (dict(x=ONE + 8), ESHAPE), (dict(x=ONE + 2), ESHAPE),
])
def test_entry_point_refuses_before_any_hip_call(kw, want):
    """Every refusal returns its code before any HIP call or dereference (the pointers are dummies, no GPU is present)."""
    _, lib = _lib()
    assert _call(lib, **kw) == want


def test_entry_point_is_declared_bound_and_wrapped():
    L, lib = _lib()
    assert hasattr(lib, "vq_act_scale_momentum") and len(L.SIGNATURES["vq_act_scale_momentum"][1]) == 10
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viditq.h")).read()
    for cite in ("quant_layer.py:118-126", ":147-154", ":128-133"):
        assert cite in src.split("int vq_act_scale_momentum")[0].rsplit("/* ----", 1)[1]
    from viditq_amd import ops
    assert callable(ops.act_scale_momentum)


# ------------------------------------------------------------------------------------------------ host logic on stub layers
class _Layer:
    """A hot layer as the route predicates see it."""

    def __init__(self, running=False, device_ok=True):
        from viditq_amd.qdiff.quantizer.dynamic_quantizer import DynamicActQuantizer
        self.act_quantizer = object.__new__(DynamicActQuantizer)
        self.smooth_quant_running_stat = running
        self._device_ok = device_ok
        self.asked = 0

    def int_route_ok(self):
        return True

    def running_stat_device_ok(self):
        self.asked += 1
        return self._device_ok and self.smooth_quant_running_stat


def _stub_block(cls, names):
    from viditq_amd.qdiff.models.quant_layer import QuantLayer
    blk = object.__new__(cls)
    torch.nn.Module.__init__(blk)
    layers = {}
    for n in names:
        lay = object.__new__(type("L", (_Layer, QuantLayer), {}))          # isinstance(., QuantLayer) without its constructor
        torch.nn.Module.__init__(lay)
        _Layer.__init__(lay)
        layers[n] = lay
    return blk, layers


def _pixart_block():
    from viditq_amd.t2i import pixart
    names = ["attn.qkv", "attn.proj", "cross_attn.q_linear", "cross_attn.kv_linear", "cross_attn.proj", "mlp.fc1", "mlp.fc2"]
    blk, L = _stub_block(pixart.PixArtMSBlock, names)
    for grp in ("attn", "cross_attn", "mlp"):
        object.__setattr__(blk, grp, types.SimpleNamespace(**{n.split(".")[1]: l for n, l in L.items() if n.startswith(grp + ".")}))
    return blk, L


def _stdit_block():
    from viditq_amd.t2v import stdit
    names = ["attn.q", "attn.k", "attn.v", "attn.proj", "attn_temp.q", "attn_temp.k", "attn_temp.v", "attn_temp.proj",
             "cross_attn.q_linear", "cross_attn.kv_linear", "cross_attn.proj", "mlp.fc1", "mlp.fc2"]
    blk, L = _stub_block(stdit.STDiTBlock, names)
    for n, lay in L.items():
        lay.act_quantizer.n_bits = 8
    for grp in ("attn", "attn_temp", "cross_attn", "mlp"):
        object.__setattr__(blk, grp, types.SimpleNamespace(**{n.split(".")[1]: l for n, l in L.items() if n.startswith(grp + ".")}))
    return blk, L


@pytest.mark.parametrize("make", [_pixart_block, _stdit_block], ids=["pixart", "stdit"])
def test_route_predicate_is_opt_in_and_tolerates_fc2_only(make, monkeypatch):
    from viditq_amd.t2v import stdit
    if "VQ_RUNNING_SMOOTH_DEVICE" not in os.environ:
        assert stdit._RUNNING_SMOOTH_DEVICE is False                   # the default is off
    blk, L = make()
    fc2, proj = L["mlp.fc2"], L["attn.proj"]
    consulted = []
    orig = type(blk).fused_running_ok
    monkeypatch.setattr(type(blk), "fused_running_ok", lambda self: consulted.append(1) or orig(self))

    # nothing runs a statistic: fused either way, the new predicate agrees and is not needed
    for flag in (False, True):
        monkeypatch.setattr(stdit, "_RUNNING_SMOOTH_DEVICE", flag)
        assert blk.fused_ok() and stdit.takes_fused(blk)
    assert consulted == [] and orig(blk)

    fc2.smooth_quant_running_stat = True
    monkeypatch.setattr(stdit, "_RUNNING_SMOOTH_DEVICE", False)
    assert not blk.fused_ok() and not stdit.takes_fused(blk)
    assert consulted == [] and fc2.asked == 0                          # flag off: never consulted
    monkeypatch.setattr(stdit, "_RUNNING_SMOOTH_DEVICE", True)
    assert not blk.fused_ok() and stdit.takes_fused(blk) and consulted == [1]
    fc2._device_ok = False                                             # e.g. the fp16 master weight was released
    assert not blk.fused_ok() and not stdit.takes_fused(blk)
    fc2._device_ok = True

    fc2.smooth_quant_running_stat = False
    proj.smooth_quant_running_stat = True                              # any other hot layer: the layerwise route
    assert not blk.fused_ok() and not stdit.takes_fused(blk)
    fc2.smooth_quant_running_stat = True
    assert not blk.fused_ok() and not stdit.takes_fused(blk)


def test_layer_predicate_reads_host_fields_only():
    """QuantLayer.running_stat_device_ok on a real layer (CPU weights: never the device route), field by field."""
    import viditq_amd  # noqa: F401
    from viditq_amd.config import to_config
    from viditq_amd.qdiff.models.quant_layer import QuantLayer
    wq = to_config(dict(n_bits=4, per_group="channel", channel_dim=0, scale_method="min_max", round_mode="nearest"))
    aq = to_config(dict(n_bits=8, per_group="token", scale_method="min_max", round_mode="nearest_ste", running_stat=False,
                        dynamic=True, sym=False, n_spatial_token=16, n_temporal_token=1, n_prompt=12,
                        smooth_quant=dict(enable=True, channel_wise_scale_type="momentum_act_max", momentum=0.95, alpha=0.3)))
    layer = QuantLayer(torch.nn.Linear(256, 64).half(), wq, aq)
    assert not layer.running_stat_device_ok()                          # no statistic running
    layer.smooth_quant_running_stat = True
    assert not layer.running_stat_device_ok()                          # not on the integer route yet
    with pytest.raises(RuntimeError):
        layer.running_stat_step(torch.zeros(1, 4, 256, dtype=torch.float16))
    plain = QuantLayer(torch.nn.Linear(256, 64).half(), wq, to_config(dict(aq, smooth_quant=dict(enable=False))))
    plain.smooth_quant_running_stat = True                             # set by a script on a layer built without smooth quant
    assert not plain.running_stat_device_ok()

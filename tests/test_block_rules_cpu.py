"""The route rules of the fused blocks, on stub layers (the kind test_running_smooth_cpu.py builds): ``fused_rules(block)``
answers what ``fused_ok()`` answers and ``fused_rules(block, running=True)`` what ``fused_running_ok()`` answers, for both
block classes, over the product of everything that vetoes the fused route; and the two quantizer predicates the route
predicates share.

Every rule is a veto (no rule ever turns a refused block back into an accepted one), so a combination is accepted exactly
when each of its parts is: the tables below give the answer of each part, the test asserts the conjunction for every
combination."""
import itertools
import types

import pytest
import torch

from test_running_smooth_cpu import _pixart_block, _stdit_block

YES, NO, RUNNING_ONLY = (True, True), (False, False), (False, True)          # (fused_ok, fused_running_ok)


def _static(per_group, n_bits=8, n_grid=1):
    return types.SimpleNamespace(per_group=per_group, n_bits=n_bits, delta=torch.ones(n_grid), zero_point=torch.zeros(n_grid))


def _set_aq(lay, aq):
    lay._modules.pop("act_quantizer", None)          # (the stub's own quantizer is a registered child module)
    lay.__dict__["act_quantizer"] = aq


# ---- one layer that is not what the route needs: (what, where) -> answer
def _not_a_quant_layer(blk, L, name):
    grp, leaf = name.split(".")
    setattr(getattr(blk, grp), leaf, torch.nn.Linear(4, 4))


def _int_route_false(blk, L, name):
    L[name].int_route_ok = lambda: False


def _static_per_group(blk, L, name):
    _set_aq(L[name], _static("token"))


def _static_tensor_wise(blk, L, name):               # allowed (on q, k and v at once it is the q/k/v axis below)
    _set_aq(L[name], _static(False))


LAYER = [(None, None, YES)] + [(f, n, a) for f, a in ((_not_a_quant_layer, NO), (_int_route_false, NO), (_static_per_group, NO),
                                                      (_static_tensor_wise, YES))
                               for n in ("attn.proj", "cross_attn.kv_linear", "mlp.fc2")]

# ---- a running statistic: (layers it runs on, running_stat_device_ok of those layers) -> answer
RUNNING = [((), True, YES), (("mlp.fc2",), True, RUNNING_ONLY), (("mlp.fc2",), False, NO), (("attn.proj",), True, NO),
           (("mlp.fc1",), True, NO), (("mlp.fc2", "attn.proj"), True, NO)]

# ---- STDiT's q, k, v of one attention: ((n_bits, dynamic) of q, k, v) -> answer
QKV = [(("attn", ((8, True), (8, True), (8, True))), YES),
       (("attn", ((8, True), (6, True), (8, True))), NO),                      # mixed bit widths
       (("attn_temp", ((8, True), (8, True), (8, False))), NO),                # mixed kinds
       (("attn_temp", ((6, False), (6, False), (6, False))), YES),             # all static tensor-wise, one width
       (("attn_temp", ((8, False), (6, False), (8, False))), NO)]


def _apply(blk, L, layer, running, qkv=None):
    fault, where, _ = layer
    if qkv is not None:
        (att, kinds), _ = qkv
        for leaf, (bits, dynamic) in zip("qkv", kinds):
            lay = L[att + "." + leaf]
            if dynamic:
                lay.act_quantizer.n_bits = bits
            else:
                _set_aq(lay, _static(False, bits))
    names, device_ok, _ = running
    for n in names:
        L[n].smooth_quant_running_stat = True
        L[n]._device_ok = device_ok
    if fault is not None:
        fault(blk, L, where)


def _check(blk, want, qkv_rule=lambda: True):
    """``want``: (fused_ok, fused_running_ok) of the table.  The per-layer loop is fused_rules; STDiT's q | k | v rule
    (``qkv_rule``; asked only of a block that passed the loop, whose q, k, v then are QuantLayers) comes on top."""
    from viditq_amd.t2v import stdit
    ok, run = want
    assert (stdit.fused_rules(blk) and qkv_rule()) == blk.fused_ok() == ok
    assert (stdit.fused_rules(blk, running=True) and qkv_rule()) == blk.fused_running_ok() == run
    assert stdit.fused_running_rules(blk) == stdit.fused_rules(blk, running=True)


PAIRS = list(itertools.product(LAYER, RUNNING))
PAIR_IDS = ["%s@%s+running@%s%s" % (getattr(f, "__name__", "sound").strip("_"), n, "|".join(names) or "none", "" if dev else "(not served)")
            for (f, n, _), (names, dev, _) in PAIRS]
QKV_IDS = ["%s:%s" % (att, "".join("%d%s" % (b, "d" if d else "s") for b, d in kinds)) for (att, kinds), _ in QKV]


@pytest.mark.parametrize("layer,running", PAIRS, ids=PAIR_IDS)
def test_pixart_rules(layer, running):
    blk, L = _pixart_block()
    _apply(blk, L, layer, running)
    _check(blk, tuple(a and b for a, b in zip(layer[2], running[2])))


@pytest.mark.parametrize("qkv", QKV, ids=QKV_IDS)
@pytest.mark.parametrize("layer,running", PAIRS, ids=PAIR_IDS)
def test_stdit_rules(layer, running, qkv):
    blk, L = _stdit_block()
    _apply(blk, L, layer, running, qkv)
    _check(blk, tuple(a and b and c for a, b, c in zip(layer[2], running[2], qkv[1])), blk._qkv_share_quantizer)


def test_stdit_rules_are_fused_rules_plus_the_qkv_helper():
    """fused_rules itself does not look at q | k | v (PixArt has one fused Linear): STDiT adds its own check."""
    from viditq_amd.t2v import stdit
    blk, L = _stdit_block()
    L["attn.k"].act_quantizer.n_bits = 6
    assert stdit.fused_rules(blk) and stdit.fused_rules(blk, running=True)
    assert not blk.fused_ok() and not blk.fused_running_ok()


def test_a_running_statistic_is_asked_about_only_where_it_is_tolerated():
    from viditq_amd.t2v import stdit
    for make in (_pixart_block, _stdit_block):
        blk, L = make()
        L["mlp.fc2"].smooth_quant_running_stat = L["attn.proj"].smooth_quant_running_stat = True
        assert not stdit.fused_rules(blk) and L["mlp.fc2"].asked == 0 and L["attn.proj"].asked == 0
        assert not stdit.fused_rules(blk, running=True) and L["attn.proj"].asked == 0


# ---------------------------------------------------------------------------------------------------- the two predicates
def _dynamic(n_bits):
    from viditq_amd.qdiff.quantizer.dynamic_quantizer import DynamicActQuantizer
    aq = object.__new__(DynamicActQuantizer)
    torch.nn.Module.__init__(aq)
    aq.n_bits = n_bits
    return aq


def test_tensorwise_static():
    from viditq_amd.t2v import stdit
    assert stdit._tensorwise_static(_static(False))
    assert stdit._tensorwise_static(_static(False, 6))
    assert not stdit._tensorwise_static(_dynamic(8))
    assert not stdit._tensorwise_static(_static("token", n_grid=12))                        # per-token: one grid per prompt token
    assert not stdit._tensorwise_static(types.SimpleNamespace(delta=torch.ones(12), zero_point=torch.zeros(1)))
    assert not stdit._tensorwise_static(types.SimpleNamespace(delta=torch.ones(1), zero_point=torch.zeros(12)))


def test_same_dynamic():
    from viditq_amd.t2v import stdit
    lay = lambda aq: types.SimpleNamespace(act_quantizer=aq)  # noqa: E731
    assert stdit._same_dynamic([lay(_dynamic(8))])
    assert stdit._same_dynamic([lay(_dynamic(6)), lay(_dynamic(6)), lay(_dynamic(6))])
    assert not stdit._same_dynamic([lay(_dynamic(8)), lay(_dynamic(6)), lay(_dynamic(8))])  # mixed widths
    assert not stdit._same_dynamic([lay(_dynamic(8)), lay(_static(False)), lay(_dynamic(8))])   # mixed kinds
    assert not stdit._same_dynamic([lay(_static(False)), lay(_static(False))])              # tensor-wise
    assert not stdit._same_dynamic([lay(_static("token", n_grid=12))])                      # per-token static


def test_the_route_predicates_answer_through_them(monkeypatch):
    """The four static predicates refuse a dynamic, a per-token and a mixed set before they ask ops anything."""
    from viditq_amd import ops
    from viditq_amd.t2v import stdit
    for sw in ("_STATIC_FUSED", "_STATIC_ATTN_QUANT", "_STATIC_FWD_ATTN_QUANT", "_STATIC_GEMM_QUANT"):
        monkeypatch.setattr(stdit, sw, True)
    asked = []
    for fn in ("attn_temporal_static_ok", "gemm_rowquant_static_ok", "rowquant_static_ok"):
        monkeypatch.setattr(ops, fn, lambda *a, _fn=fn, **k: asked.append(_fn) or True)
    lay = lambda aq: types.SimpleNamespace(act_quantizer=aq, smooth_quant_running_stat=False)  # noqa: E731
    pw1 = types.SimpleNamespace(N=256, K=64, n_bits=8)
    for aq in (_dynamic(8), _static("token", n_grid=12)):
        assert not stdit._static_attn_quant(lay(aq), 4, 4, 16) and not stdit._static_fwd_attn_quant(lay(aq))
        assert not stdit._static_gemm_quant(pw1, lay(aq), 64) and not stdit._static_one_pass([lay(aq)], 64)
    assert not stdit._static_one_pass([lay(_static(False)), lay(_dynamic(8))], 64)
    assert not stdit._static_one_pass([lay(_static(False)), lay(_static(False, 6))], 64)
    assert asked == []
    tw = lay(_static(False))
    assert stdit._static_attn_quant(tw, 4, 4, 16) and stdit._static_fwd_attn_quant(tw)
    assert stdit._static_gemm_quant(pw1, tw, 64) and stdit._static_one_pass([tw, lay(_static(False))], 64)
    assert asked == ["attn_temporal_static_ok", "gemm_rowquant_static_ok", "rowquant_static_ok"]

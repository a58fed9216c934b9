"""The fused DPM-Solver++ step without a GPU: the exact cases prove themselves, the coefficient table + order schedule +
history rotation reproduce the eager solver bit for bit through the CPU model of dpm_step_cases.py, the entry points
refuse bad arguments in the documented order before any HIP call, and the route is off unless asked for."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dpm_step_cases as dc
from helpers import _FakeTensor


@pytest.mark.parametrize("case", dc.d1_cases(), ids=lambda c: c.name)
def test_d1_cases_are_exact_in_fp16_and_fp32(case):
    big = dc.d1_prove(case)
    assert 0 < big < 2.0 ** 11


def test_d1_operands_encode_their_position():
    c = dc.D1Case((2, 3, 7), 2, False, 1)
    flat = np.concatenate([c.eps.reshape(-1), c.x.reshape(-1)])
    assert np.array_equal(flat * 16, np.round(flat * 16)) and np.abs(flat).max() <= 8
    # neighbours along every axis and the two batch halves differ
    assert (c.eps[0] != c.eps[2]).all() and (c.eps[0] != c.eps[1]).all()
    assert (c.x[:, 0] != c.x[:, 1]).all() and (c.x[..., 0] != c.x[..., 1]).all()
    assert not np.array_equal(c.hist[0], c.hist[1]) and not np.array_equal(c.hist[1], c.hist[2])


def test_order_schedule_of_the_table():
    s = dc.make_solver()
    assert s.multistep_orders(5, 2, True) == [1, 2, 2, 2, 1]
    assert s.multistep_orders(5, 3, True) == [1, 2, 3, 2, 1]
    assert s.multistep_orders(5, 3, False) == [1, 2, 3, 3, 3]
    assert s.multistep_orders(3, 3, True) == [1, 2, 1]
    assert s.multistep_orders(4, 1, True) == [1, 1, 1, 1]
    rows = s.multistep_rows(5, 3, "time_uniform", None, None, True, "dpmsolver")
    assert tuple(rows.shape) == (5, dc.ROW) and rows.dtype == torch.float32
    assert rows[:, dc.ORDER].tolist() == [1, 2, 3, 2, 1] and rows[:, dc.CFG].tolist() == [4.5] * 5
    assert torch.equal(rows[:, dc.INV_ALPHA], torch.tensor(1.0) / rows[:, dc.ALPHA])
    ts = s.time_steps("time_uniform", 1.0, 1e-3, 5)
    want = [float((ts[k + 1].float() - 1.0 / 1000) * 1000.0) for k in range(5)]
    assert rows[:, dc.T_NEXT].tolist() == want
    assert s.multistep_rows(5, 2, "time_uniform", None, None, True, "taylor")[:, dc.TAYLOR].tolist() == [1.0] * 5


@pytest.mark.parametrize("half", [True, False], ids=["fp16model", "fp32model"])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("solver_type", ["dpmsolver", "taylor"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_table_reproduces_the_eager_solver_bit_for_bit(order, solver_type, lower, half):
    """CPU model x multistep_rows == sample(fused=False) on CPU tensors (torch's CPU path divides by alpha_t)."""
    calls = []
    s = dc.make_solver(4.5, dc.analytic_model(half, calls))
    x = torch.from_numpy(dc.gauss((2, 4, 3, 5), seed=order))
    for steps in sorted({order, 5, 20}):
        del calls[:]
        want = s.sample(x, steps=steps, order=order, lower_order_final=lower, solver_type=solver_type, fused=False)
        t_eager = [float(t[0]) for t in calls]
        del calls[:]
        got = dc.run_table(s, x, steps, order, lower, solver_type, half)
        assert [float(t[0]) for t in calls] == t_eager and len(t_eager) == steps
        assert want.dtype == torch.float32 and torch.equal(got, want), (steps, float((got - want).abs().max()))


# ---------------------------------------------------------------------------------------------------- refusals
GOOD = 1 << 20


def _step_args(**kw):
    a = dict(eps=GOOD, x=GOOD, hist=GOOD, coef=GOOD, step=None, x_out=GOOD, x_model=None, n=1, C=4, inner=8, ld_eps=32,
             row=0, n_rows=1, eps_f16=0, xm_f16=0, stream=None)
    a.update(kw)
    return [ctypes.c_void_p(v) if k in ("eps", "x", "hist", "coef", "step", "x_out", "x_model", "stream") and v is not None
            else v for k, v in a.items()]


# (arguments on top of a valid base, the code the entry point must return); none of them reaches a HIP call
REFUSALS = [
    (dict(eps=None), -1), (dict(x=None), -1), (dict(hist=None), -1), (dict(coef=None), -1), (dict(x_out=None), -1),
    (dict(n=0), -1), (dict(C=0), -1), (dict(inner=0), -1), (dict(inner=-8), -1), (dict(row=-1), -1), (dict(row=1), -1),
    (dict(n_rows=0), -1),
    (dict(ld_eps=31), -2),                                   # < C * inner
    (dict(ld_eps=34), -2),                                   # inner % 4 == 0: four elements per access
    (dict(eps=GOOD + 8), -2), (dict(eps=GOOD + 4, eps_f16=1), -2), (dict(x=GOOD + 4), -2), (dict(hist=GOOD + 8), -2),
    (dict(x_out=GOOD + 4), -2), (dict(x_model=GOOD + 8), -2), (dict(x_model=GOOD + 4, xm_f16=1), -2),
    (dict(inner=7, ld_eps=28, eps=GOOD + 2), -2),            # one element per access: still its own 4 bytes
    (dict(inner=7, ld_eps=27), -2),
    (dict(step=GOOD + 2), -2), (dict(coef=GOOD + 2), -2),
    (dict(eps_f16=2), -4), (dict(eps_f16=-1), -4), (dict(xm_f16=3), -4),
    # the order: EINVAL before ESHAPE before EUNSUP
    (dict(eps=None, ld_eps=31, eps_f16=2), -1), (dict(row=-1, eps_f16=2), -1), (dict(ld_eps=31, eps_f16=2), -2),
    (dict(x=GOOD + 4, xm_f16=7), -2),
]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    return _lib.load()


def test_step_entry_point_refusal_table_and_order():
    lib = _lib()
    for kw, code in REFUSALS:
        assert lib.vq_cfg_dpmpp_step(*_step_args(**kw)) == code, kw


def test_advance_entry_point_refusals():
    lib = _lib()
    p = ctypes.c_void_p(GOOD)
    assert lib.vq_dpmpp_advance(None, p, 1, p, 1, None) == -1
    assert lib.vq_dpmpp_advance(p, None, 1, p, 1, None) == -1
    assert lib.vq_dpmpp_advance(p, p, 1, None, 1, None) == -1
    assert lib.vq_dpmpp_advance(p, p, 0, p, 1, None) == -1
    assert lib.vq_dpmpp_advance(p, p, 1, p, 0, None) == -1
    assert lib.vq_dpmpp_advance(ctypes.c_void_p(GOOD + 2), p, 1, p, 1, None) == -2
    assert lib.vq_dpmpp_advance(p, p, 1, ctypes.c_void_p(GOOD + 1), 1, None) == -2


def _fakes(kw):
    a = dict(eps=GOOD, x=GOOD, n=1, C=4, inner=8, ld_eps=32, eps_f16=0)
    a.update({k: v for k, v in kw.items() if k in a})
    n, C, inner = a["n"], a["C"], a["inner"]
    dt = {0: torch.float32, 1: torch.float16}.get(a["eps_f16"], torch.bfloat16)
    eps = _FakeTensor((2 * n, C, inner), (a["ld_eps"], inner, 1), a["eps"], dt)
    x = _FakeTensor((n, C, inner), (C * inner, inner, 1), a["x"], torch.float32)
    return eps, x


def test_ok_predicate_agrees_with_the_entry_point():
    """ops.cfg_dpmpp_step_ok says no exactly where the entry point refuses, on every row of the table that is about eps
    and x (what the predicate is given), and yes on the valid layouts."""
    lib = _lib()
    from viditq_amd import ops
    asked = 0
    for kw, code in REFUSALS:
        if not set(kw) <= {"eps", "x", "n", "C", "inner", "ld_eps", "eps_f16"} or kw.get("eps", 1) is None \
                or kw.get("x", 1) is None or min(kw.get("n", 1), kw.get("C", 1), kw.get("inner", 1)) < 0:
            continue
        assert lib.vq_cfg_dpmpp_step(*_step_args(**kw)) == code
        assert ops.cfg_dpmpp_step_ok(*_fakes(kw)) is False, kw
        asked += 1
    assert asked >= 12
    for kw in (dict(), dict(eps_f16=1), dict(ld_eps=64), dict(inner=7, ld_eps=28, eps=GOOD + 4), dict(inner=1, ld_eps=4),
               dict(inner=7, ld_eps=56, eps=GOOD + 2, eps_f16=1), dict(n=3, C=3, inner=12, ld_eps=72, eps=GOOD + 8, eps_f16=1)):
        assert ops.cfg_dpmpp_step_ok(*_fakes(kw)) is True, kw
    eps, x = _fakes({})
    x.dtype = torch.float16
    assert ops.cfg_dpmpp_step_ok(eps, x) is False                      # the latent is fp32
    eps, x = _fakes({})
    eps._st = (32, 1, 4)
    assert ops.cfg_dpmpp_step_ok(eps, x) is False                      # not dense within a batch element
    eps, x = _fakes({})
    eps.is_cuda = False
    assert ops.cfg_dpmpp_step_ok(eps, x) is False


# Every layout the two ``_fakes`` tables (this file: eps [2n, C, inner]; test_ddpm_step_cpu.py: eps [2n, 2C, inner]) hand to
# the predicates: (channel multiplier m of the layout, n, C, inner, ld_eps), then what the two geometry functions that
# _step_geometry replaced returned for it - the DPM-Solver++ one (an element is C * inner) and the IDDPM one (2C * inner).
GEOMETRIES = [
    (1, 0, 4, 8, 32, (0, 4, 8, 32), None), (1, 1, 0, 8, 32, (1, 0, 8, 32), (1, 0, 8, 32)),
    (1, 1, 4, 0, 32, (1, 4, 0, 32), None), (1, 1, 4, 8, 31, (1, 4, 8, 31), None), (1, 1, 4, 8, 34, (1, 4, 8, 34), None),
    (1, 1, 4, 8, 32, (1, 4, 8, 32), None), (1, 1, 4, 7, 28, (1, 4, 7, 28), None), (1, 1, 4, 7, 27, (1, 4, 7, 27), None),
    (1, 1, 4, 8, 64, (1, 4, 8, 64), None), (1, 1, 4, 1, 4, (1, 4, 1, 4), None), (1, 1, 4, 7, 56, (1, 4, 7, 56), None),
    (1, 3, 3, 12, 72, (3, 3, 12, 72), None),
    (2, 0, 4, 8, 64, None, (0, 4, 8, 64)), (2, 1, 0, 8, 64, (1, 0, 8, 64), (1, 0, 8, 64)),
    (2, 1, 4, 0, 64, None, (1, 4, 0, 64)), (2, 1, 4, 8, 63, None, (1, 4, 8, 63)), (2, 1, 4, 8, 32, None, (1, 4, 8, 32)),
    (2, 1, 4, 8, 66, None, (1, 4, 8, 66)), (2, 1, 4, 8, 64, None, (1, 4, 8, 64)), (2, 1, 4, 7, 56, None, (1, 4, 7, 56)),
    (2, 1, 4, 7, 55, None, (1, 4, 7, 55)), (2, 1, 4, 8, 65, None, (1, 4, 8, 65)), (2, 1, 4, 8, 68, None, (1, 4, 8, 68)),
    (2, 1, 4, 8, 72, None, (1, 4, 8, 72)),
    (2, 2, 3, 7, 41, None, (2, 3, 7, 41)), (2, 2, 3, 7, 42, None, (2, 3, 7, 42)), (2, 2, 3, 7, 43, None, (2, 3, 7, 43)),
    (2, 2, 3, 7, 44, None, (2, 3, 7, 44)), (2, 2, 3, 7, 46, None, (2, 3, 7, 46)), (2, 2, 3, 7, 50, None, (2, 3, 7, 50)),
    (2, 3, 4, 12, 95, None, (3, 4, 12, 95)), (2, 3, 4, 12, 96, None, (3, 4, 12, 96)), (2, 3, 4, 12, 97, None, (3, 4, 12, 97)),
    (2, 3, 4, 12, 98, None, (3, 4, 12, 98)), (2, 3, 4, 12, 100, None, (3, 4, 12, 100)),
    (2, 3, 4, 12, 104, None, (3, 4, 12, 104)),
    (2, 1, 1, 1, 1, None, (1, 1, 1, 1)), (2, 1, 1, 1, 2, None, (1, 1, 1, 2)), (2, 1, 1, 1, 3, None, (1, 1, 1, 3)),
    (2, 1, 1, 1, 4, None, (1, 1, 1, 4)), (2, 1, 1, 1, 6, None, (1, 1, 1, 6)), (2, 1, 1, 1, 10, None, (1, 1, 1, 10)),
    (2, 2, 4, 2, 15, None, (2, 4, 2, 15)), (2, 2, 4, 2, 16, None, (2, 4, 2, 16)), (2, 2, 4, 2, 17, None, (2, 4, 2, 17)),
    (2, 2, 4, 2, 18, None, (2, 4, 2, 18)), (2, 2, 4, 2, 20, None, (2, 4, 2, 20)), (2, 2, 4, 2, 24, None, (2, 4, 2, 24)),
]


def test_merged_geometry_returns_what_the_two_geometry_functions_returned():
    """ops._step_geometry(eps, x, 1) and (eps, x, 2) on every layout of GEOMETRIES, and None from both for strides that
    are not dense within a batch element."""
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    assert len(GEOMETRIES) == 48
    for m, n, C, inner, ld, want1, want2 in GEOMETRIES:
        eps = _FakeTensor((2 * n, m * C, inner), (ld, inner, 1), GOOD, torch.float32)
        x = _FakeTensor((n, C, inner), (C * inner, inner, 1), GOOD, torch.float32)
        assert ops._step_geometry(eps, x, 1) == want1, (m, n, C, inner, ld)
        assert ops._step_geometry(eps, x, 2) == want2, (m, n, C, inner, ld)
        eps._st = (ld, 1, m * C)
        if inner > 1 and m * C > 1:
            assert ops._step_geometry(eps, x, 1) is None and ops._step_geometry(eps, x, 2) is None
    eps, x = _fakes({})
    x._st = (64, 8, 1)
    assert ops._step_geometry(eps, x, 1) is None                       # the latent itself is dense


def test_ops_refuse_cpu_tensors():
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L, ops
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)   # noqa: E731
    with pytest.raises(ops.VQError):
        ops.cfg_dpmpp_step(f(2, 4, 8), f(1, 4, 8), f(3, 32), f(1, L.DPMPP_ROW), 0)
    with pytest.raises(ops.VQError):
        ops.dpmpp_advance(torch.zeros(1, dtype=torch.int32), f(1, L.DPMPP_ROW), f(2))
    assert ops.cfg_dpmpp_step_ok(f(2, 4, 8), f(1, 4, 8)) is False
    assert L.DPMPP_ROW == dc.ROW and L.DPMPP_T_NEXT == dc.T_NEXT and L.DPMPP_INV_R01 == dc.INV_R01


# ---------------------------------------------------------------------------------------------------- the switch
def test_switch_is_off_by_default_and_cpu_tensors_stay_eager(monkeypatch):
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    from viditq_amd.t2i import dpm_solver as ds
    assert ds._switch("VQ_DPM_FUSED_NO_SUCH_VARIABLE", False) is False
    assert ds._DPM_FUSED == (os.environ.get("VQ_DPM_FUSED", "0") != "0")
    n_calls = [0]

    def counted(*a, **k):
        n_calls[0] += 1
        raise AssertionError("the fused step was launched")
    monkeypatch.setattr(ops, "cfg_dpmpp_step", counted)
    s = dc.make_solver(4.5, dc.analytic_model(True))
    x = torch.from_numpy(dc.gauss((1, 4, 4, 4), seed=3))
    base = s.sample(x, steps=5, order=2, fused=False)
    assert torch.equal(s.sample(x, steps=5, order=2, fused=True), base)      # CPU tensors: the eager route
    assert torch.equal(s.sample(x, steps=5, order=2), base)
    seen = []
    s.sample(x, steps=5, order=2, fused=True, step_callback=lambda i, v: seen.append((i, v)))
    assert [i for i, _ in seen] == [2, 3, 4, 5] and torch.equal(seen[-1][1], base)
    assert n_calls[0] == 0


def test_step_graph_refuses_a_forward_that_moves_a_running_statistic():
    """A running smooth-quant statistic updates host-visible state in every forward (GraphedModel launches such a model
    eagerly): the captured step refuses it before anything runs."""
    import types
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    from viditq_amd.graph import DPMStepGraph
    from viditq_amd.qdiff.models.quant_layer import QuantLayer
    lay = object.__new__(QuantLayer)
    lay.__dict__.update(weight_quant=True, act_quant=True, weight_quantizer=types.SimpleNamespace(n_bits=8),
                        act_quantizer=types.SimpleNamespace(n_bits=8), smooth_quant=False, smooth_quant_running_stat=True,
                        channel_wise_scale_type="momentum_act_max")

    class Root:
        def modules(self):
            return [lay]

        def forward_with_dpmsolver(self, x, t, y, **kw):
            raise AssertionError("the forward ran")
    with pytest.raises(ops.VQError, match="running"):
        DPMStepGraph(Root().forward_with_dpmsolver, None, {}, torch.zeros(1, 4, 2, 2), torch.zeros(2, dc.ROW), 999.0)

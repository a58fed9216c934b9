"""The SA-Solver port and its fused step without a GPU: the port against vectors recorded from the reference
(tests/golden/t2i_sa_solver.npz, made by tests/golden/make_golden_sa_solver.py) bit for bit, its RNG stream, the coefficient
table driving the CPU model of sa_step_cases.py along the recorded trajectories, the exact cases prove themselves, the entry
point refuses bad arguments in the documented order before any HIP call, and the fused route is off unless asked for."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sa_step_cases as sc
from helpers import _FakeTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "t2i_sa_solver.npz"))


def _run(name, calls=None, noise=True, **kw):
    mode, steps, p, c, pc_mode, skip, eta, half = sc.TRAJECTORIES[name]
    key = "traj.%s." % name
    s = sc.make_solver(sc.GUIDE, sc.analytic_model(half, calls))
    return s.sample(mode, torch.from_numpy(GOLD[key + "z"]), sc.tau_window(eta), steps, skip_type=skip, skip_order=1,
                    predictor_order=p, corrector_order=c, pc_mode=pc_mode, return_intermediate=True,
                    noise_steps=torch.from_numpy(GOLD[key + "noise"]) if noise else None, **kw)


# ---------------------------------------------------------------------------------------------------- the port
@pytest.mark.parametrize("name", list(sc.TRAJECTORIES))
def test_port_reproduces_the_recorded_trajectories(name):
    """Every intermediate, the final sample and the model-input times, bit for bit, fed from the recorded noise."""
    calls = []
    x, mid = _run(name, calls)
    key = "traj.%s." % name
    want = torch.from_numpy(GOLD[key + "mid"])
    assert len(mid) == want.shape[0] and all(m.dtype == torch.float32 for m in mid)
    for i, m in enumerate(mid):
        assert torch.equal(m, want[i]), (name, i, float((m - want[i]).abs().max()))
    assert torch.equal(x, torch.from_numpy(GOLD[key + "final"])) and torch.equal(x, mid[-1])
    assert torch.equal(torch.stack([t[0] for t in calls]), torch.from_numpy(GOLD[key + "times"])), name
    assert all(bool((t == t[0]).all()) and t.numel() == 2 for t in calls)
    mode, steps, p, c, pc_mode = sc.TRAJECTORIES[name][:5]
    nfe = steps + (2 if mode == "more_steps" else 0) + (steps - 1 if pc_mode == "PECE" else 0)
    assert len(calls) == nfe, (name, len(calls))
    assert len(mid) == steps + 1 + (mode == "more_steps")


def test_live_run_against_the_imported_reference():
    """With the reference at hand: a second seed, bit for bit, drawing its own noise on both sides."""
    sys.path.insert(0, ROOT)
    from oracle import ref_import
    if not ref_import.available():
        return                                                        # the recorded vectors above are the check
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_sa_solver as mg
    for name in ("few_p2c2_f16", "few_p3c4", "few_p2c2_pece"):
        mode, steps, p, c, pc_mode, skip, eta, half = sc.TRAJECTORIES[name]
        want_mid, want_x, want_t = mg.reference_trajectory(name, seed=23)
        calls = []
        torch.manual_seed(23)
        x, mid = sc.make_solver(sc.GUIDE, sc.analytic_model(half, calls)).sample(
            mode, sc.start_latent(23), sc.tau_window(eta), steps, skip_type=skip, predictor_order=p, corrector_order=c,
            pc_mode=pc_mode, return_intermediate=True)
        assert torch.equal(torch.stack(mid), want_mid) and torch.equal(x, want_x), name
        assert torch.equal(torch.stack([t[0] for t in calls]), want_t), name


def test_recorded_trajectories_differ_where_the_settings_do():
    base = GOLD["traj.few_p2c2.final"]
    assert np.isfinite(base).all() and np.array_equal(GOLD["traj.few_p2c2.z"], GOLD["traj.few_p3c4.z"])
    for other in list(sc.TRAJECTORIES)[1:]:
        assert not np.array_equal(GOLD["traj.%s.final" % other], base), other
    # tau = 0 outside [0.2, 0.8]: with the 6-step time grid the first corrected sample is the same for eta 1 and 0
    assert np.array_equal(GOLD["traj.few_p2c2.mid"][1], GOLD["traj.few_p2c2_eta0.mid"][1])
    assert not np.array_equal(GOLD["traj.few_p2c2.mid"][3], GOLD["traj.few_p2c2_eta0.mid"][3])


@pytest.mark.parametrize("name", ["few_p2c2", "few_p2c2_pece", "more_p3c4"])
def test_rng_stream_is_the_references(name):
    """After torch.manual_seed the port's own 1 + S draws - one before the first model call, one per step, the last step
    included - reproduce the recorded noise stack: the trajectory is the recorded one without being handed the stack."""
    steps = sc.TRAJECTORIES[name][1]
    assert torch.equal(sc.noise_stack(sc.SEED, steps), torch.from_numpy(GOLD["traj.%s.noise" % name]))
    torch.manual_seed(sc.SEED)
    x, mid = _run(name, noise=False)
    assert torch.equal(torch.stack(mid), torch.from_numpy(GOLD["traj.%s.mid" % name]))
    after = torch.randn(3)                                            # and not one draw more or fewer
    torch.manual_seed(sc.SEED)
    for _ in range(1 + steps):
        torch.randn(*sc.LATENT)
    assert torch.equal(after, torch.randn(3))
    g = torch.Generator().manual_seed(sc.SEED)                        # a generator in place of the global one
    x2, _ = _run(name, noise=False, generator=g)
    assert torch.equal(x2, x)


@pytest.mark.parametrize("li", range(len(sc.TIME_LISTS)))
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_updates_and_coefficients_against_the_reference(li, order):
    s = sc.make_solver()
    prev, t = sc.TIME_LISTS[li]
    x, models, noise = sc.update_inputs(li)
    t_prev, t = [torch.tensor(v) for v in prev[-order:]], torch.tensor(t)
    lam = lambda v: s.ns.marginal_lambda(v.reshape(1))   # noqa: E731
    for ti, tau in enumerate(sc.TAUS):
        for name in sc.UPDATES:
            got = getattr(s, name)(order, x, tau, models[-order:], t_prev, noise, t)
            want = torch.from_numpy(GOLD["upd.%s.L%d.o%d.tau%d" % (name, li, order, ti)])
            assert got.dtype == torch.float32 and torch.equal(got, want), (name, tau, float((got - want).abs().max()))
        gc = s.get_coefficients_fn(order, lam(t_prev[-1]), lam(t), [lam(t_prev[-(i + 1)]) for i in range(order)], tau)
        got = torch.cat([torch.as_tensor(v, dtype=torch.float32).reshape(1) for v in gc])
        assert torch.equal(got, torch.from_numpy(GOLD["upd.get_coefficients_fn.L%d.o%d.tau%d" % (li, order, ti)])), tau
    if order == 2:                                                    # the 'few steps' modification is visible
        assert not np.array_equal(GOLD["upd.adams_bashforth_update.L%d.o2.tau1" % li],
                                  GOLD["upd.adams_bashforth_update_few_steps.L%d.o2.tau1" % li])


@pytest.mark.parametrize("skip", sc.SKIPS)
@pytest.mark.parametrize("N", sc.GRID_N)
def test_time_grids_against_the_reference(skip, N):
    s = sc.make_solver()
    got = s.get_time_steps(skip, 1.0, 1.0 / 1000, N, 1)
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(GOLD["grid.%s.N%d" % (skip, N)]))
    assert s.ns.total_N == 1000                                       # no clipped_lambda cut in this schedule
    with pytest.raises(ValueError):
        s.get_time_steps("time_uniform", 1.0, 1e-3, N)


def test_model_fn_promotes_an_fp16_model_output_to_fp32():
    s = sc.make_solver(sc.GUIDE, sc.analytic_model(True))
    x = sc.start_latent()
    assert s._noise(x, torch.tensor(0.5)).dtype == torch.float16
    assert s.model_fn(x, torch.tensor(0.5)).dtype == torch.float32


# ---------------------------------------------------------------------------------------------------- pec_rows
@pytest.mark.parametrize("name", sc.KERNEL_TRAJECTORIES)
def test_model_through_pec_rows_follows_the_recorded_trajectory(name):
    """The numpy fp32 model of the kernel's arithmetic, driven by the table from the recorded start latent and noise,
    equals the reference's trajectory bit for bit at every step, the model-input times included."""
    steps, eta, half = sc.TRAJECTORIES[name][1], sc.TRAJECTORIES[name][6], sc.TRAJECTORIES[name][7]
    key = "traj.%s." % name
    s = sc.make_solver(sc.GUIDE, sc.analytic_model(half))
    mid, seen = sc.run_table(s, torch.from_numpy(GOLD[key + "z"]), torch.from_numpy(GOLD[key + "noise"]), sc.tau_window(eta),
                             steps, half)
    assert len(mid) == steps + 1
    for i, m in enumerate(mid):
        assert np.array_equal(m, GOLD[key + "mid"][i]), (name, i, float(np.abs(m - GOLD[key + "mid"][i]).max()))
    assert np.array_equal(np.asarray(seen, dtype=np.float32), GOLD[key + "times"])


@pytest.mark.parametrize("steps,p,c", [(6, 2, 2), (5, 2, 2), (2, 2, 2), (6, 1, 1), (6, 2, 1), (6, 1, 2)])
def test_pec_rows_layout(steps, p, c):
    s = sc.make_solver()
    tau = sc.tau_window(1)
    rows = s.pec_rows(tau, steps, predictor_order=p, corrector_order=c)
    assert tuple(rows.shape) == (steps, sc.ROW) and rows.dtype == torch.float32
    r = rows.numpy()
    assert np.isfinite(r).all() and r[:, sc.CFG].tolist() == [sc.GUIDE] * steps
    assert r[0, sc.OC] == 0 and not r[0, sc.CX:sc.CN + 1].any()       # call 0 corrects nothing
    assert r[-1, sc.OP] == 1 and r[-1, sc.PN] == 0 and r[-1, sc.PG1] == 0   # the final step: order 1, tau = 0
    used = [s.orders_used(k, steps, p, c) for k in range(1, steps + 1)]
    assert r[1:, sc.OC].tolist() == [float(u[1]) for u in used[:-1]]
    assert r[:, sc.OP].tolist() == [float(u[0]) for u in used]
    assert set(r[:, sc.OC].tolist()) <= {0.0, 1.0, 2.0} and set(r[:, sc.OP].tolist()) <= {1.0, 2.0}
    assert not r[:, 13].any() and not r[:, 15].any()
    ts = s.get_time_steps("time", 1.0, 1.0 / 1000, steps)
    assert r[:, sc.T_NEXT].tolist() == [s._t_val(ts[k + 1]) for k in range(steps)]
    for k in range(steps):
        assert r[k, sc.SIGMA] == float(s.ns.marginal_std(ts[k].reshape(1)))
        assert r[k, sc.ALPHA] == float(s.ns.marginal_alpha(ts[k].reshape(1)))
        assert (r[k, sc.CG1] != 0) == (r[k, sc.OC] == 2) and (r[k, sc.PG1] != 0) == (r[k, sc.OP] == 2)
        if k > 0:                                                     # tau = 0 outside the window: no noise term
            assert (r[k, sc.CN] != 0) == bool(tau(ts[k]))
        if k + 1 < steps:
            assert (r[k, sc.PN] != 0) == bool(tau(ts[k + 1]))
    if (steps, p, c) == (6, 2, 2):
        assert r[:, sc.T_NEXT][:-1].tolist() == GOLD["traj.few_p2c2.times"][1:].tolist()
        assert r[:, sc.OC].tolist() == [0, 2, 2, 2, 2, 2] and r[:, sc.OP].tolist() == [1, 2, 2, 2, 2, 1]


def test_pec_rows_assert_the_orders_the_kernel_serves():
    s = sc.make_solver()
    for p, c in ((3, 2), (2, 3), (3, 4)):
        with pytest.raises(AssertionError):
            s.pec_rows(sc.tau_window(1), 6, predictor_order=p, corrector_order=c)


# ---------------------------------------------------------------------------------------------------- the CPU model
@pytest.mark.parametrize("case", sc.p1_cases(), ids=lambda c: c.name)
def test_p1_cases_are_exact_in_fp16_and_fp32(case):
    big = sc.p1_prove(case)
    assert 0 < big < 2.0 ** 11


def test_p1_operands_and_rows_show_every_choice():
    shape = (2, 3, 7)
    c = sc.P1Case(shape, "all", 2)
    flat = np.concatenate([c.eps.reshape(-1), c.x.reshape(-1), c.xp.reshape(-1), c.hist.reshape(-1), c.noise.reshape(-1)])
    assert np.array_equal(flat * 16, np.round(flat * 16)) and np.abs(flat).max() <= 8
    assert (c.eps[0] != c.eps[2]).all() and (c.eps[0] != c.eps[1]).all()          # batch halves, batch elements
    assert (c.x != c.xp).all() and (c.hist[0] != c.hist[1]).all() and (c.noise[0] != c.noise[1]).all()
    base = c.expected()
    for kind, k in (("all", 3), ("o11", 2), ("oc0", 2)):                        # ring / history parity, orders
        other = sc.P1Case(shape, kind, k).expected()
        assert not np.array_equal(other[0], base[0]) or not np.array_equal(other[1], base[1]), kind
    # a one-hot row's output is that operand alone: a swapped column, history slot or noise slot is another number
    n = shape[0]
    for k in (2, 3):
        m1, zc, zp = c.hist[(k - 1) % 2].reshape(shape), c.noise[k % 2].reshape(shape), c.noise[(k + 1) % 2].reshape(shape)
        u, cc = c.eps[:n], c.eps[n:]
        m = (c.xp - 0.5 * (u + 2 * (cc - u))) / 0.5
        zero = np.zeros(shape, dtype=np.float32)
        want = {sc.CX: (2 * c.x, zero), sc.CG0: (2 * m, zero), sc.CG1: (2 * m1, zero), sc.CN: (2 * zc, zero),
                sc.PX: (zero, zero), sc.PG0: (zero, 2 * m), sc.PG1: (zero, 2 * m1), sc.PN: (zero, 2 * zp)}
        for kind in sc.COEFS:
            xc, xq, _ = sc.P1Case(shape, kind, k).expected()
            assert np.array_equal(xc, want[kind][0]), (sc.COEF_NAMES[kind], k)
            if kind in (sc.PX, sc.PG0, sc.PG1, sc.PN):
                assert np.array_equal(xq, want[kind][1]), (sc.COEF_NAMES[kind], k)
    kinds = {(c.kind, c.k % 2) for c in sc.p1_cases()}
    assert kinds >= {(kind, par) for kind in sc.P1_KINDS for par in (0, 1)}
    big = [c for c in sc.p1_cases() if c.shape[2] > 8192]
    assert {c.kind for c in big if c.shape[2] == 65536} >= set(sc.COEFS) | {"all"}


# ---------------------------------------------------------------------------------------------------- refusals
GOOD = 1 << 20
PTRS = ("eps", "x", "xp", "hist", "noise", "coef", "step", "x_out", "xp_out", "x_model", "stream")
ORDER = ("eps", "x", "xp", "hist", "noise", "coef", "step", "x_out", "xp_out", "x_model", "n", "C", "inner", "ld_eps", "row",
         "n_rows", "eps_f16", "xm_f16", "stream")


def _step_args(**kw):
    a = dict(eps=GOOD, x=GOOD, xp=GOOD, hist=GOOD, noise=GOOD, coef=GOOD, step=None, x_out=GOOD, xp_out=GOOD, x_model=None,
             n=1, C=4, inner=8, ld_eps=32, row=0, n_rows=1, eps_f16=0, xm_f16=0, stream=None)
    a.update(kw)
    assert tuple(a) == ORDER
    return [ctypes.c_void_p(v) if k in PTRS and v is not None else v for k, v in a.items()]


# (arguments on top of a valid base, the code the entry point must return); none of them reaches a HIP call
REFUSALS = [
    (dict(eps=None), -1), (dict(x=None), -1), (dict(xp=None), -1), (dict(hist=None), -1), (dict(noise=None), -1),
    (dict(coef=None), -1), (dict(x_out=None), -1), (dict(xp_out=None), -1),
    (dict(n=0), -1), (dict(C=0), -1), (dict(inner=0), -1), (dict(inner=-8), -1), (dict(n_rows=0), -1),
    (dict(row=-1), -1), (dict(row=1), -1),
    (dict(ld_eps=31), -2),                                   # < C * inner
    (dict(ld_eps=34), -2),                                   # inner % 4 == 0: four elements per access
    (dict(eps=GOOD + 8), -2), (dict(eps=GOOD + 4, eps_f16=1), -2), (dict(x=GOOD + 4), -2), (dict(xp=GOOD + 8), -2),
    (dict(hist=GOOD + 4), -2), (dict(noise=GOOD + 8), -2), (dict(x_out=GOOD + 4), -2), (dict(xp_out=GOOD + 8), -2),
    (dict(x_model=GOOD + 8), -2), (dict(x_model=GOOD + 4, xm_f16=1), -2),
    (dict(inner=7, ld_eps=28, eps=GOOD + 2), -2),            # one element per access: still its own 4 bytes
    (dict(inner=7, ld_eps=27), -2),
    (dict(step=GOOD + 2), -2), (dict(coef=GOOD + 2), -2),
    (dict(eps_f16=2), -4), (dict(eps_f16=-1), -4), (dict(xm_f16=3), -4),
    # the order: EINVAL before ESHAPE before EUNSUP
    (dict(eps=None, ld_eps=31, eps_f16=2), -1), (dict(row=-1, eps_f16=2), -1), (dict(xp=None, ld_eps=31), -1),
    (dict(ld_eps=31, eps_f16=2), -2), (dict(noise=GOOD + 4, xm_f16=2), -2), (dict(x=GOOD + 4, xm_f16=7), -2),
]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    return _lib.load()


def test_entry_point_refusal_table_and_order():
    lib = _lib()
    for kw, code in REFUSALS:                                         # (the valid base itself would launch: never called)
        assert lib.vq_cfg_sa_step(*_step_args(**kw)) == code, kw
    assert lib.vq_cfg_sa_step(*[None if k in PTRS else 1 for k in ORDER]) == -1


def _fakes(kw):
    a = dict(eps=GOOD, x=GOOD, n=1, C=4, inner=8, ld_eps=32, eps_f16=0)
    a.update({k: v for k, v in kw.items() if k in a})
    n, C, inner = a["n"], a["C"], a["inner"]
    dt = {0: torch.float32, 1: torch.float16}.get(a["eps_f16"], torch.bfloat16)
    eps = _FakeTensor((2 * n, C, inner), (a["ld_eps"], inner, 1), a["eps"], dt)
    x = _FakeTensor((n, C, inner), (C * inner, inner, 1), a["x"], torch.float32)
    return eps, x


def _refusal_only(lib, kw):
    """The entry point's refusal code for ``kw``, or None where it would launch - asked WITHOUT launching: the one further
    argument that is checked last (a dtype flag) is made invalid, so -4 means "everything before passed"."""
    code = lib.vq_cfg_sa_step(*_step_args(**dict(kw, xm_f16=9)))
    return None if code == -4 else code


def test_ok_predicate_agrees_with_the_entry_point():
    lib = _lib()
    from viditq_amd import ops
    asked = 0
    for kw, code in REFUSALS:
        if not set(kw) <= {"eps", "x", "n", "C", "inner", "ld_eps", "eps_f16"} or kw.get("eps", 1) is None \
                or kw.get("x", 1) is None or min(kw.get("n", 1), kw.get("C", 1), kw.get("inner", 1)) < 0:
            continue
        assert ops.cfg_sa_step_ok(*_fakes(kw)) is False, kw
        asked += 1
    assert asked >= 10
    grid = 0
    for n, C, inner in ((1, 4, 8), (2, 3, 7), (3, 4, 12), (1, 1, 1), (2, 4, 2)):
        for pad in (-1, 0, 1, 2, 4, 8):
            for off in (0, 2, 4, 8, 16):
                for f16 in (0, 1):
                    kw = dict(n=n, C=C, inner=inner, ld_eps=C * inner + pad, eps=GOOD + off, eps_f16=f16)
                    assert ops.cfg_sa_step_ok(*_fakes(kw)) is (_refusal_only(lib, kw) is None), kw
                    kw = dict(kw, eps=GOOD, x=GOOD + off)
                    assert ops.cfg_sa_step_ok(*_fakes(kw)) is (_refusal_only(lib, kw) is None), kw
                    grid += 2
    assert grid == 600
    eps, x = _fakes({})
    x.dtype = torch.float16
    assert ops.cfg_sa_step_ok(eps, x) is False                         # the latent is fp32
    eps, x = _fakes({})
    eps.shape = (2, 8, 8)
    assert ops.cfg_sa_step_ok(eps, x) is False                         # not [2n, C, ...]
    eps, x = _fakes({})
    eps.is_cuda = False
    assert ops.cfg_sa_step_ok(eps, x) is False


def test_ops_refuse_cpu_tensors_and_constants_agree():
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L, ops
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)   # noqa: E731
    with pytest.raises(ops.VQError):
        ops.cfg_sa_step(f(2, 4, 8), f(1, 4, 8), f(1, 4, 8), f(2, 32), f(2, 32), f(1, L.SA_ROW), 0)
    assert ops.cfg_sa_step_ok(f(2, 4, 8), f(1, 4, 8)) is False
    assert L.SA_ROW == sc.ROW == L.DPMPP_ROW and L.SA_T_NEXT == sc.T_NEXT == L.DPMPP_T_NEXT
    names = ("CFG", "SIGMA", "ALPHA", "OC", "CX", "CG0", "CG1", "CN", "OP", "PX", "PG0", "PG1", "PN")
    assert tuple(getattr(L, "SA_" + v) for v in names) == tuple(getattr(sc, v) for v in names) == tuple(range(13))
    hdr = open(os.path.join(ROOT, "include", "viditq.h")).read()
    for name in names + ("T_NEXT", "ROW"):
        assert "#define VQ_SA_%s %d " % (name, getattr(L, "SA_" + name)) in hdr, name


# ---------------------------------------------------------------------------------------------------- settings
def test_unsupported_settings_say_so():
    import viditq_amd  # noqa: F401
    from viditq_amd.t2i import SASolver, SASolverSampler
    y = torch.zeros(1, 1, 2, 4)
    for kw in (dict(algorithm_type="noise_prediction"), dict(correcting_x0_fn="dynamic_thresholding"),
               dict(correcting_xt_fn=lambda x, t, step: x)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            SASolver(None, y, y, 4.5, **kw)
    with pytest.raises(NotImplementedError, match="noise_schedule"):
        SASolverSampler(None, noise_schedule="squaredcos_cap_v2")
    s = sc.make_solver(sc.GUIDE, sc.analytic_model(False))
    with pytest.raises(AssertionError):
        s.sample("some_steps", sc.start_latent(), sc.tau_window(1), 6)
    with pytest.raises(AssertionError):
        s.sample("few_steps", sc.start_latent(), sc.tau_window(1), 6, pc_mode="PCE")
    with pytest.raises(AssertionError):
        s.sample("few_steps", sc.start_latent(), sc.tau_window(1), 2, predictor_order=3, corrector_order=4)


def test_sampler_is_the_released_configuration():
    """SASolverSampler.sample: 'few_steps', 'time', P2 / C2, PEC and the tau window - the recorded trajectory."""
    import viditq_amd  # noqa: F401
    from viditq_amd.t2i import SASolverSampler
    y = torch.zeros(1, 1, 2, 4)
    for name in ("few_p2c2", "few_p2c2_f16", "few_p2c2_eta0"):
        eta, half = sc.TRAJECTORIES[name][6], sc.TRAJECTORIES[name][7]
        key = "traj.%s." % name
        smp = SASolverSampler(sc.analytic_model(half), device="cpu")
        x, none = smp.sample(6, 1, sc.LATENT[1:], conditioning=y, unconditional_conditioning=y.clone(),
                             unconditional_guidance_scale=sc.GUIDE, eta=eta, x_T=torch.from_numpy(GOLD[key + "z"]),
                             noise_steps=torch.from_numpy(GOLD[key + "noise"]))
        assert none is None and torch.equal(x, torch.from_numpy(GOLD[key + "final"])), name


# ---------------------------------------------------------------------------------------------------- the switch
def test_cpu_latents_stay_eager(monkeypatch):
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    from viditq_amd.t2i import sa_solver
    assert sa_solver._SA_FUSED == (os.environ.get("VQ_SA_FUSED", "0") != "0")

    def counted(*a, **k):
        raise AssertionError("the fused step was launched")
    monkeypatch.setattr(ops, "cfg_sa_step", counted)
    x, mid = _run("few_p2c2", fused=True)
    assert torch.equal(x, torch.from_numpy(GOLD["traj.few_p2c2.final"]))


CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
import viditq_amd
from viditq_amd.t2i import sa_solver
print("SWITCH", int(sa_solver._SA_FUSED))
"""


@pytest.mark.parametrize("value,want", [("1", "1"), ("0", "0"), (None, "0")])
def test_switch_is_read_in_a_child_process(value, want):
    env = {k: v for k, v in os.environ.items() if k != "VQ_SA_FUSED"}
    if value is not None:
        env["VQ_SA_FUSED"] = value
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("SWITCH")][-1].split() == ["SWITCH", want]

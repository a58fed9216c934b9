"""The fused SA-Solver step on the GPU (vq_cfg_sa_step, ops.cfg_sa_step, SASolver.sample(fused=True), graph.SAStepGraph):
exact cases against the CPU model per element, general cases against the CPU model and the port's eager torch expressions
on the same device bit for bit, guards around every buffer and NaN in everything a row does not read, whole trajectories,
the fallbacks, the counter form."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sa_step_cases as sc
from helpers import Arena

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def launch(ops, dev, row, k, eps, x, xp, hist, noise, half, pitch2=False, alias=False, xm=None, poison=True):
    """One launch of ``row`` as row k of a table (history and ring slots follow the row index) with every buffer in a NaN
    arena.  eps [2n, C, inner] / x / xp / hist / noise numpy.  With ``poison`` whatever the row does not read is NaN:
    m_{k-1} unless an order is 2, noise[k % 2] when OC == 0, noise[(k + 1) % 2] when OP == 0, eps beyond C * inner of a
    padded pitch.  Returns (x_out, xp_out, hist, x_model) on the CPU after the guards passed."""
    n, C, inner = x.shape
    CI, tot = C * inner, x.size
    et = torch.float16 if half else torch.float32
    ld = 2 * CI if pitch2 else CI
    A_eps, A_x, A_p = Arena(dev, 2 * n * ld, et), Arena(dev, tot, torch.float32), Arena(dev, tot, torch.float32)
    A_h, A_z = Arena(dev, 2 * tot, torch.float32), Arena(dev, 2 * tot, torch.float32)
    A_o = A_x if alias else Arena(dev, tot, torch.float32)
    A_q = A_p if alias else Arena(dev, tot, torch.float32)
    A_m = Arena(dev, 2 * tot, xm) if xm is not None else None
    ev = A_eps.t.view(2 * n, ld)                        # with pitch2 the elements [CI, 2 CI) of every batch row stay NaN
    ev[:, :CI] = torch.from_numpy(eps.reshape(2 * n, CI)).to(dev).to(et)
    A_x.t.copy_(torch.from_numpy(x.reshape(-1)))
    A_p.t.copy_(torch.from_numpy(xp.reshape(-1)))
    hist, noise = np.array(hist, dtype=np.float32).reshape(2, tot), np.array(noise, dtype=np.float32).reshape(2, tot)
    oc, op = int(row[sc.OC]), int(row[sc.OP])
    if poison:
        if oc != 2 and op != 2:
            hist[(k - 1) % 2] = NAN
        if oc == 0:
            noise[k % 2] = NAN
        if op == 0:
            noise[(k + 1) % 2] = NAN
    A_h.t.copy_(torch.from_numpy(hist.reshape(-1)))
    A_z.t.copy_(torch.from_numpy(noise.reshape(-1)))
    rows = np.zeros((k + 1, sc.ROW), dtype=np.float32)
    rows[k] = row
    coef = torch.from_numpy(rows).to(dev)
    eps_t = ev.view(2 * n, 2 * C if pitch2 else C, inner)[:, :C]
    x_t = A_x.t.view(n, C, inner)
    arenas = [A_eps, A_x, A_p, A_h, A_z, A_o, A_q] + ([A_m] if A_m else [])
    for a in arenas:
        a.snapshot()
    assert ops.cfg_sa_step_ok(eps_t, x_t)
    got = ops.cfg_sa_step(eps_t, x_t, A_p.t.view(n, C, inner), A_h.t.view(2, tot), A_z.t.view(2, tot), coef, k,
                          x_out=A_o.t.view(n, C, inner), xp_out=A_q.t.view(n, C, inner),
                          x_model=A_m.t.view(2 * n, C, inner) if A_m else None)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == A_o.t.data_ptr() and got[1].data_ptr() == A_q.t.data_ptr()
    kk = k % 2
    assert A_eps.unchanged() and A_z.unchanged(), "eps or the noise ring written"
    assert A_h.unchanged(kk * tot, (kk + 1) * tot), "a history slot other than k % 2, or its surroundings, written"
    assert A_o.unchanged(0, tot) and A_q.unchanged(0, tot), "written outside x_out / xp_out"
    if not alias:
        assert A_x.unchanged() and A_p.unchanged(), "x or xp written"
    if A_m:
        assert A_m.unchanged(0, 2 * tot), "written outside x_model"
    return (A_o.t.cpu().numpy().reshape(x.shape), A_q.t.cpu().numpy().reshape(x.shape), A_h.t.cpu().numpy().reshape(2, tot),
            A_m.t.cpu().float().numpy().reshape(2, *x.shape) if A_m else None)


def _same(got, want):
    """Equal values everywhere (as torch.equal compares: the sign of a zero, which a 0 * x term decides, is not a value)."""
    return np.array_equal(got, want)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "n%d_C%d_i%d" % s)
def test_exact_cases_per_element(ops, dev, shape):
    """P1 on every shape: bit-exact against the CPU model for fp16 and fp32 eps, every one-hot row, both ring parities,
    dense and padded pitch, outputs aliasing their inputs, x_model in fp16 / fp32 - inside NaN arenas, with NaN in
    whatever the row does not read."""
    for ci, case in enumerate(sc.p1_cases([shape])):
        half = bool(ci & 1) ^ bool(ci & 4)
        if shape[2] <= 1024:
            halves = (True, False)
        else:
            halves = (half,)
        for half in halves:
            v = ci * 2 + int(half)
            pitch2, alias, xm = bool(v & 1) ^ bool(ci & 2), bool(v & 2), (None, torch.float16, torch.float32)[v % 3]
            want_c, want_q, want_h = case.expected(half)
            got_c, got_q, got_h, got_m = launch(ops, dev, case.row, case.k, case.eps, case.x, case.xp, case.hist,
                                                case.noise, half, pitch2, alias, xm)
            tag = (case.name, half, pitch2, alias, xm)
            assert np.isfinite(got_c).all() and np.isfinite(got_q).all(), tag
            assert _same(got_c, want_c), (tag, "x_out", int((got_c != want_c).sum()), np.argwhere(got_c != want_c)[:3].tolist())
            assert _same(got_q, want_q), (tag, "xp_out", int((got_q != want_q).sum()), np.argwhere(got_q != want_q)[:3].tolist())
            assert _same(got_h[case.k % 2], want_h[case.k % 2]), tag
            if xm is not None:
                cast = torch.from_numpy(want_q).to(xm).float().numpy()
                assert np.array_equal(got_m[0], cast) and np.array_equal(got_m[1], cast), tag


@pytest.fixture(scope="module")
def p2_data():
    return sc.p2_inputs()


@pytest.mark.parametrize("half", [True, False], ids=["fp16eps", "fp32eps"])
@pytest.mark.parametrize("eta", [1, 0])
def test_general_cases_against_the_cpu_model(ops, dev, p2_data, half, eta):
    """P2: every row of a real 6-step table on Gaussian operands, bit-identical to the numpy fp32 model; fp32 and fp16
    x_model, aliased and separate outputs."""
    eps, x, xp, hist, noise = p2_data
    x3, xp3 = x.reshape(sc.P2_SHAPE), xp.reshape(sc.P2_SHAPE)
    for name, k, row in sc.p2_rows(6, eta):
        alias, xm = bool(k & 1), (torch.float16, torch.float32)[(k >> 1) & 1]
        want_c, want_q, want_h = sc.reference_step(row, eps, x3, xp3, hist, noise, k, half)
        got_c, got_q, got_h, got_m = launch(ops, dev, row, k, eps, x3, xp3, hist, noise, half, pitch2=bool(k % 3 == 0),
                                            alias=alias, xm=xm)
        assert np.isfinite(got_q).all(), name
        assert _same(got_c, want_c), (name, "x_out", int((got_c != want_c).sum()))
        assert _same(got_q, want_q), (name, "xp_out", int((got_q != want_q).sum()))
        assert _same(got_h[k % 2], want_h[k % 2]), name
        cast = torch.from_numpy(want_q).to(xm).float().numpy()
        assert np.array_equal(got_m[0], cast) and np.array_equal(got_m[1], cast), name


@pytest.mark.parametrize("half", [True, False], ids=["fp16eps", "fp32eps"])
def test_eager_parity_on_the_device(ops, dev, p2_data, half):
    """One launch against the port's own eager expressions (_guide, _x0_of_noise, the two 'few steps' updates) run on the
    GPU on the same tensors: torch.equal for the x0, the corrected and the predicted sample, on every row of the table."""
    steps, tau = 6, sc.tau_window(1)
    s = sc.make_solver()
    eps, x, xp, hist, noise = p2_data
    eps_g = torch.from_numpy(eps.astype(np.float16 if half else np.float32)).to(dev)
    x_g, xp_g = torch.from_numpy(x).to(dev), torch.from_numpy(xp).to(dev)
    h_g, z_g = torch.from_numpy(hist).to(dev), torch.from_numpy(noise).to(dev)
    coef = s.pec_rows(tau, steps).to(dev)
    ts = s.get_time_steps("time", 1.0, 1.0 / 1000, steps)
    for k in range(steps):
        m_prev = h_g[(k - 1) % 2].view(sc.P2_SHAPE)
        m_k = s._x0_of_noise(xp_g, ts[k], s._guide(eps_g))
        assert m_k.dtype == torch.float32
        xc = x_g
        if k > 0:
            oc = s.orders_used(k, steps, 2, 2)[1]
            xc = s.adams_moulton_update_few_steps(oc, x_g, tau(ts[k]), [m_prev, m_k], [ts[k - 1]],
                                                  z_g[k % 2].view(sc.P2_SHAPE), ts[k])
        op = s.orders_used(k + 1, steps, 2, 2)[0]
        xq = s.adams_bashforth_update_few_steps(op, xc, 0 if k + 1 == steps else tau(ts[k + 1]), [m_prev, m_k],
                                                [ts[max(k - 1, 0)], ts[k]][-op:] if k else [ts[0]],
                                                z_g[(k + 1) % 2].view(sc.P2_SHAPE), ts[k + 1])
        h2 = h_g.clone()
        got_c, got_q = ops.cfg_sa_step(eps_g, x_g, xp_g, h2, z_g, coef, k)
        assert torch.equal(h2[k % 2].view(sc.P2_SHAPE), m_k), (k, "x0", int((h2[k % 2].view(sc.P2_SHAPE) != m_k).sum()))
        assert torch.equal(got_c, xc), (k, "corrected", int((got_c != xc).sum()), float((got_c - xc).abs().max()))
        assert torch.equal(got_q, xq), (k, "predicted", int((got_q != xq).sum()), float((got_q - xq).abs().max()))
        assert torch.equal(h2[(k + 1) % 2], h_g[(k + 1) % 2])


def test_learned_sigma_channels_are_never_read(ops, dev):
    """eps as the chunk(2, dim=1)[0] view of a [2n, 2C, H, W] output whose other half is NaN: finite output."""
    n, C, H, W = 2, 4, 6, 10
    full = torch.full((2 * n, 2 * C, H, W), NAN, dtype=torch.float16, device=dev)
    e = torch.from_numpy(sc.gauss((2 * n, C, H, W), 5)).half().to(dev)
    full[:, :C] = e
    view = full.chunk(2, dim=1)[0]
    x = torch.from_numpy(sc.gauss((n, C, H, W), 6)).to(dev)
    assert not view.is_contiguous() and ops.cfg_sa_step_ok(view, x)
    rows = sc.make_solver().pec_rows(sc.tau_window(1), 5).to(dev)
    hist, ring = torch.zeros(2, x.numel(), device=dev), torch.randn(2, x.numel(), device=dev)
    xm = torch.empty(2 * n, C, H, W, dtype=torch.float16, device=dev)
    a = ops.cfg_sa_step(view, x, x, hist, ring, rows, 2, x_model=xm)
    b = ops.cfg_sa_step(e, x, x, hist.clone(), ring, rows, 2)
    assert torch.isfinite(a[1]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(xm[:n], a[1].half()) and torch.equal(xm[n:], a[1].half())


# ---------------------------------------------------------------------------------------------------- trajectories
def _calls():
    from viditq_amd import _lib
    return _lib.CALLS[0]


@pytest.mark.parametrize("half", [True, False], ids=["fp16model", "fp32model"])
def test_analytic_trajectories_fused_equals_eager(ops, dev, half):
    """Fused == eager at every step from the same seed, the model-input times included, for the released configuration
    and the lower orders the kernel serves; one C-ABI launch per model call."""
    x = torch.from_numpy(sc.gauss((2, 4, 8, 8), 21)).to(dev)
    for steps, p, c, eta in ((25, 2, 2, 1), (6, 2, 2, 1), (6, 2, 2, 0), (5, 1, 1, 1), (5, 2, 1, 0.5), (5, 1, 2, 1), (2, 2, 2, 1)):
        calls_e, calls_f = [], []
        kw = dict(steps=steps, predictor_order=p, corrector_order=c, pc_mode="PEC", return_intermediate=True)
        torch.manual_seed(77)
        want, mid_e = sc.make_solver(4.5, sc.analytic_model(half, calls_e)).sample("few_steps", x, sc.tau_window(eta),
                                                                                   fused=False, **kw)
        n0 = _calls()
        torch.manual_seed(77)
        got, mid_f = sc.make_solver(4.5, sc.analytic_model(half, calls_f)).sample("few_steps", x, sc.tau_window(eta),
                                                                                  fused=True, **kw)
        assert _calls() - n0 == steps                                    # one C-ABI launch per model call
        assert torch.equal(got, want), (steps, p, c, eta, float((got - want).abs().max()))
        assert len(mid_f) == len(mid_e) == steps + 1
        for i, (a, b) in enumerate(zip(mid_f, mid_e)):
            assert torch.equal(a, b), (steps, p, c, eta, i)
        assert len(calls_f) == steps and all(torch.equal(a, b) for a, b in zip(calls_e, calls_f))
        assert torch.equal(torch.randn(4, device=dev), _after(77, steps, x))    # the same 1 + S draws
    # without intermediates (outputs aliased), from a generator, and - where the model casts its input to fp16 itself -
    # with the kernel making that cast (an fp16 x_model)
    s16 = sc.make_solver(4.5, sc.analytic_model(half))
    s16.model_input_dtype = torch.float16 if half else torch.float32
    a = s16.sample("few_steps", x, sc.tau_window(1), 6, predictor_order=2, corrector_order=2, fused=True,
                   generator=torch.Generator(device=dev).manual_seed(5))
    b = sc.make_solver(4.5, sc.analytic_model(half)).sample("few_steps", x, sc.tau_window(1), 6, predictor_order=2,
                                                            corrector_order=2, fused=False,
                                                            generator=torch.Generator(device=dev).manual_seed(5))
    assert torch.equal(a, b)


def _after(seed, steps, x):
    torch.manual_seed(seed)
    for _ in range(1 + steps):
        torch.randn_like(x)
    return torch.randn(4, device=x.device)


def test_fallbacks_launch_no_fused_step(ops, dev, monkeypatch):
    """PECE, an order above 2, corrector order 0, 'more_steps', cfg_scale == 1, CPU tensors: eager, also with fused=True;
    a model output the kernel does not take is handed back and the eager route continues from that first call."""
    n_calls = [0]
    orig = ops.cfg_sa_step

    def counted(*a, **k):
        n_calls[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(ops, "cfg_sa_step", counted)
    x = torch.from_numpy(sc.gauss((1, 4, 4, 4), 2)).to(dev)
    tau = sc.tau_window(1)
    noise = torch.from_numpy(sc.gauss((7, 1, 4, 4, 4), 3)).to(dev)
    s = sc.make_solver(4.5, sc.analytic_model(True))
    for mode, kw in (("few_steps", dict(pc_mode="PECE", predictor_order=2, corrector_order=2)),
                     ("few_steps", dict(predictor_order=3, corrector_order=2)),
                     ("few_steps", dict(predictor_order=2, corrector_order=3)),
                     ("few_steps", dict(predictor_order=2, corrector_order=0)),
                     ("more_steps", dict(predictor_order=2, corrector_order=2))):
        a = s.sample(mode, x, tau, 6, fused=True, noise_steps=noise, **kw)
        assert n_calls[0] == 0, kw
        assert torch.equal(a, s.sample(mode, x, tau, 6, fused=False, noise_steps=noise, **kw))
    plain = lambda x_, t, y, **kw: x_.half() * 0.1   # noqa: E731
    sc.make_solver(1.0, plain).sample("few_steps", x, tau, 6, predictor_order=2, corrector_order=2, fused=True)
    s.sample("few_steps", x.cpu(), tau, 6, predictor_order=2, corrector_order=2, fused=True, noise_steps=noise.cpu())
    s.sample("few_steps", x, tau, 6, predictor_order=2, corrector_order=2, fused=False)
    assert n_calls[0] == 0
    s.sample("few_steps", x, tau, 6, predictor_order=2, corrector_order=2, fused=True)
    assert n_calls[0] == 6
    calls = []
    bf = lambda x_, t, y, **kw: (calls.append(1), sc.analytic_model(False)(x_, t, y).bfloat16())[1]   # noqa: E731
    kw = dict(predictor_order=2, corrector_order=2, noise_steps=noise)
    a = sc.make_solver(4.5, bf).sample("few_steps", x, tau, 6, fused=True, **kw)
    assert n_calls[0] == 6 and len(calls) == 6
    assert torch.equal(a, sc.make_solver(4.5, bf).sample("few_steps", x, tau, 6, fused=False, **kw))
    # ... and with the loop's own draws the hand-back keeps the RNG stream
    torch.manual_seed(9)
    a = sc.make_solver(4.5, bf).sample("few_steps", x, tau, 6, fused=True, predictor_order=2, corrector_order=2)
    torch.manual_seed(9)
    assert torch.equal(a, sc.make_solver(4.5, bf).sample("few_steps", x, tau, 6, fused=False, predictor_order=2,
                                                         corrector_order=2))


def test_tiny_pixart_through_the_sampler_fused_equals_eager(ops, dev):
    """SASolverSampler on the tiny PixArt of tiny_pixart_w8a8.npz (8 steps, cfg 4.5, eta 1): fused == eager bit for bit from
    the same seed, with an fp16 x_model, and step by step through the solver it builds."""
    from test_dpm_step_gpu import _tiny_pixart
    from viditq_amd.t2i import SASolverSampler
    g, qnn = _tiny_pixart(dev)
    z = g["dpm_z"].to(dev)
    kw = dict(S=8, batch_size=z.shape[0], shape=tuple(z.shape[1:]), conditioning=g["y"][:1].half().to(dev),
              unconditional_conditioning=g["dpm_null_y"].half().to(dev), unconditional_guidance_scale=4.5, eta=1, x_T=z,
              model_kwargs=dict(data_info=None, mask=g["mask"][:1].to(dev)))
    smp = SASolverSampler(qnn.forward_with_dpmsolver, device=dev)
    torch.manual_seed(3)
    eager, none = smp.sample(fused=False, **kw)
    assert none is None and torch.isfinite(eager).all() and eager.shape == z.shape
    torch.manual_seed(3)
    fused, _ = smp.sample(fused=True, **kw)
    assert torch.equal(fused, eager), float((fused - eager).abs().max())
    smp.model_input_dtype = torch.float16                 # the kernel makes the model's cast
    torch.manual_seed(3)
    assert torch.equal(smp.sample(fused=True, **kw)[0], eager)
    solver = smp.solver(kw["conditioning"], kw["unconditional_conditioning"], 4.5, kw["model_kwargs"])
    tau = lambda t: 1 if 0.2 <= t <= 0.8 else 0   # noqa: E731
    run = dict(steps=8, predictor_order=2, corrector_order=2, return_intermediate=True)
    torch.manual_seed(3)
    x_e, mid_e = solver.sample("few_steps", z, tau, fused=False, **run)
    torch.manual_seed(3)
    x_f, mid_f = solver.sample("few_steps", z, tau, fused=True, **run)
    assert torch.equal(x_e, eager) and all(torch.equal(a, b) for a, b in zip(mid_f, mid_e)) and len(mid_f) == 9
    sg = solver.step_graph(z, tau, 8)
    torch.manual_seed(3)
    assert torch.equal(sg.run(z), eager)
    torch.manual_seed(3)
    assert torch.equal(sg.run(z), eager)                  # and again: run() resets latents, time and counter


# ---------------------------------------------------------------------------------------------------- counter form
def test_counter_form_replays_one_captured_step(ops, dev):
    """{analytic model, step(step=counter), advance} in one captured graph, replayed ``steps`` times == the eager-launched
    fused loop == the eager route, from a noise stack and from the loop's own draws."""
    x = torch.from_numpy(sc.gauss((2, 4, 8, 8), 31)).to(dev)
    for half, steps, p, c, eta in ((True, 25, 2, 2, 1), (False, 6, 2, 2, 1), (True, 5, 1, 1, 0.5)):
        tau = sc.tau_window(eta)
        noise = torch.from_numpy(sc.gauss((1 + steps, 2, 4, 8, 8), 32)).to(dev)
        s = sc.make_solver(4.5, sc.analytic_model(half))
        kw = dict(predictor_order=p, corrector_order=c)
        want = s.sample("few_steps", x, tau, steps, fused=True, noise_steps=noise, **kw)
        assert torch.equal(want, s.sample("few_steps", x, tau, steps, fused=False, noise_steps=noise, **kw))
        sg = s.step_graph(x, tau, steps, **kw)
        got = sg.run(x, noise_steps=noise)
        assert torch.equal(got, want), (half, steps, p, c)
        ts = s.get_time_steps("time", 1.0, 1.0 / 1000, steps)
        assert int(sg.step) == steps - 1 and bool((sg.t.cpu() == (ts[steps].float() - 1.0 / 1000) * 1000.0).all())
        torch.manual_seed(4)
        a = sg.run(x)
        torch.manual_seed(4)
        assert torch.equal(a, s.sample("few_steps", x, tau, steps, fused=False, **kw))
        gen = lambda: torch.Generator(device=dev).manual_seed(6)   # noqa: E731
        assert torch.equal(sg.run(x, generator=gen()), s.sample("few_steps", x, tau, steps, fused=True, generator=gen(), **kw))


# ---------------------------------------------------------------------------------------------------- the switch
CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import sa_step_cases as sc
import viditq_amd
from viditq_amd import ops
from viditq_amd.t2i import sa_solver
n = [0]
orig = ops.cfg_sa_step
def counted(*a, **k):
    n[0] += 1
    return orig(*a, **k)
ops.cfg_sa_step = counted
x = torch.from_numpy(sc.gauss((1, 4, 4, 4), 3)).cuda()
kw = dict(predictor_order=2, corrector_order=2)
torch.manual_seed(1)
a = sc.make_solver(4.5, sc.analytic_model(True)).sample("few_steps", x, sc.tau_window(1), 5, **kw)
c1 = n[0]
torch.manual_seed(1)
b = sc.make_solver(4.5, sc.analytic_model(True)).sample("few_steps", x, sc.tau_window(1), 5, fused=False, **kw)
print("SWITCH", int(sa_solver._SA_FUSED), c1, n[0], int(torch.equal(a, b)))
"""


def test_switch_in_a_child_process(dev):
    """VQ_SA_FUSED=1 at import: sample() takes the fused route (5 launches for 5 steps), fused=False still overrides."""
    env = dict(os.environ, VQ_SA_FUSED="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SWITCH")][-1]
    assert line.split() == ["SWITCH", "1", "5", "5", "1"], line

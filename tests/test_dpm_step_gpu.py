"""The fused DPM-Solver++ step on the GPU (vq_cfg_dpmpp_step / vq_dpmpp_advance, ops.cfg_dpmpp_step, DPMSolverPP.sample(
fused=True), graph.DPMStepGraph): exact cases against the CPU model per element, general cases against the eager torch
expressions on the same device bit for bit, guards around every buffer, whole trajectories, the counter form."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dpm_step_cases as dc
from helpers import Arena, load_npz, quant_params_of, rel_l2, state_dict_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch(ops, dev, row, k, eps, x, hist, half, pitch2=False, alias=False, xm=None):
    """One launch of ``row`` as row k of a table (the history slot follows the row index) with every buffer in an arena.
    eps [2n, C, inner] / x / hist numpy.  Returns (x_out, hist, x_model) on the CPU after the guards passed."""
    n, C, inner = x.shape
    CI, tot = C * inner, x.size
    et = torch.float16 if half else torch.float32
    ld = 2 * CI if pitch2 else CI
    A_eps, A_x, A_h = Arena(dev, 2 * n * ld, et), Arena(dev, tot, torch.float32), Arena(dev, 3 * tot, torch.float32)
    A_o = A_x if alias else Arena(dev, tot, torch.float32)
    A_m = Arena(dev, 2 * tot, xm) if xm is not None else None
    ev = A_eps.t.view(2 * n, ld)                        # with pitch2 the learned-sigma channels [CI, 2 CI) stay NaN
    ev[:, :CI] = torch.from_numpy(eps.reshape(2 * n, CI)).to(dev).to(et)
    A_x.t.copy_(torch.from_numpy(x.reshape(-1)))
    A_h.t.copy_(torch.from_numpy(hist.reshape(-1)))
    rows = np.zeros((k + 1, dc.ROW), dtype=np.float32)
    rows[k] = row
    coef = torch.from_numpy(rows).to(dev)
    eps_t = ev.view(2 * n, 2 * C if pitch2 else C, inner)[:, :C]
    x_t = A_x.t.view(n, C, inner)
    for a in (A_eps, A_x, A_h, A_o) + ((A_m,) if A_m else ()):
        a.snapshot()
    assert ops.cfg_dpmpp_step_ok(eps_t, x_t)
    got = ops.cfg_dpmpp_step(eps_t, x_t, A_h.t.view(3, tot), coef, k,
                             x_out=A_o.t.view(n, C, inner), x_model=A_m.t.view(2 * n, C, inner) if A_m else None)
    torch.cuda.synchronize()
    assert got.data_ptr() == A_o.t.data_ptr()
    kk = k % 3
    assert A_eps.unchanged(), "eps written"
    assert A_h.unchanged(kk * tot, (kk + 1) * tot), "a history slot other than k % 3, or its surroundings, written"
    assert A_o.unchanged(0, tot), "written outside x_out"
    if not alias:
        assert A_x.unchanged(), "x written"
    if A_m:
        assert A_m.unchanged(0, 2 * tot), "written outside x_model"
    return (A_o.t.cpu().numpy().reshape(x.shape), A_h.t.cpu().numpy().reshape(3, tot),
            A_m.t.cpu().float().numpy().reshape(2, *x.shape) if A_m else None)


@pytest.mark.parametrize("shape", dc.D3_SHAPES, ids=lambda s: "n%d_C%d_i%d" % s)
def test_exact_cases_per_element(ops, dev, shape):
    """D1 x D3: bit-exact against the CPU model for fp16 and fp32 eps, orders 1 - 3, both solver types, dense and
    2 * C * inner pitch, x_out aliasing x, x_model in fp16 / fp32 - inside NaN arenas."""
    for ci, case in enumerate(dc.d1_cases([shape])):
        for half in (True, False):
            v = ci * 2 + int(half)
            pitch2, alias, xm = bool(v & 1) ^ bool(ci & 2), bool(v & 2), (None, torch.float16, torch.float32)[v % 3]
            want, want_h = dc.reference_step(case.row, case.eps, case.x, case.hist, case.k, half, "reciprocal")
            got, got_h, got_m = launch(ops, dev, case.row, case.k, case.eps, case.x, case.hist, half, pitch2, alias, xm)
            tag = (case.name, half, pitch2, alias, xm)
            assert np.isfinite(got).all(), tag
            assert np.array_equal(got, want), (tag, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())
            assert np.array_equal(got_h, want_h), tag
            if xm is not None:
                cast = torch.from_numpy(want).to(xm).float().numpy()
                assert np.array_equal(got_m[0], cast) and np.array_equal(got_m[1], cast), tag


@pytest.fixture(scope="module")
def d2_data():
    shape = (2, 4, 1056)
    return dict(shape=shape, eps=dc.gauss((4, 4, 1056), 11), x=dc.gauss(shape, 12),
                hist=dc.gauss((3, 2 * 4 * 1056), 13).astype(np.float32))


@pytest.mark.parametrize("half", [True, False], ids=["fp16eps", "fp32eps"])
def test_eager_parity_on_real_schedule_rows(ops, dev, d2_data, half):
    """D2: bit-identical to the solver's own eager expressions (_guide, _x0_of_noise, _multistep) run on the GPU on the
    same tensors - which is what fixes the form of the division (reciprocal) - and to the CPU model in that form."""
    s = dc.make_solver(4.5)
    shape, x, hist = d2_data["shape"], d2_data["x"].astype(np.float32), d2_data["hist"]
    eps = d2_data["eps"].astype(np.float16 if half else np.float32)
    eps_g = torch.from_numpy(eps).to(dev)
    x_g, h_g = torch.from_numpy(x).to(dev), torch.from_numpy(hist).to(dev)
    for name, k, row, (steps, order, st, lower) in dc.d2_rows():
        ts = s.time_steps("time_uniform", s.ns.T, 1.0 / s.ns.total_N, steps)
        o = int(row[dc.ORDER])
        assert o == s.multistep_orders(steps, order, lower)[k]
        m_k = s._x0_of_noise(x_g, ts[k], s._guide(eps_g))
        assert m_k.dtype == torch.float32
        prev = [h_g[(k - j) % 3].view(shape) for j in range(o - 1, 0, -1)] + [m_k]
        want = s._multistep(x_g, prev, [ts[k - j] for j in range(o - 1, -1, -1)], ts[k + 1], o, st)
        rows = np.zeros((k + 1, dc.ROW), dtype=np.float32)
        rows[k] = row
        coef = torch.from_numpy(rows).to(dev)
        h2 = h_g.clone()
        got = ops.cfg_dpmpp_step(eps_g, x_g, h2, coef, k)
        assert torch.equal(h2[k % 3].view(shape), m_k), (name, "x0", int((h2[k % 3].view(shape) != m_k).sum()))
        assert torch.equal(got, want), (name, int((got != want).sum()), float((got - want).abs().max()))
        ref, ref_h = dc.reference_step(row, eps, x, hist, k, half, "reciprocal")
        assert np.array_equal(got.cpu().numpy(), ref) and np.array_equal(h2.cpu().numpy(), ref_h), name
        for j in (1, 2):
            assert torch.equal(h2[(k + j) % 3], h_g[(k + j) % 3]), name


def test_learned_sigma_channels_are_never_read(ops, dev):
    """eps as the chunk(2, dim=1)[0] view of a [2n, 2C, H, W] output whose other half is NaN: finite output."""
    n, C, H, W = 2, 4, 6, 10
    full = torch.full((2 * n, 2 * C, H, W), float("nan"), dtype=torch.float16, device=dev)
    e = torch.from_numpy(dc.gauss((2 * n, C, H, W), 5)).half().to(dev)
    full[:, :C] = e
    view = full.chunk(2, dim=1)[0]
    assert not view.is_contiguous() and view.stride(0) == 2 * C * H * W and ops.cfg_dpmpp_step_ok(view, torch.zeros(n, C, H, W, device=dev))
    x = torch.from_numpy(dc.gauss((n, C, H, W), 6)).to(dev)
    rows = dc.make_solver().multistep_rows(5, 2).to(dev)
    hist = torch.zeros(3, x.numel(), device=dev)
    xm = torch.empty(2 * n, C, H, W, dtype=torch.float16, device=dev)
    a = ops.cfg_dpmpp_step(view, x, hist, rows, 0, x_model=xm)
    b = ops.cfg_dpmpp_step(e, x, hist.clone(), rows, 0)
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(xm[:n], a.half()) and torch.equal(xm[n:], a.half())


# ---------------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("half", [True, False], ids=["fp16model", "fp32model"])
def test_analytic_trajectories_fused_equals_eager(ops, dev, half):
    """20 steps at orders 1, 2, 3 and 'taylor' (and a 5-step order-3 run without lower_order_final): fused == eager, bit
    for bit, the model-input times included; a step_callback keeps tensors no later step writes."""
    x = torch.from_numpy(dc.gauss((2, 4, 8, 8), 21)).to(dev)
    for steps, order, st, lower in ((20, 1, "dpmsolver", True), (20, 2, "dpmsolver", True), (20, 3, "dpmsolver", True),
                                    (20, 2, "taylor", True), (5, 3, "dpmsolver", False), (3, 3, "dpmsolver", True)):
        calls_e, calls_f, seen_e, seen_f = [], [], [], []
        kw = dict(steps=steps, order=order, solver_type=st, lower_order_final=lower)
        want = dc.make_solver(4.5, dc.analytic_model(half, calls_e)).sample(
            x, fused=False, step_callback=lambda i, v: seen_e.append((i, v)), **kw)
        n0 = _calls()
        got = dc.make_solver(4.5, dc.analytic_model(half, calls_f)).sample(
            x, fused=True, step_callback=lambda i, v: seen_f.append((i, v)), **kw)
        assert _calls() - n0 == steps                                    # one C-ABI launch per model call
        assert torch.equal(got, want), (steps, order, st, float((got - want).abs().max()))
        assert len(calls_f) == steps and all(torch.equal(a, b) for a, b in zip(calls_e, calls_f))
        assert [i for i, _ in seen_f] == [i for i, _ in seen_e]
        assert all(torch.equal(a[1], b[1]) for a, b in zip(seen_e, seen_f))
        # denoise_to_zero: the extra call stays eager
        assert torch.equal(dc.make_solver(4.5, dc.analytic_model(half)).sample(x, fused=True, denoise_to_zero=True, **kw),
                           dc.make_solver(4.5, dc.analytic_model(half)).sample(x, fused=False, denoise_to_zero=True, **kw))


def _calls():
    from viditq_amd import _lib
    return _lib.CALLS[0]


def test_unfused_modes_launch_no_fused_step(ops, dev, monkeypatch):
    """cfg_scale == 1, no uncondition, the singlestep solvers: eager as before, also with fused=True."""
    n_calls = [0]
    orig = ops.cfg_dpmpp_step

    def counted(*a, **k):
        n_calls[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(ops, "cfg_dpmpp_step", counted)
    x = torch.from_numpy(dc.gauss((1, 4, 4, 4), 2)).to(dev)
    model = lambda x_, t, y, **kw: x_.half() * 0.1   # noqa: E731
    dc.make_solver(1.0, model).sample(x, steps=4, order=2, fused=True)
    s = dc.make_solver(4.5, dc.analytic_model(True))
    s.sample(x, steps=4, order=2, method="singlestep", fused=True)
    s.sample(x, steps=4, order=2, fused=False)
    assert n_calls[0] == 0
    s.sample(x, steps=4, order=2, fused=True)
    assert n_calls[0] == 4
    # a model output the kernel does not take (bf16): the eager route continues from that first call
    calls = []
    bf = lambda x_, t, y, **kw: (calls.append(1), dc.analytic_model(False)(x_, t, y).bfloat16())[1]   # noqa: E731
    a = dc.make_solver(4.5, bf).sample(x, steps=4, order=2, fused=True)
    assert n_calls[0] == 4 and len(calls) == 4
    assert torch.equal(a, dc.make_solver(4.5, bf).sample(x, steps=4, order=2, fused=False))


def _tiny_pixart(dev):
    import viditq_amd  # noqa
    from viditq_amd.config import to_config
    from viditq_amd.qdiff.models import QuantModel
    from viditq_amd.qdiff.quantizer import BaseQuantizer
    from viditq_amd.t2i import PixArtMS
    g = load_npz("tiny_pixart_w8a8.npz")
    m = PixArtMS(input_size=16, depth=2, hidden_size=64, num_heads=4, model_max_length=12, caption_channels=32,
                 dtype=torch.float16)
    m.load_state_dict(state_dict_of(g), strict=True)
    m = m.half().to(dev).eval()
    wq = to_config(dict(n_bits=8, per_group="channel", channel_dim=0, scale_method="min_max", round_mode="nearest"))
    aq = to_config(dict(n_bits=8, per_group="token", scale_method="min_max", round_mode="nearest_ste", running_stat=False,
                        dynamic=True, sym=False, n_spatial_token=64, n_temporal_token=1, n_prompt=12,
                        smooth_quant=dict(enable=False)))
    qnn = QuantModel(m, wq, aq, model_type="pixart")
    qnn.set_module_name_for_quantizer(qnn.model)
    qnn.fp_layer_list = ["x_embedder", "t_embedder", "t_block", "y_embedder", "csize_embedder", "ar_embedder"]
    qp = quant_params_of(g)
    qnn.set_quant_params_dict({mod.module_name: [qp.get(mod.module_name, {}), {}] for mod in qnn.model.modules()
                               if isinstance(mod, BaseQuantizer)})
    qnn.set_quant_init_done("weight")
    qnn.set_quant_init_done("activation")
    qnn.set_quant_state(True, True)
    return g, qnn


def test_tiny_pixart_trajectory_fused_equals_eager(ops, dev):
    """The t2i loop of test_tiny_pixart_dpm_solver_trajectory (5 steps, order 2, cfg 4.5): fused == eager bit for bit,
    under the existing 2.5e-3 against the reference's trajectory, through GraphedModel, with an fp16 x_model, and
    as ONE captured step replayed five times (DPMStepGraph)."""
    from viditq_amd.graph import GraphedModel
    from viditq_amd.t2i.dpm_solver import DPMS_sigma
    g, qnn = _tiny_pixart(dev)
    kw = dict(condition=g["y"][:1].half().to(dev), uncondition=g["dpm_null_y"].half().to(dev), cfg_scale=4.5,
              model_kwargs=dict(data_info=None, mask=g["mask"][:1].to(dev)))
    run = dict(steps=5, order=2, skip_type="time_uniform", method="multistep")
    z = g["dpm_z"].to(dev)
    eager = DPMS_sigma(qnn.forward_with_dpmsolver, **kw).sample(z, fused=False, **run)
    fused = DPMS_sigma(qnn.forward_with_dpmsolver, **kw).sample(z, fused=True, **run)
    assert torch.equal(fused, eager), float((fused - eager).abs().max())
    assert rel_l2(fused.cpu().float(), g["dpm_final"]) < 2.5e-3
    gm = GraphedModel(qnn.forward_with_dpmsolver, qnn=qnn)
    fused_g = DPMS_sigma(gm, **kw).sample(z, fused=True, **run)
    assert torch.equal(fused_g, eager) and len(gm.graphs) == 1
    assert rel_l2(fused_g.cpu().float(), g["dpm_final"]) < 2.5e-3
    s16 = DPMS_sigma(qnn.forward_with_dpmsolver, **kw)
    s16.model_input_dtype = torch.float16                 # the kernel makes the model's cast
    assert torch.equal(s16.sample(z, fused=True, **run), eager)
    sg = s16.step_graph(z, steps=5, order=2)
    assert torch.equal(sg.run(z), eager)
    assert torch.equal(sg.run(z), eager)                  # and again: run() resets latent, time and counter


# ---------------------------------------------------------------------------------------------------- counter form
def test_counter_form_replays_one_captured_step(ops, dev):
    """{analytic model, step(step=counter), advance} in one captured graph, replayed ``steps`` times == the host-row
    form; the model-input time after each replay is the reference expression (t - 1/N) * 1000 in fp32; the counter
    saturates at the last row."""
    x = torch.from_numpy(dc.gauss((2, 4, 8, 8), 31)).to(dev)
    for half, steps, order, st in ((True, 20, 2, "dpmsolver"), (False, 20, 3, "dpmsolver"), (True, 5, 2, "taylor")):
        s = dc.make_solver(4.5, dc.analytic_model(half))
        want = s.sample(x, steps=steps, order=order, solver_type=st, fused=True)
        assert torch.equal(want, s.sample(x, steps=steps, order=order, solver_type=st, fused=False))
        sg = s.step_graph(x, steps=steps, order=order, solver_type=st)
        ts = s.time_steps("time_uniform", s.ns.T, 1.0 / s.ns.total_N, steps)
        t_seen, c_seen = [], []
        got = sg.run(x, step_callback=lambda i, v: (t_seen.append(sg.t.clone()), c_seen.append(sg.step.clone())))
        assert torch.equal(got, want), (half, steps, order, st)
        for k in range(steps):
            t_ref = (ts[k + 1].float() - 1.0 / s.ns.total_N) * 1000.0
            assert t_seen[k].dtype == torch.float32 and bool((t_seen[k].cpu() == t_ref).all()), k
            assert int(c_seen[k]) == min(k + 1, steps - 1)
        sg.graph.replay()                                  # one more: the counter stays on the last row
        torch.cuda.synchronize()
        assert int(sg.step) == steps - 1 and bool(torch.isfinite(sg.x).all())


def test_advance_saturates_and_fills(ops, dev):
    rows = torch.zeros(3, dc.ROW)
    rows[:, dc.T_NEXT] = torch.tensor([10.0, 20.0, 30.0])
    rows = rows.to(dev)
    buf = torch.full((300 + 2,), float("nan"), device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for want_t, want_c in ((10.0, 1), (20.0, 2), (30.0, 2), (30.0, 2)):
        ops.dpmpp_advance(step, rows, buf[1:301])
        assert int(step) == want_c and bool((buf[1:301] == want_t).all())
        assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[301]))


# ---------------------------------------------------------------------------------------------------- the switch
CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import dpm_step_cases as dc
import viditq_amd
from viditq_amd import ops
from viditq_amd.t2i import dpm_solver as ds
n = [0]
orig = ops.cfg_dpmpp_step
def counted(*a, **k):
    n[0] += 1
    return orig(*a, **k)
ops.cfg_dpmpp_step = counted
x = torch.from_numpy(dc.gauss((1, 4, 4, 4), 3)).cuda()
a = dc.make_solver(4.5, dc.analytic_model(True)).sample(x, steps=5, order=2)
c1 = n[0]
b = dc.make_solver(4.5, dc.analytic_model(True)).sample(x, steps=5, order=2, fused=False)
print("SWITCH", int(ds._DPM_FUSED), c1, n[0], int(torch.equal(a, b)))
"""


def test_switch_in_a_child_process(dev):
    """VQ_DPM_FUSED=1 at import: sample() takes the fused route (5 launches for 5 steps), fused=False still overrides."""
    env = dict(os.environ, VQ_DPM_FUSED="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SWITCH")][-1]
    assert line.split() == ["SWITCH", "1", "5", "5", "1"], line

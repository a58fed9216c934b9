"""The IDDPM sampler and its fused step without a GPU: the schedule and the eager loop against vectors recorded from the
reference (tests/golden/t2i_iddpm.npz, made by tests/golden/make_golden_iddpm.py), the exact cases prove themselves, the
coefficient table drives the CPU model of ddpm_step_cases.py along the recorded trajectory, the entry point refuses bad
arguments in the documented order before any HIP call, and the fused route is off unless asked for."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddpm_step_cases as pc
from helpers import _FakeTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "t2i_iddpm.npz"))
RESPACINGS = ("100", "20", "10", "ddim25")
ARRAYS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
          "posterior_log_variance_clipped", "log_betas")
CFG = 4.5


# ---------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("resp", RESPACINGS)
def test_schedule_arrays_against_the_reference(resp):
    s = pc.make_sampler(resp)
    assert list(s.timestep_map) == GOLD[resp + ".timestep_map"].tolist()
    assert s.num_timesteps == len(s.timestep_map) == {"100": 100, "20": 20, "10": 10, "ddim25": 25}[resp]
    for name in ARRAYS:
        got, want = getattr(s, name), GOLD["%s.%s" % (resp, name)]
        assert got.dtype == np.float64 and got.shape == want.shape
        # the same numpy expressions on the same float64 betas: equal, not merely close (rtol 1e-12 is the issue's floor)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        assert np.array_equal(got, want), (resp, name, float(np.abs(got - want).max()))


@pytest.mark.parametrize("resp", RESPACINGS)
@pytest.mark.parametrize("clip", [False, True])
def test_step_rows_are_the_fp32_casts_in_loop_order(resp, clip):
    s = pc.make_sampler(resp)
    rows = s.step_rows(CFG, clip)
    steps = s.num_timesteps
    assert tuple(rows.shape) == (steps, pc.ROW) and rows.dtype == torch.float32
    r = rows.numpy()
    rev = lambda name: GOLD["%s.%s" % (resp, name)][::-1].astype(np.float32)   # noqa: E731  row k belongs to i = steps-1-k
    for col, name in ((pc.A, ARRAYS[0]), (pc.B, ARRAYS[1]), (pc.C1, ARRAYS[2]), (pc.C2, ARRAYS[3]), (pc.MIN_LOG, ARRAYS[4]),
                      (pc.MAX_LOG, ARRAYS[5])):
        assert np.array_equal(r[:, col].view(np.int32), rev(name).view(np.int32)), (resp, name)
    assert r[:, pc.CFG].tolist() == [CFG] * steps and r[:, pc.CLIP].tolist() == [float(clip)] * steps
    assert r[:, pc.NONZERO].tolist() == [1.0] * (steps - 1) + [0.0]
    tm = GOLD[resp + ".timestep_map"].tolist()
    assert r[:, pc.T_NEXT].tolist() == [float(tm[(steps - 1 - k) - 1]) for k in range(steps)]
    assert r[-1, pc.T_NEXT] == tm[-1]                                  # the last row wraps to the first forward's time
    assert not r[:, 9:14].any() and not r[:, 15].any()


# ---------------------------------------------------------------------------------------------------- eager loop
def _run_eager(s, z, noise, clip, half=False, cfg=CFG, **kw):
    calls, seen = [], []
    final = s.p_sample_loop(pc.analytic_cfg_model(half, calls), tuple(z.shape), z, clip_denoised=clip,
                            model_kwargs=dict(cfg_scale=cfg), noise_steps=noise,
                            step_callback=lambda i, smp, x0: seen.append((i, smp, x0)), **kw)
    return final, seen, [int(t[0][0]) for t in calls]


@pytest.mark.parametrize("clip", [False, True])
def test_eager_loop_reproduces_the_recorded_trajectories(clip):
    """sample and pred_xstart of every step, bit for bit, with the recorded noise stack."""
    s = pc.make_sampler("10")
    z, noise = torch.from_numpy(GOLD["traj.z"]), torch.from_numpy(GOLD["traj.noise"])
    key = "traj.clip%d" % int(clip)
    final, seen, ts = _run_eager(s, z, noise, clip)
    assert ts == GOLD[key + ".timesteps"].tolist() == list(s.timestep_map)[::-1]
    assert [i for i, _, _ in seen] == list(range(10))[::-1]
    for k, (_, smp, x0) in enumerate(seen):
        assert smp.dtype == torch.float32
        assert np.array_equal(smp.numpy(), GOLD[key + ".sample"][k]), (k, "sample")
        assert np.array_equal(x0.numpy(), GOLD[key + ".pred_xstart"][k]), (k, "pred_xstart")
    assert torch.equal(final, seen[-1][1])
    if clip:
        assert float(np.abs(GOLD[key + ".pred_xstart"]).max()) <= 1.0
        assert not np.array_equal(GOLD[key + ".sample"], GOLD["traj.clip0.sample"])
    # the progressive form yields the same dicts, and the loop draws the stack itself from the global generator
    torch.manual_seed(7)
    outs = list(s.p_sample_loop_progressive(pc.analytic_cfg_model(False), tuple(z.shape), z, clip_denoised=clip,
                                            model_kwargs=dict(cfg_scale=CFG)))
    assert len(outs) == 10 and np.array_equal(outs[-1]["sample"].numpy(), GOLD[key + ".sample"][-1])
    # a generator in place of the global one: the same draws as its own randn calls
    g = torch.Generator().manual_seed(11)
    stack = torch.stack([torch.randn(*z.shape, generator=g) for _ in range(10)])
    a = _run_eager(s, z, stack, clip)[0]
    b = s.p_sample_loop(pc.analytic_cfg_model(False), tuple(z.shape), z, clip_denoised=clip,
                        model_kwargs=dict(cfg_scale=CFG), generator=torch.Generator().manual_seed(11))
    assert torch.equal(a, b)


def test_live_run_against_the_imported_reference():
    """With the reference at hand: a second seed, both clip settings and an fp16 model output, bit for bit."""
    sys.path.insert(0, ROOT)
    from oracle import ref_import
    if not ref_import.available():
        return                                                        # the recorded vectors above are the check
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_iddpm as mg
    IDDPM = mg.reference_iddpm()
    s = pc.make_sampler("10")
    for clip, half in ((False, False), (True, False), (False, True)):
        want_s, want_0, want_t = mg.reference_trajectory(IDDPM, "10", clip, seed=23, half=half)
        final, seen, ts = _run_eager(s, mg.start_latent(23), mg.noise_stack(23, 10), clip, half)
        assert ts == want_t
        assert torch.equal(torch.stack([v for _, v, _ in seen]), want_s), (clip, half)
        assert torch.equal(torch.stack([v for _, _, v in seen]), want_0), (clip, half)


# ---------------------------------------------------------------------------------------------------- the CPU model
@pytest.mark.parametrize("case", pc.p1_cases(), ids=lambda c: c.name)
def test_p1_cases_are_exact_in_fp16_and_fp32(case):
    big = pc.p1_prove(case)
    assert 0 < big < 2.0 ** 11


def test_p1_operands_encode_their_position():
    c = pc.P1Case((2, 3, 7), 1, 0, 3)
    flat = np.concatenate([c.eps.reshape(-1), c.x.reshape(-1), c.noise.reshape(-1)])
    assert np.array_equal(flat * 16, np.round(flat * 16)) and np.abs(flat).max() <= 8
    assert (c.eps[0] != c.eps[2]).all() and (c.eps[0] != c.eps[1]).all()          # batch halves, batch elements
    assert (c.eps[:, :3] != c.eps[:, 3:]).all()                                   # eps and variance channels
    assert (c.x[:, 0] != c.x[:, 1]).all() and (c.x[..., 0] != c.x[..., 1]).all() and (c.x != c.noise).all()
    # every choice of the kernel is visible in the expected output
    base = c.expected()[0]
    for other in (pc.P1Case((2, 3, 7), 0, 0, 3), pc.P1Case((2, 3, 7), 1, 1, 3), pc.P1Case((2, 3, 7), 1, 0, 1)):
        assert not np.array_equal(other.expected()[0], base), other.name


@pytest.mark.parametrize("clip", [False, True])
def test_model_through_step_rows_follows_the_recorded_trajectory(clip):
    """x0 of the CPU model, driven by step_rows from the recorded start latent, equals the reference's pred_xstart at every
    step, and mean - on the last step, where nothing is added - its sample, bit for bit; out through torch's own exp equals
    sample at every step."""
    s = pc.make_sampler("10")
    z, noise = torch.from_numpy(GOLD["traj.z"]), torch.from_numpy(GOLD["traj.noise"])
    key = "traj.clip%d" % int(clip)
    steps = pc.run_table(s, z, noise, CFG, clip, half=False)
    assert len(steps) == 10
    for k, (x0, mean, out) in enumerate(steps):
        want0, want = GOLD[key + ".pred_xstart"][k][:1].reshape(x0.shape), GOLD[key + ".sample"][k][:1].reshape(out.shape)
        assert np.array_equal(x0, want0), (k, "x0")
        assert np.array_equal(out, want), (k, "out")
    assert np.array_equal(steps[-1][1], GOLD[key + ".sample"][-1][:1].reshape(steps[-1][1].shape))


# ---------------------------------------------------------------------------------------------------- refusals
GOOD = 1 << 20
PTRS = ("eps", "x", "noise", "coef", "step", "x_out", "x0_out", "x_model", "stream")


def _step_args(**kw):
    a = dict(eps=GOOD, x=GOOD, noise=GOOD, coef=GOOD, step=None, x_out=GOOD, x0_out=None, x_model=None, n=1, C=4, inner=8,
             ld_eps=64, guided=3, row=0, n_rows=1, eps_f16=0, xm_f16=0, stream=None)
    a.update(kw)
    return [ctypes.c_void_p(v) if k in PTRS and v is not None else v for k, v in a.items()]


# (arguments on top of a valid base, the code the entry point must return); none of them reaches a HIP call
REFUSALS = [
    (dict(eps=None), -1), (dict(x=None), -1), (dict(noise=None), -1), (dict(coef=None), -1), (dict(x_out=None), -1),
    (dict(n=0), -1), (dict(C=0), -1), (dict(inner=0), -1), (dict(inner=-8), -1), (dict(n_rows=0), -1),
    (dict(row=-1), -1), (dict(row=1), -1), (dict(guided=-1), -1),
    (dict(ld_eps=63), -2),                                   # < 2 * C * inner
    (dict(ld_eps=32), -2),                                   # the DPM step's C * inner is not enough here
    (dict(guided=5), -2),                                    # > C
    (dict(ld_eps=66), -2),                                   # inner % 4 == 0: four elements per access
    (dict(eps=GOOD + 8), -2), (dict(eps=GOOD + 4, eps_f16=1), -2), (dict(x=GOOD + 4), -2), (dict(noise=GOOD + 8), -2),
    (dict(x_out=GOOD + 4), -2), (dict(x0_out=GOOD + 8), -2), (dict(x_model=GOOD + 8), -2),
    (dict(x_model=GOOD + 4, xm_f16=1), -2),
    (dict(inner=7, ld_eps=56, eps=GOOD + 2), -2),            # one element per access: still its own 4 bytes
    (dict(inner=7, ld_eps=55), -2),
    (dict(step=GOOD + 2), -2), (dict(coef=GOOD + 2), -2),
    (dict(eps_f16=2), -4), (dict(eps_f16=-1), -4), (dict(xm_f16=3), -4),
    # the order: EINVAL before ESHAPE before EUNSUP, and within EINVAL / ESHAPE the table's order cannot be told apart
    (dict(eps=None, ld_eps=63, eps_f16=2), -1), (dict(row=-1, eps_f16=2), -1), (dict(guided=-1, ld_eps=63), -1),
    (dict(ld_eps=63, eps_f16=2), -2), (dict(guided=5, xm_f16=2), -2), (dict(x=GOOD + 4, xm_f16=7), -2),
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
        assert lib.vq_cfg_ddpm_step(*_step_args(**kw)) == code, kw
    null = [None if k in PTRS else 1 for k in ("eps", "x", "noise", "coef", "step", "x_out", "x0_out", "x_model", "n", "C",
                                                "inner", "ld_eps", "guided", "row", "n_rows", "eps_f16", "xm_f16", "stream")]
    assert lib.vq_cfg_ddpm_step(*null) == -1


def _fakes(kw):
    a = dict(eps=GOOD, x=GOOD, n=1, C=4, inner=8, ld_eps=64, eps_f16=0)
    a.update({k: v for k, v in kw.items() if k in a})
    n, C, inner = a["n"], a["C"], a["inner"]
    dt = {0: torch.float32, 1: torch.float16}.get(a["eps_f16"], torch.bfloat16)
    eps = _FakeTensor((2 * n, 2 * C, inner), (a["ld_eps"], inner, 1), a["eps"], dt)
    x = _FakeTensor((n, C, inner), (C * inner, inner, 1), a["x"], torch.float32)
    return eps, x


def test_ok_predicate_agrees_with_the_entry_point():
    """ops.cfg_ddpm_step_ok says no exactly where the entry point refuses, on every row of the table that is about eps and
    x (what the predicate is given), and on a grid of shapes, pitches and misalignments both give the same answer."""
    lib = _lib()
    from viditq_amd import ops
    asked = 0
    for kw, code in REFUSALS:
        if not set(kw) <= {"eps", "x", "n", "C", "inner", "ld_eps", "eps_f16"} or kw.get("eps", 1) is None \
                or kw.get("x", 1) is None or min(kw.get("n", 1), kw.get("C", 1), kw.get("inner", 1)) < 0:
            continue
        assert ops.cfg_ddpm_step_ok(*_fakes(kw)) is False, kw
        asked += 1
    assert asked >= 10
    grid = 0
    for n, C, inner in ((1, 4, 8), (2, 3, 7), (3, 4, 12), (1, 1, 1), (2, 4, 2)):
        for pad in (-1, 0, 1, 2, 4, 8):
            for off in (0, 2, 4, 8, 16):
                for f16 in (0, 1):
                    kw = dict(n=n, C=C, inner=inner, ld_eps=2 * C * inner + pad, eps=GOOD + off, eps_f16=f16)
                    code = _refusal_only(lib, kw)
                    assert ops.cfg_ddpm_step_ok(*_fakes(kw)) is (code is None), (kw, code)
                    kw = dict(kw, eps=GOOD, x=GOOD + off)
                    assert ops.cfg_ddpm_step_ok(*_fakes(kw)) is (_refusal_only(lib, kw) is None), kw
                    grid += 2
    assert grid == 600
    eps, x = _fakes({})
    x.dtype = torch.float16
    assert ops.cfg_ddpm_step_ok(eps, x) is False                       # the latent is fp32
    eps, x = _fakes({})
    eps._st = (64, 1, 8)
    assert ops.cfg_ddpm_step_ok(eps, x) is False                       # not dense within a batch element
    eps, x = _fakes({})
    eps.shape = (2, 4, 8)
    assert ops.cfg_ddpm_step_ok(eps, x) is False                       # no variance channels
    eps, x = _fakes({})
    eps.is_cuda = False
    assert ops.cfg_ddpm_step_ok(eps, x) is False


def _refusal_only(lib, kw):
    """The entry point's refusal code for ``kw``, or None where it would launch - asked WITHOUT launching: a null stream
    and dummy pointers must not reach a kernel, so a layout the table accepts is recognised by making the one further
    argument invalid that is checked last (a dtype flag): -4 then means "everything before passed"."""
    code = lib.vq_cfg_ddpm_step(*_step_args(**dict(kw, xm_f16=9, guided=min(3, kw.get("C", 4)))))
    return None if code == -4 else code


def test_ops_refuse_cpu_tensors():
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib as L, ops
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)   # noqa: E731
    with pytest.raises(ops.VQError):
        ops.cfg_ddpm_step(f(2, 8, 8), f(1, 4, 8), f(1, 4, 8), f(1, L.DDPM_ROW), 0)
    assert ops.cfg_ddpm_step_ok(f(2, 8, 8), f(1, 4, 8)) is False
    assert L.DDPM_ROW == pc.ROW == L.DPMPP_ROW and L.DDPM_T_NEXT == pc.T_NEXT == L.DPMPP_T_NEXT
    assert (L.DDPM_CFG, L.DDPM_A, L.DDPM_B, L.DDPM_C1, L.DDPM_C2, L.DDPM_MIN_LOG, L.DDPM_MAX_LOG, L.DDPM_NONZERO,
            L.DDPM_CLIP) == (pc.CFG, pc.A, pc.B, pc.C1, pc.C2, pc.MIN_LOG, pc.MAX_LOG, pc.NONZERO, pc.CLIP)
    hdr = open(os.path.join(ROOT, "include", "viditq.h")).read()
    for name in ("CFG", "A", "B", "C1", "C2", "MIN_LOG", "MAX_LOG", "NONZERO", "CLIP", "T_NEXT", "ROW"):
        assert "#define VQ_DDPM_%s %d " % (name, getattr(L, "DDPM_" + name)) in hdr, name


# ---------------------------------------------------------------------------------------------------- settings
def test_unsupported_settings_say_so():
    import viditq_amd  # noqa: F401
    from viditq_amd.t2i import IDDPM
    for kw in (dict(predict_xstart=True), dict(learn_sigma=False), dict(pred_sigma=False), dict(use_kl=True),
               dict(rescale_learned_sigmas=True), dict(noise_schedule="squaredcos_cap_v2"),
               dict(learn_sigma=False, sigma_small=True)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            IDDPM("10", **kw)
    s = IDDPM("10", "linear", False, False, False, True, True, False, 1000, False, False)    # the factory's positional surface
    assert s.num_timesteps == 10 and IDDPM("", diffusion_steps=50).num_timesteps == 50
    z = torch.zeros(2, 4, 2, 2)
    fn = lambda *a, **k: None   # noqa: E731
    for kw in (dict(cond_fn=fn), dict(denoised_fn=fn)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            s.p_sample_loop(pc.analytic_cfg_model(False), z.shape, z, model_kwargs=dict(cfg_scale=CFG), **kw)
        with pytest.raises(NotImplementedError):
            s.p_sample(pc.analytic_cfg_model(False), z, torch.zeros(2, dtype=torch.long), model_kwargs=dict(cfg_scale=CFG),
                       **kw)
        with pytest.raises(NotImplementedError):
            next(s.p_sample_loop_progressive(pc.analytic_cfg_model(False), z.shape, z, model_kwargs=dict(cfg_scale=CFG),
                                             **kw))
    for name in ("p_mean_variance", "p_sample", "p_sample_loop", "p_sample_loop_progressive", "p_sample_graph",
                 "num_timesteps", "timestep_map", "step_rows"):
        assert hasattr(s, name), name


# ---------------------------------------------------------------------------------------------------- the switch
def test_cpu_latents_and_foreign_models_stay_eager(monkeypatch):
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    from viditq_amd.t2i import iddpm
    assert iddpm._DDPM_FUSED == (os.environ.get("VQ_DDPM_FUSED", "0") != "0")

    def counted(*a, **k):
        raise AssertionError("the fused step was launched")
    monkeypatch.setattr(ops, "cfg_ddpm_step", counted)
    s = pc.make_sampler("10")
    z, noise = torch.from_numpy(GOLD["traj.z"]), torch.from_numpy(GOLD["traj.noise"])
    base = _run_eager(s, z, noise, False, fused=False)[0]
    assert torch.equal(_run_eager(s, z, noise, False, fused=True)[0], base)       # not a net of the package
    net = pc.analytic_net(False)
    got = s.p_sample_loop(net.forward_with_cfg, tuple(z.shape), z, clip_denoised=False, noise_steps=noise, fused=True,
                          model_kwargs=dict(y=torch.zeros(2, 1, 2, 4), cfg_scale=CFG))
    assert torch.equal(got, base)                                                 # a net of the package, a CPU latent
    assert np.array_equal(got.numpy(), GOLD["traj.clip0.sample"][-1])


CHILD = r"""
import sys, torch
sys.path.insert(0, %r)
import viditq_amd
from viditq_amd.t2i import iddpm
print("SWITCH", int(iddpm._DDPM_FUSED))
"""


@pytest.mark.parametrize("value,want", [("1", "1"), ("0", "0"), (None, "0")])
def test_switch_is_read_in_a_child_process(value, want):
    env = {k: v for k, v in os.environ.items() if k != "VQ_DDPM_FUSED"}
    if value is not None:
        env["VQ_DDPM_FUSED"] = value
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("SWITCH")][-1].split() == ["SWITCH", want]


def test_step_graph_refuses_a_forward_that_moves_a_running_statistic():
    import types
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    from viditq_amd.graph import DDPMStepGraph
    from viditq_amd.qdiff.models.quant_layer import QuantLayer
    lay = object.__new__(QuantLayer)
    lay.__dict__.update(weight_quant=True, act_quant=True, weight_quantizer=types.SimpleNamespace(n_bits=8),
                        act_quantizer=types.SimpleNamespace(n_bits=8), smooth_quant=False, smooth_quant_running_stat=True,
                        channel_wise_scale_type="momentum_act_max")

    class Root:
        def modules(self):
            return [lay]

        def forward(self, x, t, y, mask=None, **kw):
            raise AssertionError("the forward ran")
    with pytest.raises(ops.VQError, match="running"):
        DDPMStepGraph(Root().forward, None, None, {}, torch.zeros(1, 4, 2, 2), torch.zeros(2, pc.ROW), 999.0)

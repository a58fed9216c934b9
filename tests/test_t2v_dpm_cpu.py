"""The STDiT DPM-Solver++ scheduler and its patch-major step without a GPU: schedule and trajectories against the
reference's own recordings (tests/golden/t2v_dpm_solver.npz) bit for bit, the coefficient table through a NumPy statement
of the kernel, the index map against STDiT.unpatchify, the entry point's refusals and their order, the host logic."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import dpm_step_cases as dc
import t2v_dpm_cases as tc
from helpers import GOLD, _FakeTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = [(s, c) for s in tc.STEPS if s >= 2 for c in tc.CFGS]


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLD, "t2v_dpm_solver.npz"))
    return {k: z[k] for k in z.files}


def _sched():
    import viditq_amd  # noqa: F401
    from viditq_amd.t2v import dpm_solver as vd
    return vd


def _solver(cfg=4.0, net=None, split=False):
    vd = _sched()
    enc = tc.ToyTextEncoder()
    return vd.DMP_SOLVER(20, cfg).solver(net or tc.AnalyticSTDiT(), enc, tc.PROMPTS, None, split)


# ---------------------------------------------------------------------------------------------------- schedule
def test_schedule_and_time_steps_equal_the_reference_bit_for_bit(gold):
    s = _solver()
    assert np.array_equal(s.ns.t_array.numpy(), gold["ns.t_array"]) and s.ns.t_array.dtype == torch.float32
    assert np.array_equal(s.ns.log_alpha_array.numpy(), gold["ns.log_alpha_array"])
    assert s.ns.total_N == int(gold["ns.total_N"])
    for steps in tc.STEPS:
        ts = s.time_steps("time_uniform", s.ns.T, 1.0 / s.ns.total_N, steps)
        assert ts.dtype == torch.float32 and np.array_equal(ts.numpy(), gold["ts.%d" % steps]), steps


def test_the_one_schedule_difference_from_t2i_is_pinned(gold):
    """The t2v file lowers the order of the last steps only below 10 steps: a 20-step run ends with order 2.  With the
    t2i rule the recorded 20-step trajectory is NOT reproduced, with lower_order_final(steps) it is (below)."""
    vd = _sched()
    assert [vd.lower_order_final(s) for s in (1, 2, 3, 9, 10, 20)] == [True, True, True, True, False, False]
    s = _solver()
    assert s.multistep_orders(20, 2, vd.lower_order_final(20))[-3:] == [2, 2, 2]
    assert s.multistep_orders(3, 2, vd.lower_order_final(3)) == [1, 2, 1]
    key = "traj.s20.cfg4."
    z = torch.from_numpy(gold[key + "z"])
    t2i_rule = s.sample(z, steps=20, order=2, lower_order_final=True)
    assert not np.array_equal(t2i_rule.numpy(), gold[key + "final"])
    assert np.array_equal(s.sample(z, steps=20, order=2, lower_order_final=False).numpy(), gold[key + "final"])


def test_a_step_count_below_the_order_is_refused_as_in_the_reference(gold):
    """steps = 1 with order 2 trips the reference's own assertion (recorded as refused); so it does here."""
    assert gold["refused_steps"].tolist() == [1]
    vd = _sched()
    with pytest.raises(AssertionError):
        vd.DMP_SOLVER(1, 4.0).sample(tc.AnalyticSTDiT(), tc.ToyTextEncoder(), tc.Z_SIZE, tc.PROMPTS, "cpu")


# ---------------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize("steps,cfg", RECORDED)
def test_eager_loop_reproduces_the_recorded_trajectory(gold, steps, cfg):
    vd = _sched()
    key = "traj.s%d.cfg%g." % (steps, cfg)
    calls = []
    torch.manual_seed(tc.SEED)                                  # the draw of the start latent, as the reference makes it
    got = vd.DMP_SOLVER(steps, cfg).sample(tc.AnalyticSTDiT(calls), tc.ToyTextEncoder(), tc.Z_SIZE, tc.PROMPTS, "cpu")
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), gold[key + "final"])
    assert len(calls) == steps
    for k, (x, t, y, mask) in enumerate(calls):
        assert np.array_equal(x.numpy(), gold[key + "x_in"][k]), k
        assert t.dtype == torch.float32 and np.array_equal(t.numpy(), gold[key + "t_in"][k]), k
        assert np.array_equal(y.numpy(), gold[key + "y_in"]) and np.array_equal(mask.numpy(), gold[key + "mask"])


class ReplayNet:
    """Returns the recorded output of call k and asserts that its input is the recorded input of call k."""
    dtype, patch_size, out_channels = torch.float32, tc.PATCH, tc.C_OUT

    def __init__(self, gold, key):
        self.g, self.key, self.k = gold, key, 0

    def forward(self, x, timestep, y, mask=None):
        k = self.k
        self.k += 1
        assert np.array_equal(x.numpy(), self.g[self.key + "x_in"][k]), ("input of call", k)
        assert np.array_equal(timestep.numpy(), self.g[self.key + "t_in"][k]), ("time of call", k)
        assert np.array_equal(mask.numpy(), self.g[self.key + "mask"])
        return torch.from_numpy(self.g[self.key + "out"][k])


@pytest.mark.parametrize("steps,cfg", RECORDED)
def test_replayed_model_outputs_pin_the_solver_without_the_network(gold, steps, cfg):
    vd = _sched()
    key = "traj.s%d.cfg%g." % (steps, cfg)
    net = ReplayNet(gold, key)
    got = vd.DMP_SOLVER(steps, cfg).sample(net, tc.ToyTextEncoder(), tc.Z_SIZE, tc.PROMPTS, "cpu",
                                           init_noise=torch.from_numpy(gold[key + "z"]))
    assert net.k == steps and np.array_equal(got.numpy(), gold[key + "final"])


@pytest.mark.parametrize("steps,cfg", RECORDED)
def test_row_table_through_the_numpy_kernel_follows_the_recorded_trajectory(gold, steps, cfg):
    """multistep_rows + the kernel's per-element arithmetic and index map (t2v_dpm_cases.reference_step_patch) on the
    recorded, patchified model outputs: every next model input and the final sample, bit for bit.  (The division by
    alpha_t in the CPU form, which is what recorded them.)"""
    vd = _sched()
    key = "traj.s%d.cfg%g." % (steps, cfg)
    s = vd.DMP_SOLVER(steps, cfg).solver(tc.AnalyticSTDiT(), tc.ToyTextEncoder(), tc.PROMPTS)
    rows = s.multistep_rows(steps, 2, "time_uniform", None, None, vd.lower_order_final(steps), "dpmsolver").numpy()
    n = len(tc.PROMPTS)
    x = gold[key + "z"]
    hist = np.zeros((3, x.size), dtype=np.float32)
    t_in = np.float32(s._t_val(s.time_steps("time_uniform", s.ns.T, 1.0 / s.ns.total_N, steps)[0]))
    for k in range(steps):
        assert np.array_equal(np.concatenate([x, x]), gold[key + "x_in"][k]), k
        assert (gold[key + "t_in"][k] == t_in).all(), k
        pm = tc.patchify(torch.from_numpy(gold[key + "out"][k]), tc.PATCH).numpy()
        x, hist = tc.reference_step_patch(rows[k], pm[:n], pm[n:], x, hist, k, tc.PATCH, tc.C_OUT, "divide")
        t_in = rows[k][dc.T_NEXT]
    assert np.array_equal(x, gold[key + "final"])


# ---------------------------------------------------------------------------------------------------- index map
@pytest.mark.parametrize("shape", tc.SHAPES, ids=tc.shape_id)
def test_index_map_equals_unpatchify_for_every_element(shape):
    import viditq_amd  # noqa: F401
    from viditq_amd.t2v.stdit import STDiT
    n, C, Co, T, H, W, patch, _ = shape
    P = patch[0] * patch[1] * patch[2]
    tokens = T * H * W // P
    flat = torch.arange(n * tokens * P * Co, dtype=torch.int64).reshape(n, tokens, P * Co)
    net = types.SimpleNamespace(input_size=(T, H, W), patch_size=patch, out_channels=Co)
    want = STDiT.unpatchify(net, flat)[:, :C].numpy()
    got = tc.gather(flat.numpy(), C, T, H, W, Co, patch)
    assert got.shape == (n, C, T, H, W) and np.array_equal(got, want)
    assert np.array_equal(tc.patchify(STDiT.unpatchify(net, flat), patch).numpy(), flat.numpy())


# ---------------------------------------------------------------------------------------------------- refusals
GOOD = 1 << 20
PTRS = ("eps_u", "eps_c", "x", "hist", "coef", "step", "x_out", "x_model", "stream")


def _args(**kw):
    a = dict(eps_u=GOOD, eps_c=GOOD, x=GOOD, hist=GOOD, coef=GOOD, step=None, x_out=GOOD, x_model=None, n=1, C=4, C_out=8,
             T=2, H=4, W=6, p_t=1, p_h=2, p_w=2, ld_eps=384, row=0, n_rows=1, eps_f16=0, xm_f16=0, xm_copies=1, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return [ctypes.c_void_p(v) if k in PTRS and v is not None else v for k, v in a.items()]


NARROW = dict(C=3, C_out=6, ld_eps=288)                      # one element per access
# (arguments on top of a valid base, the code the entry point must return); none of them reaches a HIP call
REFUSALS = [
    (dict(eps_u=None), -1), (dict(eps_c=None), -1), (dict(x=None), -1), (dict(hist=None), -1), (dict(coef=None), -1),
    (dict(x_out=None), -1), (dict(n=0), -1), (dict(C=0), -1), (dict(C_out=0), -1), (dict(T=0), -1), (dict(H=0), -1),
    (dict(W=-6), -1), (dict(p_t=0), -1), (dict(p_h=-1), -1), (dict(p_w=0), -1), (dict(row=-1), -1), (dict(row=1), -1),
    (dict(n_rows=0), -1),
    (dict(C=9), -2),                                         # C > C_out
    (dict(T=3, p_t=2), -2), (dict(H=5), -2), (dict(W=7), -2),
    (dict(ld_eps=383), -2),                                  # < T*H*W*C_out
    (dict(ld_eps=386), -2),                                  # four channels per eps access
    (dict(eps_u=GOOD + 8), -2), (dict(eps_c=GOOD + 8), -2), (dict(eps_u=GOOD + 4, eps_f16=1), -2),
    (dict(eps_c=GOOD + 4, eps_f16=1), -2),
    (dict(x=GOOD + 4), -2), (dict(hist=GOOD + 4), -2), (dict(x_out=GOOD + 4), -2),        # two elements along w
    (dict(x_model=GOOD + 4), -2), (dict(x_model=GOOD + 2, xm_f16=1), -2),
    (dict(NARROW, eps_u=GOOD + 2), -2), (dict(NARROW, x=GOOD + 2), -2),                  # one element: still its 4 bytes
    (dict(NARROW, eps_c=GOOD + 1, eps_f16=1), -2), (dict(NARROW, x_model=GOOD + 1, xm_f16=1), -2),
    (dict(step=GOOD + 2), -2), (dict(coef=GOOD + 2), -2),
    (dict(T=4, p_t=4, ld_eps=768), -4), (dict(p_h=4), -4), (dict(p_w=3), -4),
    (dict(eps_f16=2), -4), (dict(eps_f16=-1), -4), (dict(xm_f16=3), -4), (dict(xm_copies=0), -4), (dict(xm_copies=3), -4),
    # the order: EINVAL before ESHAPE before EUNSUP
    (dict(eps_u=None, ld_eps=383, eps_f16=2), -1), (dict(row=-1, p_w=3), -1), (dict(ld_eps=383, p_w=3), -2),
    (dict(x=GOOD + 4, xm_copies=3), -2), (dict(H=5, eps_f16=2), -2),
]
# what the entry point takes (VQ_OK would need a GPU, so these are asked of the predicate only)
VALID = [dict(), dict(eps_f16=1), dict(ld_eps=392), dict(eps_u=GOOD + 16, eps_c=GOOD + 8, eps_f16=1), dict(x=GOOD + 8),
         dict(NARROW), dict(NARROW, ld_eps=289, eps_u=GOOD + 4, x=GOOD + 4), dict(NARROW, eps_u=GOOD + 2, eps_f16=1),
         dict(W=5, p_w=1, ld_eps=320, x=GOOD + 4, eps_u=GOOD + 4),       # C == 4 but odd W: one element per access
         dict(T=4, p_t=2, ld_eps=768), dict(n=3), dict(C=4, C_out=4, ld_eps=192)]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    return _lib.load()


def test_entry_point_refusal_table_and_order():
    lib = _lib()
    for kw, code in REFUSALS:
        assert lib.vq_cfg_dpmpp_step_patch(*_args(**kw)) == code, kw


def _fakes(kw):
    a = dict(eps_u=GOOD, eps_c=GOOD, x=GOOD, n=1, C=4, C_out=8, T=2, H=4, W=6, p_t=1, p_h=2, p_w=2, ld_eps=384, eps_f16=0)
    a.update({k: v for k, v in kw.items() if k in a})
    P = max(1, a["p_t"] * a["p_h"] * a["p_w"])
    n, C, T, H, W = a["n"], a["C"], a["T"], a["H"], a["W"]
    dt = {0: torch.float32, 1: torch.float16}.get(a["eps_f16"], torch.bfloat16)
    es, st = (n, T * H * W // P, P * a["C_out"]), (a["ld_eps"], P * a["C_out"], 1)
    x = _FakeTensor((n, C, T, H, W), (C * T * H * W, T * H * W, H * W, W, 1), a["x"], torch.float32)
    return _FakeTensor(es, st, a["eps_u"], dt), _FakeTensor(es, st, a["eps_c"], dt), x, (a["p_t"], a["p_h"], a["p_w"])


def test_ok_predicate_agrees_with_the_entry_point():
    """ops.cfg_dpmpp_step_patch_ok says no exactly where the entry point refuses, on every row of the table that is about
    what the predicate is given (eps_u, eps_c, x, the patch), and yes on the valid layouts."""
    lib = _lib()
    from viditq_amd import ops
    given = {"eps_u", "eps_c", "x", "n", "C", "C_out", "T", "H", "W", "p_t", "p_h", "p_w", "ld_eps", "eps_f16"}
    asked = 0
    for kw, code in REFUSALS:
        if not set(kw) <= given or None in kw.values() or min(v for v in list(kw.values()) + [0]) < 0:
            continue
        assert lib.vq_cfg_dpmpp_step_patch(*_args(**kw)) == code
        assert ops.cfg_dpmpp_step_patch_ok(*_fakes(kw)) is False, kw
        asked += 1
    assert asked >= 24
    for kw in VALID:
        assert ops.cfg_dpmpp_step_patch_ok(*_fakes(kw)) is True, kw
        bad = dict(kw, row=-1)                                # the entry point got past nothing else: only the row is wrong
        assert lib.vq_cfg_dpmpp_step_patch(*_args(**bad)) == -1
        # ... and with a flag out of range as the only fault it reaches the last check: shapes and alignment passed
        assert lib.vq_cfg_dpmpp_step_patch(*_args(**dict(kw, xm_copies=3))) == -4, kw
    u, c, x, p = _fakes({})
    x.dtype = torch.float16
    assert ops.cfg_dpmpp_step_patch_ok(u, c, x, p) is False                      # the latent is fp32
    u, c, x, p = _fakes({})
    c._st = (400, 32, 1)
    assert ops.cfg_dpmpp_step_patch_ok(u, c, x, p) is False                      # one pitch for both outputs
    u, c, x, p = _fakes({})
    u._st = c._st = (384, 1, 12)
    assert ops.cfg_dpmpp_step_patch_ok(u, c, x, p) is False                      # a token's columns are dense
    u, c, x, p = _fakes({})
    u.is_cuda = False
    assert ops.cfg_dpmpp_step_patch_ok(u, c, x, p) is False
    f = lambda *s: torch.zeros(*s)   # noqa: E731
    assert ops.cfg_dpmpp_step_patch_ok(f(1, 12, 32), f(1, 12, 32), f(1, 4, 2, 4, 6), (1, 2, 2)) is False
    with pytest.raises(ops.VQError):
        ops.cfg_dpmpp_step_patch(f(1, 12, 32), f(1, 12, 32), f(1, 4, 2, 4, 6), f(3, 192), f(1, dc.ROW), 0, (1, 2, 2))


def test_symbol_is_declared_and_bound_with_one_signature():
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+vq_cfg_dpmpp_step_patch\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert m, "vq_cfg_dpmpp_step_patch is not declared in include/viditq.h"
    params = [" ".join(q.split()) for q in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", q).group(1) for q in params]
    assert names == ["eps_u", "eps_c", "x", "hist", "coef", "step", "x_out", "x_model", "n", "C", "C_out", "T", "H", "W",
                     "p_t", "p_h", "p_w", "ld_eps", "row", "n_rows", "eps_f16", "xm_f16", "xm_copies", "stream"]
    res, argtypes = _lib.SIGNATURES["vq_cfg_dpmpp_step_patch"]
    kinds = [ctypes.c_void_p if "*" in q else (ctypes.c_long if q.startswith("long") else ctypes.c_int) for q in params]
    assert res is ctypes.c_int and list(argtypes) == kinds
    assert hasattr(_lib.load(), "vq_cfg_dpmpp_step_patch")


# ---------------------------------------------------------------------------------------------------- host logic
def test_cfg_split_runs_two_forwards_of_n_samples_cond_first(gold):
    vd = _sched()
    key = "traj.s3.cfg4."
    z = torch.from_numpy(gold[key + "z"])
    enc = tc.ToyTextEncoder()
    joint, split = [], []
    a = vd.DMP_SOLVER(3, 4.0).sample(tc.AnalyticSTDiT(joint), enc, tc.Z_SIZE, tc.PROMPTS, "cpu", init_noise=z)
    b = vd.DMP_SOLVER(3, 4.0).sample(tc.AnalyticSTDiT(split), enc, tc.Z_SIZE, tc.PROMPTS, "cpu", init_noise=z, cfg_split=True)
    n = len(tc.PROMPTS)
    assert len(joint) == 3 and len(split) == 2 * 3
    y, null = enc.encode(tc.PROMPTS)["y"], enc.null(n)
    for k in range(3):
        (xc, t_c, yc, mc), (xu, t_u, yu, mu) = split[2 * k], split[2 * k + 1]
        assert xc.shape[0] == n and torch.equal(xc, xu) and torch.equal(xc, joint[k][0][:n])
        assert torch.equal(yc, y) and torch.equal(yu, null)                      # cond first, then uncond
        assert torch.equal(t_c, joint[k][1][:n]) and torch.equal(t_u, t_c) and torch.equal(mc, mu)
        assert torch.equal(joint[k][2], torch.cat([null, y]))                    # the joint route: (uncond | cond)
    assert torch.equal(a, b)                                   # a per-sample model: the same numbers either way
    assert np.array_equal(a.numpy(), gold[key + "final"])


def test_timestep_wise_mp_raises_and_names_are_exported():
    import viditq_amd  # noqa: F401
    from viditq_amd import t2v
    assert t2v.DPM_SOLVER is t2v.DMP_SOLVER and callable(t2v.forward_with_dpmsolver)
    net = tc.AnalyticSTDiT()
    net.timestep_wise_mp = True
    with pytest.raises(NotImplementedError):
        t2v.DMP_SOLVER(20, 4.0).sample(net, tc.ToyTextEncoder(), tc.Z_SIZE, tc.PROMPTS, "cpu")
    sig = inspect.signature(t2v.DMP_SOLVER.sample)
    assert list(sig.parameters)[1:] == ["model", "text_encoder", "z_size", "prompts", "device", "additional_args",
                                        "init_noise", "generator", "cfg_split", "fused", "step_callback"]
    assert inspect.signature(t2v.DMP_SOLVER.__init__).parameters["cfg_scale"].default == 4.0
    out = t2v.forward_with_dpmsolver(tc.AnalyticSTDiT(), torch.zeros(2, 4, 2, 4, 6), torch.zeros(2), torch.zeros(2, 1, 3, 4))
    assert tuple(out.shape) == (2, 4, 2, 4, 6)
    from viditq_amd.t2v.stdit import STDiT
    assert inspect.signature(STDiT.forward).parameters["patch_major"].default is False


def test_timestep_id_is_the_hosts_model_input_time():
    """A QuantModel is handed every model-input time as ``timestep_id`` (no forward reads t[0] back)."""
    vd = _sched()
    s = _solver()
    seen = []
    s._takes_id = True
    s.model = lambda x, t, y, **kw: (seen.append((kw.get("timestep_id"), float(t[0]))), tc.analytic_eps(x, t, y)[:, :4])[1]
    s.sample(torch.zeros(2, *tc.Z_SIZE), steps=3, order=2, lower_order_final=vd.lower_order_final(3))
    assert len(seen) == 3 and all(isinstance(i, float) and i == t for i, t in seen)


def test_switch_is_read_once_at_import_and_cpu_tensors_stay_eager(monkeypatch, gold):
    vd = _sched()
    from viditq_amd import ops
    assert vd._T2V_DPM_FUSED == (os.environ.get("VQ_T2V_DPM_FUSED", "0") != "0")
    monkeypatch.setenv("VQ_T2V_DPM_FUSED", "0" if vd._T2V_DPM_FUSED else "1")
    assert vd._T2V_DPM_FUSED == (os.environ["VQ_T2V_DPM_FUSED"] == "0")         # not read again

    def launched(*a, **k):
        raise AssertionError("the fused step was launched")
    monkeypatch.setattr(ops, "cfg_dpmpp_step_patch", launched)
    key = "traj.s3.cfg7."
    got = vd.DMP_SOLVER(3, 7.0).sample(tc.AnalyticSTDiT(), tc.ToyTextEncoder(), tc.Z_SIZE, tc.PROMPTS, "cpu",
                                       init_noise=torch.from_numpy(gold[key + "z"]), fused=True)
    assert np.array_equal(got.numpy(), gold[key + "final"])

"""The table-driven, patch-major DDIM step and the fused STDiT DDIM loop without a GPU: the coefficient table against the
scalars the eager step passes, the entry point's refusals and their order, the predicate against the entry point, the host
model of the step on exactly computable operands, the host logic of the loop."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import fp_edge_cases as fe
import t2v_ddim_cases as dd
import t2v_dpm_cases as tc
from helpers import _FakeTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _iddpm():
    import viditq_amd  # noqa: F401
    from viditq_amd.t2v import iddpm
    return iddpm


# ---------------------------------------------------------------------------------------------------- the table
class _SpyOps:
    """Stands in for ``ops`` inside IDDPM.ddim_step: records the scalars it is passed."""

    def __init__(self):
        self.seen = []

    def cfg_ddim_step(self, cond, uncond, x, cfg, one_plus_k, A, Bc, abar_prev, out=None):
        self.seen.append((cfg, one_plus_k, A, Bc, abar_prev))
        return x


@pytest.mark.parametrize("steps", [2, 20, 100])
@pytest.mark.parametrize("with_ks", [False, True], ids=["no_ks", "ks"])
def test_ddim_rows_equal_the_scalars_of_the_eager_step_bit_for_bit(monkeypatch, steps, with_ks):
    iddpm = _iddpm()
    from viditq_amd import _lib
    d = iddpm.IDDPM(num_sampling_steps=steps, cfg_scale=4.5)
    ks = torch.tensor([(-0.2, 0.0, 0.37, 0.011)[j % 4] for j in range(20)]) if with_ks else None
    rows = d.ddim_rows(d.cfg_scale, ks)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (d.num_timesteps, 16) and d.num_timesteps == steps
    assert (_lib.DDIM_ROW, _lib.DDIM_CFG, _lib.DDIM_ONE_PLUS_K, _lib.DDIM_A, _lib.DDIM_BC, _lib.DDIM_ABAR_PREV,
            _lib.DDIM_T_NEXT) == (dd.ROW, dd.CFG, dd.ONE_PLUS_K, dd.A, dd.BC, dd.ABAR_PREV, dd.T_NEXT)
    spy = _SpyOps()
    monkeypatch.setattr(iddpm, "ops", spy)
    order = list(range(steps))[::-1]
    x = torch.zeros(1, 4, 1)
    for i in order:                                            # what the loop does per step
        t_id = d.timestep_map[i]
        k = 0.0 if ks is None else float(ks[(999 - t_id) // 50])
        d.ddim_step(x, x, x, i, d.cfg_scale, k)
    f32 = lambda v: np.float32(ctypes.c_float(v).value)        # noqa: E731  (the C ABI takes them as float)
    used = {dd.CFG, dd.ONE_PLUS_K, dd.A, dd.BC, dd.ABAR_PREV, dd.T_NEXT}
    for r, i in enumerate(order):
        got = rows[r].numpy()
        want = np.array([f32(v) for v in spy.seen[r]], dtype=np.float32)
        assert np.array_equal(got[[dd.CFG, dd.ONE_PLUS_K, dd.A, dd.BC, dd.ABAR_PREV]].view(np.int32), want.view(np.int32)), r
        nxt = d.timestep_map[order[min(r + 1, steps - 1)]]
        assert got[dd.T_NEXT] == np.float32(nxt) and float(got[dd.T_NEXT]) == nxt
        assert all(got[j] == 0 for j in range(16) if j not in used)
    if with_ks:
        assert len({float(v) for v in rows[:, dd.ONE_PLUS_K]}) > 1
    else:
        assert bool((rows[:, dd.ONE_PLUS_K] == 1).all())
    assert float(rows[0, dd.A]) == float(np.float32(d.sqrt_recip_alphas_cumprod[steps - 1]))     # row 0: the highest t


# ---------------------------------------------------------------------------------------------------- refusals
GOOD = 1 << 20
PTRS = ("eps_c", "eps_u", "x", "coef", "step", "x_out", "x_model", "stream")


def _args(**kw):
    a = dict(eps_c=GOOD, eps_u=GOOD, x=GOOD, coef=GOOD, step=None, x_out=GOOD, x_model=None, n=1, C=4, C_out=8, T=2, H=4,
             W=6, p_t=1, p_h=2, p_w=2, ld_eps=384, guided=3, row=0, n_rows=1, eps_f16=0, xm_f16=0, xm_copies=1, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return [ctypes.c_void_p(v) if k in PTRS and v is not None else v for k, v in a.items()]


NARROW = dict(C=3, C_out=6, ld_eps=288)                      # one element per access
# (arguments on top of a valid base, the code the entry point must return); none of them reaches a HIP call.  The table of
# vq_cfg_dpmpp_step_patch without hist, plus guided.
REFUSALS = [
    (dict(eps_c=None), -1), (dict(eps_u=None), -1), (dict(x=None), -1), (dict(coef=None), -1), (dict(x_out=None), -1),
    (dict(n=0), -1), (dict(C=0), -1), (dict(C_out=0), -1), (dict(T=0), -1), (dict(H=0), -1), (dict(W=-6), -1),
    (dict(p_t=0), -1), (dict(p_h=-1), -1), (dict(p_w=0), -1), (dict(row=-1), -1), (dict(row=1), -1), (dict(n_rows=0), -1),
    (dict(guided=-1), -1),
    (dict(C=9), -2),                                         # C > C_out
    (dict(T=3, p_t=2), -2), (dict(H=5), -2), (dict(W=7), -2),
    (dict(ld_eps=383), -2),                                  # < T*H*W*C_out
    (dict(ld_eps=386), -2),                                  # four channels per eps access
    (dict(eps_u=GOOD + 8), -2), (dict(eps_c=GOOD + 8), -2), (dict(eps_u=GOOD + 4, eps_f16=1), -2),
    (dict(eps_c=GOOD + 4, eps_f16=1), -2),
    (dict(x=GOOD + 4), -2), (dict(x_out=GOOD + 4), -2),      # two elements along w
    (dict(x_model=GOOD + 4), -2), (dict(x_model=GOOD + 2, xm_f16=1), -2),
    (dict(NARROW, eps_u=GOOD + 2), -2), (dict(NARROW, x=GOOD + 2), -2),                  # one element: still its 4 bytes
    (dict(NARROW, eps_c=GOOD + 1, eps_f16=1), -2), (dict(NARROW, x_model=GOOD + 1, xm_f16=1), -2),
    (dict(step=GOOD + 2), -2), (dict(coef=GOOD + 2), -2),
    (dict(T=4, p_t=4, ld_eps=768), -4), (dict(p_h=4), -4), (dict(p_w=3), -4),
    (dict(eps_f16=2), -4), (dict(eps_f16=-1), -4), (dict(xm_f16=3), -4), (dict(xm_copies=0), -4), (dict(xm_copies=3), -4),
    # the order: EINVAL before ESHAPE before EUNSUP
    (dict(eps_u=None, ld_eps=383, eps_f16=2), -1), (dict(row=-1, p_w=3), -1), (dict(ld_eps=383, p_w=3), -2),
    (dict(x=GOOD + 4, xm_copies=3), -2), (dict(H=5, eps_f16=2), -2), (dict(guided=-2, H=5), -1), (dict(guided=-1, p_w=3), -1),
]
VALID = [dict(), dict(eps_f16=1), dict(ld_eps=392), dict(eps_u=GOOD + 16, eps_c=GOOD + 8, eps_f16=1), dict(x=GOOD + 8),
         dict(NARROW), dict(NARROW, ld_eps=289, eps_u=GOOD + 4, x=GOOD + 4), dict(NARROW, eps_u=GOOD + 2, eps_f16=1),
         dict(W=5, p_w=1, ld_eps=320, x=GOOD + 4, eps_u=GOOD + 4),       # C == 4 but odd W: one element per access
         dict(T=4, p_t=2, ld_eps=768), dict(n=3), dict(C=4, C_out=4, ld_eps=192), dict(guided=0), dict(guided=9)]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    return _lib.load()


def test_entry_point_refusal_table_and_order():
    lib = _lib()
    for kw, code in REFUSALS:
        assert lib.vq_cfg_ddim_step_patch(*_args(**kw)) == code, kw


def _fakes(kw):
    a = dict(eps_c=GOOD, eps_u=GOOD, x=GOOD, n=1, C=4, C_out=8, T=2, H=4, W=6, p_t=1, p_h=2, p_w=2, ld_eps=384, eps_f16=0)
    a.update({k: v for k, v in kw.items() if k in a})
    P = max(1, a["p_t"] * a["p_h"] * a["p_w"])
    n, C, T, H, W = a["n"], a["C"], a["T"], a["H"], a["W"]
    dt = {0: torch.float32, 1: torch.float16}.get(a["eps_f16"], torch.bfloat16)
    es, st = (n, T * H * W // P, P * a["C_out"]), (a["ld_eps"], P * a["C_out"], 1)
    x = _FakeTensor((n, C, T, H, W), (C * T * H * W, T * H * W, H * W, W, 1), a["x"], torch.float32)
    return _FakeTensor(es, st, a["eps_c"], dt), _FakeTensor(es, st, a["eps_u"], dt), x, (a["p_t"], a["p_h"], a["p_w"])


def test_ok_predicate_agrees_with_the_entry_point():
    """ops.cfg_ddim_step_patch_ok says no exactly where the entry point refuses, on every row of the table that is about
    what the predicate is given (eps_c, eps_u, x, the patch), and yes on the valid layouts."""
    lib = _lib()
    from viditq_amd import ops
    given = {"eps_u", "eps_c", "x", "n", "C", "C_out", "T", "H", "W", "p_t", "p_h", "p_w", "ld_eps", "eps_f16"}
    asked = 0
    for kw, code in REFUSALS:
        if not set(kw) <= given or None in kw.values() or min(v for v in list(kw.values()) + [0]) < 0:
            continue
        assert lib.vq_cfg_ddim_step_patch(*_args(**kw)) == code
        assert ops.cfg_ddim_step_patch_ok(*_fakes(kw)) is False, kw
        asked += 1
    assert asked >= 24
    for kw in VALID:
        assert ops.cfg_ddim_step_patch_ok(*_fakes(kw)) is True, kw
        assert lib.vq_cfg_ddim_step_patch(*_args(**dict(kw, row=-1))) == -1          # only the row is wrong
        # with a flag out of range as the only fault it reaches the last check: shapes and alignment passed
        assert lib.vq_cfg_ddim_step_patch(*_args(**dict(kw, xm_copies=3))) == -4, kw
    c, u, x, p = _fakes({})
    x.dtype = torch.float16
    assert ops.cfg_ddim_step_patch_ok(c, u, x, p) is False                       # the latent is fp32
    c, u, x, p = _fakes({})
    u._st = (400, 32, 1)
    assert ops.cfg_ddim_step_patch_ok(c, u, x, p) is False                       # one pitch for both outputs
    c, u, x, p = _fakes({})
    c.is_cuda = False
    assert ops.cfg_ddim_step_patch_ok(c, u, x, p) is False
    f = lambda *s: torch.zeros(*s)   # noqa: E731
    assert ops.cfg_ddim_step_patch_ok(f(1, 12, 32), f(1, 12, 32), f(1, 4, 2, 4, 6), (1, 2, 2)) is False
    with pytest.raises(ops.VQError):
        ops.cfg_ddim_step_patch(f(1, 12, 32), f(1, 12, 32), f(1, 4, 2, 4, 6), f(1, dd.ROW), 0, (1, 2, 2))
    # one geometry helper behind both patch-major predicates
    assert ops.cfg_dpmpp_step_patch_ok.__code__.co_names == ops.cfg_ddim_step_patch_ok.__code__.co_names == ("_patch_ok",)


def test_symbol_is_declared_and_bound_with_one_signature():
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "viditq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+vq_cfg_ddim_step_patch\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert m, "vq_cfg_ddim_step_patch is not declared in include/viditq.h"
    params = [" ".join(q.split()) for q in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", q).group(1) for q in params]
    assert names == ["eps_c", "eps_u", "x", "coef", "step", "x_out", "x_model", "n", "C", "C_out", "T", "H", "W", "p_t",
                     "p_h", "p_w", "ld_eps", "guided", "row", "n_rows", "eps_f16", "xm_f16", "xm_copies", "stream"]
    res, argtypes = _lib.SIGNATURES["vq_cfg_ddim_step_patch"]
    kinds = [ctypes.c_void_p if "*" in q else (ctypes.c_long if q.startswith("long") else ctypes.c_int) for q in params]
    assert res is ctypes.c_int and list(argtypes) == kinds
    assert hasattr(_lib.load(), "vq_cfg_ddim_step_patch")
    for name, val in (("ROW", 16), ("CFG", 0), ("ONE_PLUS_K", 1), ("A", 2), ("BC", 3), ("ABAR_PREV", 4), ("T_NEXT", 14)):
        assert re.search(r"#define\s+VQ_DDIM_%s\s+%d\b" % (name, val), src), name


# ---------------------------------------------------------------------------------------------------- the host model
@pytest.mark.parametrize("shape", tc.SHAPES[:5], ids=tc.shape_id)
def test_host_model_is_exact_on_the_s1_operands(shape):
    """Through the index map the S1 operands give the dense S1 case back; its fp64 evaluation is exact and contraction
    cannot change it (fp_edge_cases.s1_prove), for guidance on 0, 3 and all channels; every mutant moves the result."""
    n, C, Co, T, H, W, patch, _ = shape
    for pi in (0, 17, 40, len(fe.S1_PARAMS) - 1):
        params = fe.S1_PARAMS[pi]
        pm_c, pm_u, x, s = dd.s1_patch(shape, params)
        assert bool(torch.isnan(pm_c).any()) and bool(torch.isnan(pm_u).any())      # the sigma channels
        got = dd.scase_of(pm_c, pm_u, x, params, patch, Co)
        for a, b in ((got.cond, s.cond), (got.uncond, s.uncond), (got.x, s.x)):
            assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
        fe.s1_prove(got)
        exact = dd.reference_step_patch(pm_c, pm_u, x, params, patch, Co)
        assert torch.equal(exact, s.exact.reshape(x.shape)) and bool(torch.isfinite(exact).all())
        assert torch.equal(dd.reference_step_patch(pm_c, pm_u, x, params, patch, Co, dtype=torch.float32).double(), exact)
        g0 = dd.reference_step_patch(pm_c, pm_u, x, params, patch, Co, guided=0)
        gC = dd.reference_step_patch(pm_c, pm_u, x, params, patch, Co, guided=C)
        assert torch.equal(gC, dd.reference_step_patch(pm_c, pm_u, x, params, patch, Co, mutant="cfg_all_channels"))
        assert torch.equal(g0[:, 3:], exact[:, 3:]) and torch.equal(gC[:, :3], exact[:, :3])
        assert not torch.equal(g0[:, :3], exact[:, :3])
        for q in (g0, gC):                                     # exact too: every value a multiple of 2^-10 below 2^13
            assert torch.equal(q * 1024, (q * 1024).round()) and float(q.abs().max()) < 2.0 ** 13


def test_every_mutant_is_caught_by_the_host_model():
    params = fe.S1_PARAMS[40]
    assert params[1] == 2.0                                    # 1 + k != 1, or a skipped division would not show
    small, big = tc.SHAPES[1], tc.SHAPES[5]
    assert small[6] == (1, 2, 2) and small[1] == 4             # a 2 x 2 patch and a fourth, unguided channel
    pm_c, pm_u, x, s = dd.s1_patch(small, params)
    exact = s.exact.reshape(x.shape)
    for m in dd.MUTANTS:
        if dd.MUTANT_FAMILY[m] == "S1":
            bad = dd.reference_step_patch(pm_c, pm_u, x, params, small[6], small[2], mutant=m)
            assert not torch.equal(bad, exact), m
    # the S3 mutant needs a latent the first pass of the grid does not cover
    assert dd._item_index(*[big[i] for i in (0, 1, 3, 4, 5)]).max() < dd.FIRST_PASS_ITEMS
    for shape in tc.SHAPES[6:]:
        dims = [shape[i] for i in (0, 1, 3, 4, 5)]
        assert dd._item_index(*dims).max() >= dd.FIRST_PASS_ITEMS, shape


# ---------------------------------------------------------------------------------------------------- host logic
def _loop(fused, split, calls=None, seen=None, ks=None, steps=4, net=None):
    iddpm = _iddpm()
    enc = tc.ToyTextEncoder()
    net = net or tc.AnalyticSTDiT(calls)
    net.cfg_split = split
    n = len(tc.PROMPTS)
    args = dict(y=torch.cat([enc.encode(tc.PROMPTS)["y"], enc.null(n)]), mask=enc.encode(tc.PROMPTS)["mask"])
    g = torch.Generator().manual_seed(3)
    z = torch.randn(n, *tc.Z_SIZE, generator=g)
    cb = None if seen is None else (lambda i, v: seen.append((i, v.clone())))
    return iddpm.IDDPM(num_sampling_steps=steps, cfg_scale=4.0).ddim_sample_loop(net, z, args, ks=ks, step_callback=cb,
                                                                                 fused=fused)


@pytest.mark.parametrize("split", [False, True], ids=["joint", "split"])
def test_fused_on_cpu_tensors_is_the_eager_loop(monkeypatch, split):
    """No launch, the same bits step by step, the same number of forwards."""
    from viditq_amd import ops
    launched = []
    monkeypatch.setattr(ops, "cfg_ddim_step_patch", lambda *a, **k: launched.append(1))
    real = ops.cfg_ddim_step

    def cpu_step(cond, uncond, x, cfg, opk, A, Bc, abp, out=None):
        """The dense step on the host (this test is about the loop, which must not care where the step runs)."""
        n, C = x.shape[:2]
        s = fe.SCase("", "", "", n, C, x[0, 0].numel(), cond.reshape(n, 2 * C, -1), uncond.reshape(n, 2 * C, -1),
                     x.reshape(n, C, -1), cfg, opk, A, Bc, abp)
        return fe.sampler_reference(s, dtype=torch.float32).reshape(x.shape)

    monkeypatch.setattr(ops, "cfg_ddim_step", cpu_step)
    ks = torch.tensor([0.25] * 20)
    ce, cf, se, sf = [], [], [], []
    want = _loop(False, split, ce, se, ks)
    got = _loop(True, split, cf, sf, ks)
    assert real is not cpu_step and not launched
    assert torch.equal(got, want) and len(cf) == len(ce) == 4 * (2 if split else 1)
    assert [i for i, _ in sf] == [i for i, _ in se] == [3, 2, 1, 0]
    assert all(torch.equal(a[1], b[1]) for a, b in zip(se, sf))
    for a, b in zip(ce, cf):
        assert all(torch.equal(p, q) for p, q in zip(a[:3], b[:3]))


def test_switch_is_read_once_at_import(monkeypatch):
    iddpm = _iddpm()
    assert iddpm._T2V_DDIM_FUSED == (os.environ.get("VQ_T2V_DDIM_FUSED", "0") != "0")
    monkeypatch.setenv("VQ_T2V_DDIM_FUSED", "0" if iddpm._T2V_DDIM_FUSED else "1")
    assert iddpm._T2V_DDIM_FUSED == (os.environ["VQ_T2V_DDIM_FUSED"] == "0")         # not read again
    sig = inspect.signature(iddpm.IDDPM.ddim_sample_loop)
    assert sig.parameters["fused"].default is None and sig.parameters["graphed"].default is False
    assert inspect.signature(iddpm.IDDPM.sample).parameters["fused"].default is None
    assert list(inspect.signature(iddpm.IDDPM.step_graph).parameters)[1:] == ["model", "x", "model_args", "ks", "warmup"]


def test_patch_major_is_asked_of_the_model_not_assumed():
    iddpm = _iddpm()

    class Plain:
        def forward(self, x, timestep, y, mask=None):
            return x

    assert iddpm.takes_patch_major(tc.AnalyticSTDiT()) is True and iddpm.takes_patch_major(Plain()) is False


def test_one_helper_makes_the_patch_major_forwards_of_both_schedulers():
    import viditq_amd  # noqa: F401
    from viditq_amd.t2v import dpm_solver, iddpm
    assert dpm_solver.patch_forward_pair is iddpm.patch_forward_pair
    for fn in (dpm_solver.VideoDPMSolverPP._forward_patch, iddpm.IDDPM._ddim_fused):
        src = inspect.getsource(fn)
        assert "patch_forward_pair(" in src and "patch_major" not in src.split('"""')[2], fn.__qualname__
    calls = []
    net = tc.AnalyticSTDiT(calls)
    enc = tc.ToyTextEncoder()
    y, null = enc.encode(tc.PROMPTS)["y"], enc.null(2)
    x, t = torch.zeros(2, *tc.Z_SIZE), torch.full((2,), 7.0)
    a, b = iddpm.patch_forward_pair(net, x, t, (y, null), True, dict(mask=None))
    assert torch.equal(calls[0][2], y) and torch.equal(calls[1][2], null) and a.shape == b.shape == (2, 2 * 2 * 3, 4 * 8)
    j0, j1 = iddpm.patch_forward_pair(net, torch.cat([x, x]), torch.cat([t, t]), torch.cat([y, null]), False, dict(mask=None))
    assert len(calls) == 3 and torch.equal(j0, a) and torch.equal(j1, b)


def test_step_graph_refuses_timestep_wise_mp():
    iddpm = _iddpm()
    from viditq_amd import ops
    net = tc.AnalyticSTDiT()
    net.timestep_wise_mp = True
    with pytest.raises(ops.VQError, match="timestep_wise_mp"):
        iddpm.IDDPM(num_sampling_steps=4).step_graph(net, torch.zeros(2, *tc.Z_SIZE), dict(y=torch.zeros(4, 1, 3, 4)))

"""The patch-major DDIM step and the fused STDiT DDIM loops on the GPU (vq_cfg_ddim_step_patch, ops.cfg_ddim_step_patch,
IDDPM.ddim_sample_loop(fused=True), graph.VideoDDIMStepGraph): the kernel against vq_cfg_ddim_step on the unpatchified
fp32 tensor bit for bit, the exactly computable cases per element, NaN in everything it must not read and canaries around
everything it writes, the counter form, fused loops against eager ones step by step, the one-graph step, the fallbacks."""
import itertools

import pytest
import torch

import dpm_step_cases as dc
import fp_edge_cases as fe
import t2v_ddim_cases as dd
import t2v_dpm_cases as tc
from helpers import FP_LAYERS, Arena, load_npz

pytestmark = pytest.mark.gpu


def _calls():
    from viditq_amd import _lib
    return _lib.CALLS[0]


def _iddpm(steps, cfg=4.0):
    from viditq_amd.t2v import IDDPM
    return IDDPM(num_sampling_steps=steps, cfg_scale=cfg)


@pytest.fixture(scope="module")
def rows6():
    """Six rows: both ends and the middle of a real 100-step table, and three of a table that carries 1 + k from
    {0.8, 1, 1.37}."""
    ks = torch.tensor([(-0.2, 0.0, 0.37)[j % 3] for j in range(20)], dtype=torch.float64)
    d = _iddpm(100, 4.0)
    plain, ptqd = d.ddim_rows(4.0), d.ddim_rows(7.5, ks)
    rows = torch.stack([plain[0], plain[50], plain[99], ptqd[3], ptqd[41], ptqd[97]])
    assert sorted(round(float(v), 2) for v in rows[3:, dd.ONE_PLUS_K]) == [0.8, 1.0, 1.37]
    return rows


_INS = {}


def _inputs(shape):
    """Seeded CPU operands of one shape, made once: the full model output [2n, C_out, T, H, W], cond first
    (fp16-representable, so that both storage types hold the same numbers), and x."""
    if shape not in _INS:
        n, C, Co, T, H, W, patch, pad = shape
        g = torch.Generator().manual_seed(sum(shape[:6]))
        _INS[shape] = (torch.randn(2 * n, Co, T, H, W, generator=g).half().float(), torch.randn(n, C, T, H, W, generator=g))
    return _INS[shape]


def launch(ops, dev, shape, full, x, rows, k, half, joint, copies, alias, xm_half, guided=3, counter=None):
    """One launch of row k inside NaN arenas: NaN in the sigma channels, the pitch padding and (split) nothing shared
    between the halves; canaries around x_out and x_model.  ``full``: [2n, C_out, T, H, W], cond | uncond.  Returns x_out
    after the checks on everything but its values."""
    n, C, Co, T, H, W, patch, pad = shape
    et = torch.float16 if half else torch.float32
    total = x.numel()
    full = full.clone()
    full[:, C:] = float("nan")                                # the learned-sigma channels: never read
    pm = tc.patchify(full, patch)                             # [2n, tokens, columns]
    dense = pm.shape[1] * pm.shape[2]
    ld = dense + pad
    if joint:
        A_e = [Arena(dev, 2 * n * ld, et)]
        views = [A_e[0].t.view(2 * n, ld)[:n], A_e[0].t.view(2 * n, ld)[n:]]
    else:                                                     # two buffers: each half is surrounded by NaN only
        A_e = [Arena(dev, n * ld, et), Arena(dev, n * ld, et)]
        views = [a.t.view(n, ld) for a in A_e]
    for v, src in zip(views, (pm[:n], pm[n:])):               # the pitch padding stays NaN
        v[:, :dense] = src.reshape(n, dense).to(dev).to(et)
    eps_c, eps_u = (v[:, :dense].unflatten(1, (pm.shape[1], pm.shape[2])) for v in views)
    A_x = Arena(dev, total, torch.float32)
    A_o = A_x if alias else Arena(dev, total, torch.float32)
    mt = torch.float16 if xm_half else torch.float32
    A_m = Arena(dev, copies * total, mt)
    A_x.t.copy_(x.reshape(-1))
    x_t = A_x.t.view(n, C, T, H, W)
    arenas = A_e + [A_x, A_m] + ([] if alias else [A_o])
    for a in arenas:
        a.snapshot()
    assert ops.cfg_ddim_step_patch_ok(eps_c, eps_u, x_t, patch)
    assert eps_c.stride(0) == ld and (not joint or eps_u.data_ptr() == eps_c.data_ptr() + n * ld * eps_c.element_size())
    step = None if counter is None else torch.tensor([counter], dtype=torch.int32, device=dev)
    got = ops.cfg_ddim_step_patch(eps_c, eps_u, x_t, rows.to(dev), k if counter is None else 0, patch, step=step,
                                  x_out=A_o.t.view(n, C, T, H, W), x_model=A_m.t.view(copies * n, C, T, H, W), guided=guided)
    torch.cuda.synchronize()
    tag = (tc.shape_id(shape), k, half, joint, copies, alias, xm_half, guided)
    assert got.data_ptr() == A_o.t.data_ptr()
    assert bool(torch.isfinite(got).all()), tag
    cast = got.to(mt).reshape(-1)
    for q in range(copies):
        assert torch.equal(A_m.t[q * total:(q + 1) * total], cast), (tag, "x_model", q)
    for a in A_e:
        assert a.unchanged(), (tag, "eps written")
    assert A_o.unchanged(0, total), (tag, "written outside x_out")
    assert A_m.unchanged(0, copies * total), (tag, "written outside x_model")
    if not alias:
        assert A_x.unchanged(), (tag, "x written")
    return got, tag


def dense_step(ops, dev, shape, full, x, rows, k):
    """The two launches the kernel replaces: the unpatchified fp32 tensor through ops.cfg_ddim_step."""
    n = shape[0]
    cond, unc = full[:n].contiguous().to(dev), full[n:].contiguous().to(dev)
    return ops.cfg_ddim_step(cond, unc, x.to(dev), *dd.params_of(rows[k]))


# ---------------------------------------------------------------------------------------------------- 1, 3
@pytest.mark.parametrize("shape", tc.SHAPES, ids=tc.shape_id)
def test_patch_kernel_equals_the_dense_kernel_bit_for_bit(ops, dev, rows6, shape):
    """Six rows x fp16 / fp32 storage x joint / split pointers x xm_copies 1 / 2 x x_out aliasing x: every combination
    on the small shapes, each value of each axis (rotating) on the three large ones.  Reads and writes are checked in every
    launch (``launch``)."""
    full, x = _inputs(shape)
    small = x.numel() < 100000
    combos = list(itertools.product(range(6), (True, False), (True, False), (1, 2), (False, True)))
    if not small:
        combos = [c for i, c in enumerate(combos) if i % 11 == 0]       # 9 of 96
        assert {c[0] for c in combos} == set(range(6))
        assert all({c[j] for c in combos} == {True, False} for j in (1, 2, 4)) and {c[3] for c in combos} == {1, 2}
    want = {}
    for i, (k, half, joint, copies, alias) in enumerate(combos):
        if k not in want:
            want[k] = dense_step(ops, dev, shape, full, x, rows6, k)
        got, tag = launch(ops, dev, shape, full, x, rows6, k, half, joint, copies, alias, xm_half=bool((i + k) & 1))
        assert torch.equal(got, want[k]), (tag, int((got != want[k]).sum()), float((got - want[k]).abs().max()))


_S1 = {}


def _s1(shape, pi):
    if (shape, pi) not in _S1:
        _S1[(shape, pi)] = dd.s1_patch(shape, fe.S1_PARAMS[pi])
    return _S1[(shape, pi)]


@pytest.mark.parametrize("shape", tc.SHAPES, ids=tc.shape_id)
def test_guided_channel_counts_against_the_exact_model(ops, dev, shape):
    """guided in {0, 3, C, C + 5} on the S1 operands against the fp64-exact host model (the dense entry point fixes 3)."""
    n, C, Co, T, H, W, patch, pad = shape
    small = n * C * T * H * W < 100000
    for j, pi in enumerate((40, 17, 65) if small else (40,)):
        params = fe.S1_PARAMS[pi]
        pm_c, pm_u, x, s = _s1(shape, pi)
        full = torch.cat([s.cond.reshape(n, Co, T, H, W), s.uncond.reshape(n, Co, T, H, W)])
        rows = dd.rows_of([params])
        for i, guided in enumerate((0, 3, C, C + 5)):
            exact = dd.reference_step_patch(pm_c, pm_u, x, params, patch, Co, guided=min(guided, C))
            got, tag = launch(ops, dev, shape, full, x, rows, 0, bool((i + j) & 1), bool(i & 2), 1 + (i & 1), bool(j & 1),
                              bool(i & 1), guided=guided)
            assert torch.equal(got.cpu().double(), exact), (tag, pi)


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("shape", tc.SHAPES, ids=tc.shape_id)
def test_exact_cases_per_element_and_their_mutants(ops, dev, shape):
    """S1 (small shapes) / S3 (the shapes a single pass does not cover) operands through the entry point against the
    fp64-exact reference, bit for bit per element; each mutant that applies is first shown to move the host model."""
    n, C, Co, T, H, W, patch, pad = shape
    second_pass = dd._item_index(n, C, T, H, W).max() >= dd.FIRST_PASS_ITEMS
    pi = 40
    params = fe.S1_PARAMS[pi]
    pm_c, pm_u, x, s = _s1(shape, pi)
    exact = s.exact.reshape(x.shape)
    caught = []
    for m in dd.MUTANTS:
        if m == "second_pass_missing" and not second_pass:
            continue
        if m == "hw_swapped" and patch[1] * patch[2] == 1:
            continue
        if m == "cfg_all_channels" and C <= 3:
            continue
        assert not torch.equal(dd.reference_step_patch(pm_c, pm_u, x, params, patch, Co, mutant=m), exact), m
        caught.append(m)
    assert len(caught) >= 3 and (not second_pass or "second_pass_missing" in caught)
    full = torch.cat([s.cond.reshape(n, Co, T, H, W), s.uncond.reshape(n, Co, T, H, W)])
    for half, joint in ((False, True), (True, False)):
        got, tag = launch(ops, dev, shape, full, x, dd.rows_of([params]), 0, half, joint, 2 if joint else 1, False, half)
        bad = got.cpu().double() != exact
        assert not bool(bad.any()), (tag, int(bad.sum()), bad.nonzero()[0].tolist())
    # and the dense entry point on the same operands (what test 1 compares against) gives the same exact values
    assert torch.equal(dense_step(ops, dev, shape, full, x, dd.rows_of([params]), 0).cpu().double(), exact)


# ---------------------------------------------------------------------------------------------------- 4
def test_counter_form_equals_explicit_rows_and_advance_moves_it(ops, dev, rows6):
    shape = tc.SHAPES[1]
    full, x = _inputs(shape)
    for k in (0, 2, 5):
        want = dense_step(ops, dev, shape, full, x, rows6, k)
        got, tag = launch(ops, dev, shape, full, x, rows6, k, True, True, 2, False, True, counter=k)
        assert torch.equal(got, want), tag
    got, tag = launch(ops, dev, shape, full, x, rows6, 5, False, False, 1, True, False, counter=5 + 6)
    assert torch.equal(got, dense_step(ops, dev, shape, full, x, rows6, 5)), "a counter beyond the table reads the last row"
    rows = rows6.clone()
    rows[:, dd.T_NEXT] = torch.tensor([900.0, 800.0, 700.0, 600.0, 500.0, 500.0])
    rows_d = rows.to(dev)
    step = torch.tensor([3], dtype=torch.int32, device=dev)
    t = torch.zeros(4, dtype=torch.float32, device=dev)
    ops.dpmpp_advance(step, rows_d, t)
    assert int(step) == 4 and t.tolist() == [600.0] * 4
    ops.dpmpp_advance(step, rows_d, t)
    ops.dpmpp_advance(step, rows_d, t)
    assert int(step) == 5 and t.tolist() == [500.0] * 4                    # saturates on the last row


# ---------------------------------------------------------------------------------------------------- 5
def _args(dev, n=2):
    enc = tc.ToyTextEncoder(dev)
    e = enc.encode(tc.PROMPTS[:n])
    return dict(y=torch.cat([e["y"], enc.null(n)]), mask=e["mask"])


KS = torch.tensor([(0.37, -0.2, 0.0, 0.011)[j % 4] for j in range(20)], dtype=torch.float64)


def _loop(sampler, net, z, args, fused, seen=None, ks=KS):
    cb = None if seen is None else (lambda i, v: seen.append((i, v.clone())))
    return sampler.ddim_sample_loop(net, z.clone(), args, ks=ks, step_callback=cb, fused=fused)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16model", "fp32model"])
@pytest.mark.parametrize("split", [False, True], ids=["joint", "split"])
def test_analytic_model_fused_graph_and_eager_agree_step_by_step(ops, dev, split, dtype):
    z = torch.from_numpy(dc.gauss((2,) + tc.Z_SIZE, 41)).to(dev)
    z2 = torch.from_numpy(dc.gauss((2,) + tc.Z_SIZE, 43)).to(dev)
    args = _args(dev)
    for steps in (2, 20):
        d = _iddpm(steps, 4.0)
        ce, cf, se, sf, sg = [], [], [], [], []
        ne, nf = tc.AnalyticSTDiT(ce, dtype), tc.AnalyticSTDiT(cf, dtype)
        ne.cfg_split = nf.cfg_split = split
        want = _loop(d, ne, z, args, False, se)
        n0 = _calls()
        got = _loop(d, nf, z, args, True, sf)
        assert _calls() - n0 == steps                          # one C-ABI launch per step
        assert torch.equal(got, want), (steps, float((got - want).abs().max()))
        assert len(cf) == len(ce) == steps * (2 if split else 1)
        for a, b in zip(ce, cf):                               # every model input: the sample (in the model's type), time, text
            assert torch.equal(a[0].to(dtype), b[0].to(dtype)) and torch.equal(a[1].float(), b[1].float())
            assert torch.equal(a[2], b[2])
        assert [i for i, _ in sf] == [i for i, _ in se] == list(range(steps))[::-1]
        assert all(torch.equal(a[1], b[1]) for a, b in zip(se, sf))
        net = tc.AnalyticSTDiT(None, dtype)
        net.cfg_split = split
        graph = d.step_graph(net, z, args, ks=KS)
        assert len(graph.graphs) == 1 and graph.xm.shape[0] == (2 if split else 4) and graph.xm.dtype == dtype
        assert int(graph.step) == 0 and bool((graph.t == graph.t_first).all()) and torch.equal(graph.x, z)
        out = graph.run(z, step_callback=lambda i, v: sg.append((i, v)))
        assert torch.equal(out, want)
        assert [i for i, _ in sg] == [i for i, _ in se] and all(torch.equal(a[1], b[1]) for a, b in zip(se, sg))
        assert torch.equal(graph.run(z2), _loop(d, ne, z2, args, False))        # another start latent: run() resets
        assert torch.equal(graph.run(z), want)


class _GoldText:
    """The text side of the tiny STDiT goldens: row 0 of ``y`` is the prompt, row 1 the null prompt."""

    def __init__(self, g, dev):
        self.args = dict(y=g["y"].half().to(dev)[:2].clone(), mask=g["mask"].to(dev)[:1].clone())


def _tiny(dev):
    from test_model_gpu import _build
    g = load_npz("tiny_stdit_w4a8.npz")
    qnn = _build(g, dev, 4, smooth=dict(alpha=[0.11, 0.11], timerange=[[0, 500], [501, 1000]]), mixed_precision=[4, 6, 8])
    qnn.set_layer_smooth_quant(model=qnn, module_name_list=FP_LAYERS, smooth_quant=False, smooth_quant_running_stat=False)
    return g, qnn


@pytest.mark.parametrize("split", [False, True], ids=["joint", "split"])
def test_tiny_stdit_time_range_plan_fused_graph_and_eager_agree(ops, dev, split):
    """The tiny STDiT behind a QuantModel, W4A8 with two smooth-quant time ranges, 20 steps (t crosses 500 halfway): today's
    eager loop, the eager-launched fused loop and VideoDDIMStepGraph - one capture per visited range, both taken before
    the first replay - give the same bits, step by step."""
    g, qnn = _tiny(dev)
    qnn.cfg_split = split
    args = _GoldText(g, dev).args
    z = torch.from_numpy(dc.gauss((1, 4, 4, 8, 8), 43)).to(dev)
    d = _iddpm(20, 4.0)
    se, sf, sg = [], [], []
    want = _loop(d, qnn, z, args, False, se)
    got = _loop(d, qnn, z, args, True, sf)
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)
    assert len(sf) == 20 and all(i == j and torch.equal(a, b) for (i, a), (j, b) in zip(se, sf))
    graph = d.step_graph(qnn, z, args, ks=KS)
    t_ids = [d.timestep_map[i] for i in range(20)][::-1]
    assert sorted(graph.graphs) == [0, 1] and graph.range_of == [0 if t <= 500 else 1 for t in t_ids]
    assert graph.range_of[0] == 1 and graph.range_of[-1] == 0
    out = graph.run(z, step_callback=lambda i, v: sg.append((i, v)))
    assert torch.equal(out, want), float((out - want).abs().max())
    assert all(i == j and torch.equal(a, b) for (i, a), (j, b) in zip(se, sg)) and len(sg) == 20
    assert torch.equal(graph.run(z), want)


# ---------------------------------------------------------------------------------------------------- 6
class _NoPatchMajor(tc.AnalyticSTDiT):
    def forward(self, x, timestep, y, mask=None):
        return super().forward(x, timestep, y, mask=mask)


class _Misaligned(tc.AnalyticSTDiT):
    """Its patch-major output is a view one element into a larger buffer: the 4-channel reads are not aligned."""

    def forward(self, x, timestep, y, mask=None, patch_major=False):
        out = super().forward(x, timestep, y, mask=mask, patch_major=patch_major)
        if not patch_major:
            return out
        buf = torch.empty(out.numel() + 1, dtype=out.dtype, device=out.device)
        buf[1:].copy_(out.reshape(-1))
        return buf[1:].view(out.shape)


@pytest.mark.parametrize("split", [False, True], ids=["joint", "split"])
def test_fallbacks_are_taken_and_cost_no_forward(ops, dev, monkeypatch, split):
    n_launch = [0]
    orig = ops.cfg_ddim_step_patch

    def counted(*a, **k):
        n_launch[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(ops, "cfg_ddim_step_patch", counted)
    z = torch.from_numpy(dc.gauss((2,) + tc.Z_SIZE, 53)).to(dev)
    args = _args(dev)
    d = _iddpm(3, 4.0)
    ref_calls = []
    ref_net = tc.AnalyticSTDiT(ref_calls, torch.float16)
    ref_net.cfg_split = split
    want = _loop(d, ref_net, z, args, False)
    for cls in (_NoPatchMajor, _Misaligned):
        calls = []
        net = cls(calls, torch.float16)
        net.cfg_split = split
        got = _loop(d, net, z, args, True)
        assert torch.equal(got, want), cls.__name__
        assert len(calls) == len(ref_calls) == 3 * (2 if split else 1), cls.__name__
    assert n_launch[0] == 0
    net = tc.AnalyticSTDiT(None, torch.float16)
    net.cfg_split = split
    assert torch.equal(_loop(d, net, z, args, True), want) and n_launch[0] == 3
    assert torch.equal(_loop(d, net, z, args, False), want) and n_launch[0] == 3

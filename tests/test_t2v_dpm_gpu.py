"""The patch-major DPM-Solver++ step and the STDiT DPM-Solver++ loops on the GPU (vq_cfg_dpmpp_step_patch,
ops.cfg_dpmpp_step_patch, t2v.DMP_SOLVER(fused=True), graph.VideoDPMStepGraph): the kernel against vq_cfg_dpmpp_step on
the unpatchified fp32 tensor bit for bit, NaN in everything it must not read and canaries around everything it writes,
the counter form, fused loops against eager ones step by step, the one-graph step, the fallbacks."""
import itertools

import pytest
import torch

import dpm_step_cases as dc
import t2v_dpm_cases as tc
from helpers import FP_LAYERS, Arena, load_npz

pytestmark = pytest.mark.gpu

KINDS = [(1, "dpmsolver"), (2, "dpmsolver"), (3, "dpmsolver"), (2, "taylor")]


def _calls():
    from viditq_amd import _lib
    return _lib.CALLS[0]


@pytest.fixture(scope="module")
def rows20():
    """[(order, solver type) -> a real 20-step table that has a row of that order at k = 7]."""
    s = dc.make_solver(4.5)
    return {(o, st): s.multistep_rows(20, o, "time_uniform", None, None, False, st) for o, st in KINDS}


def _inputs(shape, seed):
    """Seeded CPU operands of one shape, made once per shape: the full model output [2n, C_out, T, H, W] (fp16-representable,
    so that both storage types hold the same numbers), x, and three history slots."""
    n, C, Co, T, H, W, patch, pad = shape
    g = torch.Generator().manual_seed(seed)
    full = torch.randn(2 * n, Co, T, H, W, generator=g).half().float()
    x = torch.randn(n, C, T, H, W, generator=g)
    hist = torch.randn(3, x.numel(), generator=g)
    return full, x, hist


def run_case(ops, dev, shape, ins, rows, k, half, joint, copies, alias, xm_half, counter=None):
    """One launch of row k inside NaN arenas against ops.cfg_dpmpp_step on the unpatchified fp32 tensor."""
    n, C, Co, T, H, W, patch, pad = shape
    full, x, hist = ins
    order = int(rows[k][dc.ORDER])
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
    else:
        A_e = [Arena(dev, n * ld, et), Arena(dev, n * ld, et)]
        views = [a.t.view(n, ld) for a in A_e]
    for v, src in zip(views, (pm[:n], pm[n:])):               # the pitch padding stays NaN
        v[:, :dense] = src.reshape(n, dense).to(dev).to(et)
    eps_u, eps_c = (v[:, :dense].unflatten(1, (pm.shape[1], pm.shape[2])) for v in views)
    h = hist.clone()
    for j in range(order, 3):                                 # the slots an update of this order does not read
        h[(k - j) % 3] = float("nan")
    A_x, A_h = Arena(dev, total, torch.float32), Arena(dev, 3 * total, torch.float32)
    A_o = A_x if alias else Arena(dev, total, torch.float32)
    mt = torch.float16 if xm_half else torch.float32
    A_m = Arena(dev, copies * total, mt)
    A_x.t.copy_(x.reshape(-1))
    A_h.t.copy_(h.reshape(-1))
    coef = rows.to(dev)
    x_t = A_x.t.view(n, C, T, H, W)
    # the sibling on the unpatchified fp32 tensor (made before the launch: x may be overwritten)
    ref_eps = full[:, :C].contiguous().to(dev)
    h_ref = A_h.t.view(3, total).clone()
    want = ops.cfg_dpmpp_step(ref_eps, x_t.clone(), h_ref, coef, k)
    arenas = A_e + [A_x, A_h, A_m] + ([] if alias else [A_o])
    for a in arenas:
        a.snapshot()
    assert ops.cfg_dpmpp_step_patch_ok(eps_u, eps_c, x_t, patch)
    assert eps_u.stride(0) == ld and (not joint or eps_c.data_ptr() == eps_u.data_ptr() + n * ld * eps_u.element_size())
    step = None if counter is None else torch.tensor([counter], dtype=torch.int32, device=dev)
    got = ops.cfg_dpmpp_step_patch(eps_u, eps_c, x_t, A_h.t.view(3, total), coef, k if counter is None else 0, patch, step=step,
                                   x_out=A_o.t.view(n, C, T, H, W), x_model=A_m.t.view(copies * n, C, T, H, W))
    torch.cuda.synchronize()
    tag = (tc.shape_id(shape), order, k, half, joint, copies, alias, xm_half)
    assert got.data_ptr() == A_o.t.data_ptr()
    assert bool(torch.isfinite(got).all()), tag
    assert torch.equal(got, want), (tag, int((got != want).sum()))
    kk = k % 3
    assert torch.equal(A_h.t.view(3, total)[kk], h_ref[kk]), (tag, "x0")
    cast = want.to(mt).reshape(-1)
    for q in range(copies):
        assert torch.equal(A_m.t[q * total:(q + 1) * total], cast), (tag, "x_model", q)
    for a in A_e:
        assert a.unchanged(), (tag, "eps written")
    assert A_h.unchanged(kk * total, (kk + 1) * total), (tag, "a history slot other than k % 3, or its surroundings, written")
    assert A_o.unchanged(0, total), (tag, "written outside x_out")
    assert A_m.unchanged(0, copies * total), (tag, "written outside x_model")
    if not alias:
        assert A_x.unchanged(), (tag, "x written")


@pytest.mark.parametrize("shape", tc.SHAPES, ids=tc.shape_id)
def test_patch_kernel_equals_the_dense_kernel_bit_for_bit(ops, dev, rows20, shape):
    """Orders 1, 2, 3 and 'taylor' x fp16 / fp32 storage x joint / split pointers x xm_copies 1 / 2 x x_out aliasing x:
    every combination on the small shapes, each value of each axis (rotating) on the three large ones."""
    ins = _inputs(shape, seed=sum(shape[:6]))
    small = ins[1].numel() < 100000
    combos = list(itertools.product(range(len(KINDS)), (True, False), (True, False), (1, 2), (False, True)))
    if not small:
        combos = [c for i, c in enumerate(combos) if i % 9 == 0]        # 8 of 64: every kind, both values of every axis
        assert {c[0] for c in combos} == {0, 1, 2, 3}
        assert all({c[j] for c in combos} == {True, False} for j in (1, 2, 4)) and {c[3] for c in combos} == {1, 2}
    for i, (ki, half, joint, copies, alias) in enumerate(combos):
        o, st = KINDS[ki]
        rows = rows20[(o, st)]
        k = 7 + i % 3                                         # walks through the three history slots
        assert int(rows[k][dc.ORDER]) == o
        run_case(ops, dev, shape, ins, rows, k, half, joint, copies, alias, xm_half=bool((i + ki) & 1))


def test_counter_form_equals_explicit_rows_and_saturates(ops, dev, rows20):
    shape = tc.SHAPES[1]
    ins = _inputs(shape, seed=5)
    rows = rows20[(3, "dpmsolver")]
    for k in (0, 1, 7, 19):
        run_case(ops, dev, shape, ins, rows, k, True, True, 2, False, True, counter=k)
    # a counter beyond the table reads the last row
    run_case(ops, dev, shape, ins, rows, 19, False, False, 1, True, False, counter=19 + 6)


# ---------------------------------------------------------------------------------------------------- loops
def _sample(dev, net, steps, cfg, split, fused, z, seen=None, enc=None):
    from viditq_amd.t2v import DMP_SOLVER
    cb = None if seen is None else (lambda i, v: seen.append((i, v)))
    return DMP_SOLVER(steps, cfg).sample(net, enc or tc.ToyTextEncoder(dev), tuple(z.shape[1:]), [""] * z.shape[0], dev,
                                         init_noise=z, cfg_split=split, fused=fused, step_callback=cb)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16model", "fp32model"])
@pytest.mark.parametrize("split", [False, True], ids=["joint", "split"])
def test_analytic_model_fused_equals_eager_step_by_step(ops, dev, split, dtype):
    z = torch.from_numpy(dc.gauss((2,) + tc.Z_SIZE, 41)).to(dev)
    for steps, cfg in ((20, 4.0), (3, 7.0), (2, 4.0)):
        ce, cf, se, sf = [], [], [], []
        want = _sample(dev, tc.AnalyticSTDiT(ce, dtype), steps, cfg, split, False, z, se)
        n0 = _calls()
        got = _sample(dev, tc.AnalyticSTDiT(cf, dtype), steps, cfg, split, True, z, sf)
        assert _calls() - n0 == steps                          # one C-ABI launch per model call
        assert torch.equal(got, want), (steps, cfg, float((got - want).abs().max()))
        assert len(cf) == len(ce) == steps * (2 if split else 1)
        for a, b in zip(ce, cf):                               # every model input: the sample (in the model's type) and time
            assert torch.equal(a[0].to(dtype), b[0].to(dtype)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert [i for i, _ in sf] == [i for i, _ in se] and all(torch.equal(a[1], b[1]) for a, b in zip(se, sf))


class _GoldText:
    """The text side of the tiny STDiT goldens as a text encoder: row 0 of ``y`` is the prompt, row 1 the null prompt."""

    def __init__(self, g, dev):
        self.y, self.mask = g["y"].half().to(dev), g["mask"].to(dev)

    def encode(self, prompts):
        return dict(y=self.y[:1].clone(), mask=self.mask[:1].clone())

    def null(self, n):
        return self.y[1:2].clone()


def _tiny(dev, plan):
    from test_model_gpu import _build
    if plan == "w8a8":
        g = load_npz("tiny_stdit_w8a8.npz")
        return g, _build(g, dev, 8)
    g = load_npz("tiny_stdit_w4a8.npz")
    qnn = _build(g, dev, 4, smooth=dict(alpha=[0.11, 0.11], timerange=[[0, 500], [501, 1000]]), mixed_precision=[4, 6, 8])
    qnn.set_layer_smooth_quant(model=qnn, module_name_list=FP_LAYERS, smooth_quant=False, smooth_quant_running_stat=False)
    return g, qnn


def _tiny_z(dev):
    return torch.from_numpy(dc.gauss((1, 4, 4, 8, 8), 43)).to(dev)


def test_tiny_stdit_patch_major_output_is_the_default_output(ops, dev):
    g, qnn = _tiny(dev, "w8a8")
    x, y, mask = g["x"].to(dev), g["y"].half().to(dev), g["mask"].to(dev)
    t = torch.tensor([500.0], device=dev)
    want = qnn(x, t, y[:1], mask=mask)
    pm = qnn(x, t, y[:1], mask=mask, patch_major=True)
    assert pm.dtype == torch.float16 and tuple(pm.shape) == (1, 4 * 4 * 4, 4 * 8) and pm.is_contiguous()
    assert want.dtype == torch.float32 and torch.equal(qnn.unpatchify(pm).float(), want)


@pytest.mark.parametrize("split", [False, True], ids=["joint", "split"])
def test_tiny_stdit_w8a8_fused_equals_eager_step_by_step(ops, dev, split):
    g, qnn = _tiny(dev, "w8a8")
    enc, z = _GoldText(g, dev), _tiny_z(dev)
    se, sf = [], []
    want = _sample(dev, qnn, 5, 4.0, split, False, z, se, enc)
    n0 = _calls()
    got = _sample(dev, qnn, 5, 4.0, split, True, z, sf, enc)
    assert _calls() - n0 > 5 and bool(torch.isfinite(got).all())
    assert [i for i, _ in sf] == [i for i, _ in se] == [2, 3, 4, 5]
    for (i, a), (_, b) in zip(se, sf):
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
    assert torch.equal(got, want)


def test_tiny_stdit_time_range_plan_fused_graph_and_eager_agree(ops, dev):
    """W4A8 with two smooth-quant time ranges, cfg_split, 20 steps (the model-input time crosses 500 after call 10): the
    eager loop, the eager-launched fused loop and VideoDPMStepGraph - two captures, both taken before the first replay -
    give the same bits, step by step."""
    from viditq_amd.t2v import DMP_SOLVER
    g, qnn = _tiny(dev, "w4a8")
    enc, z = _GoldText(g, dev), _tiny_z(dev)
    se, sf, sg = [], [], []
    want = _sample(dev, qnn, 20, 4.0, True, False, z, se, enc)
    got = _sample(dev, qnn, 20, 4.0, True, True, z, sf, enc)
    assert torch.equal(got, want) and all(torch.equal(a[1], b[1]) for a, b in zip(se, sf)) and len(sf) == 19
    graph = DMP_SOLVER(20, 4.0).step_graph(qnn, enc, tuple(z.shape[1:]), [""], dev, cfg_split=True)
    assert sorted(graph.graphs) == [0, 1] and graph.range_of == [1] * 10 + [0] * 10
    assert int(graph.step) == 0 and bool((graph.hist == 0).all()) and bool((graph.t == graph.t_first).all())
    out = graph.run(z, step_callback=lambda i, v: sg.append((i, v)))
    assert torch.equal(out, want), float((out - want).abs().max())
    assert [i for i, _ in sg] == list(range(1, 21))
    for (i, a), (_, b) in zip(se, sg[1:]):                    # (the eager callback starts after the order-2 warm-up)
        assert torch.equal(a, b), i
    assert torch.equal(graph.run(z), want)                    # and again: run() resets latent, time and counter


@pytest.mark.parametrize("split", [False, True], ids=["joint", "split"])
def test_step_graph_equals_the_eager_launched_fused_loop(ops, dev, split):
    from viditq_amd.t2v import DMP_SOLVER
    z = torch.from_numpy(dc.gauss((2,) + tc.Z_SIZE, 47)).to(dev)
    enc = tc.ToyTextEncoder(dev)
    for dtype in (torch.float16, torch.float32):
        net = tc.AnalyticSTDiT(None, dtype)
        want = _sample(dev, net, 20, 7.0, split, True, z, enc=enc)
        graph = DMP_SOLVER(20, 7.0).step_graph(net, enc, tc.Z_SIZE, tc.PROMPTS, dev, cfg_split=split)
        assert len(graph.graphs) == 1 and graph.xm.shape[0] == (2 if split else 4) and graph.xm.dtype == dtype
        assert torch.equal(graph.run(z), want)
        graph.graph.replay()                                   # one more: the counter stays on the last row
        torch.cuda.synchronize()
        assert int(graph.step) == 19


def test_fallbacks_are_taken(ops, dev, monkeypatch):
    """CPU tensors, cfg_scale == 1 and a model output the entry point refuses (a patch extent of 3) run eager, also with
    fused=True - and give what fused=False gives."""
    n_calls = [0]
    orig = ops.cfg_dpmpp_step_patch

    def counted(*a, **k):
        n_calls[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(ops, "cfg_dpmpp_step_patch", counted)
    z = torch.from_numpy(dc.gauss((2,) + tc.Z_SIZE, 53))
    a = _sample("cpu", tc.AnalyticSTDiT(), 3, 4.0, False, True, z, enc=tc.ToyTextEncoder())
    assert torch.equal(a, _sample("cpu", tc.AnalyticSTDiT(), 3, 4.0, False, False, z, enc=tc.ToyTextEncoder()))
    zd = z.to(dev)
    b = _sample(dev, tc.AnalyticSTDiT(), 3, 1.0, False, True, zd)
    assert torch.equal(b, _sample(dev, tc.AnalyticSTDiT(), 3, 1.0, False, False, zd))
    for split in (False, True):
        calls = []
        odd = tc.AnalyticSTDiT(calls, torch.float16, patch=(1, 1, 3))
        c = _sample(dev, odd, 3, 4.0, split, True, zd)
        assert len(calls) == 3 * (2 if split else 1)           # the refused first output is used, not recomputed
        assert torch.equal(c, _sample(dev, tc.AnalyticSTDiT(None, torch.float16, patch=(1, 1, 3)), 3, 4.0, split, False, zd))
    assert n_calls[0] == 0
    _sample(dev, tc.AnalyticSTDiT(), 3, 4.0, False, True, zd)
    assert n_calls[0] == 3

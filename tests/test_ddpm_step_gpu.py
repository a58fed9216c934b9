"""The fused IDDPM step on the GPU (vq_cfg_ddpm_step, ops.cfg_ddpm_step, SpacedDiffusion.p_sample_loop(fused=True),
graph.DDPMStepGraph): exact cases against the CPU model per element, general cases against the CPU model up to the one
exp, the eager torch expressions on the same device, what is never read, guards around every output, whole loops, the
counter form.

The bound of the general cases.  With h = 0.5 * lv, s = exp(h) in float64 and z the noise, the kernel computes
out = RN(mean + RN(RN(nonzero * expf(h)) * z)); nonzero is 0 or 1, so the first product is exact.  An expf within E ulp,
the rounding of the product and the rounding of the sum give
    |out - (mean + s z)| <= |s z| (2E + 1) 2^-24 (1 + 2^-20) + (|mean| + |s z|) 2^-24 (1 + 2^-20).
E is not the kernel's figure: it is the error of torch.exp on the GPU - the eager route's own exp - against float64 over
the h values of these tests, 1 ulp at most where it was measured (profiles/ddpm_step/README.md), rounded up, plus one ulp
because the library and torch may lower exp differently: EXP_ULPS = 2.
"""
import numpy as np
import pytest
import torch

import ddpm_step_cases as pc
from helpers import Arena

pytestmark = pytest.mark.gpu
EXP_ULPS = 2                                             # E above; measured 1 (profiles/ddpm_step/README.md) + 1
CFG = 4.5


def launch(ops, dev, row, eps, x, noise, half, padded=False, alias=False, xm=None, guided=3, nan_unread=True, k=0):
    """One launch of ``row`` as row k of a table with every buffer in an arena.  eps [2n, 2C, inner] / x / noise numpy.
    What the kernel must not read - uncond's channels >= guided, uncond's variance channels, the pitch padding - is NaN.
    Returns (x_out, x0_out, x_model) on the CPU after the guards passed."""
    n, C, inner = x.shape
    CI, tot = C * inner, x.size
    et = torch.float16 if half else torch.float32
    ld = 2 * CI + (8 if padded else 0)
    A_eps = Arena(dev, 2 * n * ld, et)
    A_x, A_z = Arena(dev, tot, torch.float32), Arena(dev, tot, torch.float32)
    A_o = A_x if alias else Arena(dev, tot, torch.float32)
    A_0 = Arena(dev, tot, torch.float32)
    A_m = Arena(dev, 2 * tot, xm) if xm is not None else None
    e = torch.from_numpy(eps.reshape(2 * n, 2 * C, inner)).to(dev).to(et)
    if nan_unread:
        e[n:, guided:] = float("nan")
    ev = A_eps.t.view(2 * n, ld)
    ev[:, :2 * CI] = e.reshape(2 * n, 2 * CI)
    A_x.t.copy_(torch.from_numpy(x.reshape(-1)))
    A_z.t.copy_(torch.from_numpy(noise.reshape(-1)))
    rows = np.zeros((k + 1, pc.ROW), dtype=np.float32)
    rows[k] = row
    coef = torch.from_numpy(rows).to(dev)
    eps_t = torch.as_strided(A_eps.t, (2 * n, 2 * C, inner), (ld, inner, 1))
    x_t = A_x.t.view(n, C, inner)
    arenas = [A_eps, A_x, A_z, A_o, A_0] + ([A_m] if A_m else [])
    for a in arenas:
        a.snapshot()
    assert ops.cfg_ddpm_step_ok(eps_t, x_t)
    got = ops.cfg_ddpm_step(eps_t, x_t, A_z.t.view(n, C, inner), coef, k, x_out=A_o.t.view(n, C, inner),
                            x0_out=A_0.t.view(n, C, inner), x_model=A_m.t.view(2 * n, C, inner) if A_m else None,
                            guided=guided)
    torch.cuda.synchronize()
    assert got.data_ptr() == A_o.t.data_ptr()
    assert A_eps.unchanged() and A_z.unchanged(), "an input was written"
    assert A_o.unchanged(0, tot), "written outside x_out"
    assert A_0.unchanged(0, tot), "written outside x0_out"
    if not alias:
        assert A_x.unchanged(), "x written"
    if A_m:
        assert A_m.unchanged(0, 2 * tot), "written outside x_model"
    return (A_o.t.cpu().numpy().reshape(x.shape), A_0.t.cpu().numpy().reshape(x.shape),
            A_m.t.cpu().float().numpy().reshape(2, *x.shape) if A_m else None)


@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "n%d_C%d_i%d" % s)
def test_exact_cases_per_element(ops, dev, shape):
    """P1 on every shape: x_out, x0_out and both halves of x_model bit for bit, for fp16 and fp32 eps, dense and padded
    pitch, x_out aliasing x, x_model in fp16 / fp32 - inside NaN arenas (the guard regions), the unread parts NaN."""
    for ci, case in enumerate(pc.p1_cases([shape])):
        want, want0 = case.expected()
        for half in (True, False):
            v = ci * 2 + int(half)
            padded, alias, xm = bool(v & 1) ^ bool(ci & 2), bool(v & 2), (None, torch.float16, torch.float32)[v % 3]
            got, got0, got_m = launch(ops, dev, case.row, case.eps, case.x, case.noise, half, padded, alias, xm,
                                      guided=case.guided, k=ci)
            tag = (case.name, half, padded, alias, xm)
            assert np.isfinite(got).all() and np.isfinite(got0).all(), tag
            assert np.array_equal(got, want), (tag, int((got != want).sum()), np.argwhere(got != want)[:3].tolist())
            assert np.array_equal(got0, want0), (tag, int((got0 != want0).sum()))
            if xm is not None:
                cast = torch.from_numpy(want).to(xm).float().numpy()
                assert np.array_equal(got_m[0], cast) and np.array_equal(got_m[1], cast), tag


def _ulps_of_torch_exp(dev, h):
    """The largest error of torch.exp on the GPU over ``h`` (fp32 numpy) against float64, in ulps of the exact value."""
    got = torch.exp(torch.from_numpy(h).to(dev)).cpu().numpy().astype(np.float64)
    ref = np.exp(h.astype(np.float64))
    ulp = 2.0 ** (np.floor(np.log2(ref)) - 23)
    return float((np.abs(got - ref) / ulp).max())


P2_SHAPES = [(2, 4, 1056), (2, 3, 7)]


@pytest.fixture(scope="module")
def p2_data():
    """inputs and the CPU model's (x0, mean, h, nonzero) per (shape, row, eps type): computed once, never written."""
    out = {}
    for si, shape in enumerate(P2_SHAPES):
        eps, x, noise = pc.p2_inputs(shape, 40 + si)
        for name, i, row, s in pc.p2_rows():
            for half in (True, False):
                out[(shape, name, half)] = (eps, x, noise, i, row, s, pc.reference_step(row, eps, x, noise, half))
    return out


@pytest.mark.parametrize("half", [True, False], ids=["fp16eps", "fp32eps"])
def test_general_cases_against_the_cpu_model(ops, dev, p2_data, half, parity):
    """P2: x0_out bit for bit; NONZERO = 0 rows give x_out == mean bit for bit; elsewhere the bound of the docstring."""
    worst, e_torch = 0.0, 0.0
    for (shape, name, hf), (eps, x, noise, i, row, s, (x0, mean, h, nz)) in p2_data.items():
        if hf != half:
            continue
        got, got0, _ = launch(ops, dev, row, eps, x, noise, half, padded=(shape[2] == 7))
        assert np.array_equal(got0, x0), (shape, name, int((got0 != x0).sum()))
        if nz == 0:
            assert i == 0 and np.array_equal(got, mean), (shape, name)
            continue
        centre, bound = pc.p2_bound(mean, h, nz, noise, EXP_ULPS)
        err = np.abs(got.astype(np.float64) - centre)
        print("ddpm_step %s %s half=%d: max err / bound = %.4f" % (shape, name, half, float((err / bound).max())))
        worst = max(worst, float((err / bound).max()))
        e_torch = max(e_torch, _ulps_of_torch_exp(dev, h))
        assert (err <= bound).all(), (shape, name, float((err / bound).max()))
    print("torch.exp on the GPU over these h: %.3f ulp" % e_torch)
    parity["ddpm_step_p2_half%d" % int(half)] = {"max_err_over_bound": worst, "torch_exp_ulps": e_torch,
                                                 "EXP_ULPS": EXP_ULPS}


@pytest.mark.parametrize("half", [True, False], ids=["fp16eps", "fp32eps"])
def test_eager_parity_on_the_gpu(ops, dev, p2_data, half):
    """The same inputs through the eager expressions of t2i/iddpm.py on the GPU: pred_xstart bit for bit, sample within
    twice the bound (both sides carry an exp)."""
    from viditq_amd.t2i.pixart import _PixArtBase
    for (shape, name, hf), (eps, x, noise, i, row, s, (x0, mean, h, nz)) in p2_data.items():
        if hf != half:
            continue
        n = shape[0]
        eps_g = torch.from_numpy(eps).to(dev).to(torch.float16 if half else torch.float32)
        x_g, z_g = torch.from_numpy(x).to(dev), torch.from_numpy(noise).to(dev)
        model = lambda x_, timestep, **kw: _PixArtBase.guide_cfg(eps_g, CFG)   # noqa: E731
        t = torch.full((2 * n,), i, dtype=torch.long, device=dev)
        want = s.p_sample(model, torch.cat([x_g, x_g]), t, clip_denoised=bool(row[pc.CLIP]), noise=torch.cat([z_g, z_g]))
        coef = torch.from_numpy(row[None].copy()).to(dev)
        x0_out = torch.empty_like(x_g)
        got = ops.cfg_ddpm_step(eps_g, x_g, z_g, coef, 0, x0_out=x0_out)
        assert want["pred_xstart"].dtype == torch.float32 and torch.equal(x0_out, want["pred_xstart"][:n]), (shape, name)
        _, bound = pc.p2_bound(mean, h, nz, noise, EXP_ULPS)
        err = (got.double() - want["sample"][:n].double()).abs().cpu().numpy()
        assert (err <= 2 * bound).all(), (shape, name, float((err / np.maximum(bound, 1e-300)).max()))


def test_unread_parts_do_not_reach_the_outputs(ops, dev):
    """Uncond's channels >= guided, uncond's variance channels and the pitch padding as NaN or as numbers: finite and the
    same bits, for guided 3, 1 and 0."""
    shape = (2, 4, 40)
    eps, x, noise = pc.p2_inputs(shape, 60)
    row = pc.p2_rows()[1][2]
    for guided in (3, 1, 0):
        for half in (True, False):
            a = launch(ops, dev, row, eps, x, noise, half, padded=True, xm=torch.float32, guided=guided, nan_unread=True)
            b = launch(ops, dev, row, eps, x, noise, half, padded=False, xm=torch.float32, guided=guided, nan_unread=False)
            for p, q in zip(a, b):
                assert np.isfinite(p).all() and np.array_equal(p, q), (guided, half)
    g3 = launch(ops, dev, row, eps, x, noise, False, guided=3)[0]
    g0 = launch(ops, dev, row, eps, x, noise, False, guided=0)[0]
    assert not np.array_equal(g3[:, :3], g0[:, :3]) and np.array_equal(g3[:, 3], g0[:, 3])


# ---------------------------------------------------------------------------------------------------- loops
def _kwargs(dev, **more):
    return dict(y=torch.zeros(2, 1, 2, 4, device=dev), cfg_scale=CFG, **more)


def _loop(s, model, z, noise, fused, clip=False, kw=None, **more):
    seen = []
    out = s.p_sample_loop(model, tuple(z.shape), z, clip_denoised=clip, model_kwargs=kw, noise_steps=noise, fused=fused,
                          step_callback=lambda i, smp, x0: seen.append((i, smp, x0)), **more)
    return out, seen


def _calls():
    from viditq_amd import _lib
    return _lib.CALLS[0]


@pytest.mark.parametrize("half", [True, False], ids=["fp16model", "fp32model"])
def test_loop_plumbing_is_exact_with_zero_noise(ops, dev, half):
    """out = mean whatever exp returns: fused == eager bit for bit at every step, sample and pred_xstart; the model saw
    timestep_map reversed and the duplicated latent; the return is cat([x, x])."""
    s = pc.make_sampler("10")
    n = 2
    z = torch.from_numpy(pc.gauss((n, 4, 8, 8), 21)).to(dev).repeat(2, 1, 1, 1)
    zeros = torch.zeros((10,) + tuple(z.shape), device=dev)
    for clip in (False, True):
        calls_e, calls_f = [], []
        want, seen_e = _loop(s, pc.analytic_net(half, calls_e).to(dev).forward_with_cfg, z, zeros, False, clip, _kwargs(dev))
        n0 = _calls()
        got, seen_f = _loop(s, pc.analytic_net(half, calls_f).to(dev).forward_with_cfg, z, zeros, True, clip, _kwargs(dev))
        assert _calls() - n0 == 10                                       # one C-ABI launch per model call
        assert [i for i, _, _ in seen_f] == [i for i, _, _ in seen_e] == list(range(10))[::-1]
        for (i, se, xe), (_, sf, xf) in zip(seen_e, seen_f):
            assert sf.shape[0] == n and torch.equal(sf, se[:n]), (clip, i, float((sf - se[:n]).abs().max()))
            assert torch.equal(xf, xe[:n]), (clip, i, "pred_xstart")
        assert torch.equal(got, torch.cat([seen_f[-1][1]] * 2)) and torch.equal(got[:n], want[:n])
        assert torch.equal(got.chunk(2, dim=0)[0], want.chunk(2, dim=0)[0])
        for calls in (calls_e, calls_f):
            assert [float(t[0]) for t, _ in calls] == [float(v) for v in list(s.timestep_map)[::-1]]
            assert all(bool((t == t[0]).all()) and t.numel() == 2 * n for t, _ in calls)
            assert all(torch.equal(x2[:n], x2[n:]) for _, x2 in calls)
        assert all(torch.equal(a[1], b[1]) for a, b in zip(calls_e, calls_f))


def test_tiny_pixart_loop_fused_equals_eager(ops, dev):
    """The depth-2 PixArtMS W8A8 of test_dpm_step_gpu.py through 10 steps with zero noise: fused == eager bit for bit at
    every step, with an fp16 x_model too, and as ONE captured step replayed ten times."""
    import test_dpm_step_gpu as tdpm
    g, qnn = tdpm._tiny_pixart(dev)
    s = pc.make_sampler("10")
    z = g["dpm_z"].to(dev).float().repeat(2, 1, 1, 1)
    n = z.shape[0] // 2
    kw = dict(y=torch.cat([g["y"][:1], g["dpm_null_y"]]).half().to(dev), cfg_scale=CFG, data_info=None,
              mask=g["mask"][:1].to(dev))
    zeros = torch.zeros((10,) + tuple(z.shape), device=dev)
    want, seen_e = _loop(s, qnn.forward_with_cfg, z, zeros, False, False, kw)
    got, seen_f = _loop(s, qnn.forward_with_cfg, z, zeros, True, False, kw)
    assert len(seen_f) == 10 and bool(torch.isfinite(got).all())
    for (i, se, xe), (_, sf, xf) in zip(seen_e, seen_f):
        assert torch.equal(sf, se[:n]) and torch.equal(xf, xe[:n]), i
    assert torch.equal(got[:n], want[:n]) and torch.equal(got[n:], got[:n])
    s16 = pc.make_sampler("10")
    s16.model_input_dtype = torch.float16                 # the kernel makes the model's cast
    assert torch.equal(_loop(s16, qnn.forward_with_cfg, z, zeros, True, False, kw)[0], got)
    sg = s16.p_sample_graph(qnn.forward_with_cfg, z, clip_denoised=False, model_kwargs=kw)
    assert torch.equal(sg.run(z, noise_steps=zeros), got)
    assert torch.equal(sg.run(z, noise_steps=zeros), got)


def test_loop_with_noise_step_by_step(ops, dev):
    """The eager GPU loop recorded per step (latent, model output, noise, sample); each record through ops.cfg_ddpm_step
    within the bound of that step - nothing is compared across accumulated steps."""
    s = pc.make_sampler("10")
    n = 2
    z = torch.from_numpy(pc.gauss((n, 4, 8, 8), 22)).to(dev).repeat(2, 1, 1, 1)
    noise = torch.from_numpy(pc.gauss((10, 2 * n, 4, 8, 8), 23)).to(dev)
    rows_h = s.step_rows(CFG, False)
    rows = rows_h.to(dev)
    for half in (True, False):
        calls = []
        _, seen = _loop(s, pc.analytic_net(half, calls).to(dev).forward_with_cfg, z, noise, False, False, _kwargs(dev))
        fwd = pc.analytic_forward(half)
        for k, ((t, x2), (i, smp, x0e)) in enumerate(zip(calls, seen)):
            eps = fwd(x2.to(dev), t.to(dev))
            x = x2[:n].to(dev).contiguous()
            x0 = torch.empty_like(x)
            got = ops.cfg_ddpm_step(eps, x, noise[k][:n], rows, k, x0_out=x0)
            assert torch.equal(x0, x0e[:n]), (half, k)
            r0, mean, h, nz = pc.reference_step(rows_h[k].numpy(), eps.float().cpu().numpy().reshape(2 * n, 8, -1),
                                                x.cpu().numpy().reshape(n, 4, -1),
                                                noise[k][:n].cpu().numpy().reshape(n, 4, -1), half)
            _, bound = pc.p2_bound(mean, h, nz, noise[k][:n].cpu().numpy().reshape(n, 4, -1), EXP_ULPS)
            err = (got.double() - smp[:n].double()).abs().cpu().numpy().reshape(bound.shape)
            assert (err <= 2 * bound).all(), (half, k)
            if nz == 0:
                assert torch.equal(got, smp[:n]), (half, k)


def test_fallbacks_launch_no_fused_step(ops, dev, monkeypatch):
    """A model that is not a package forward_with_cfg, a CPU latent, fused=False: eager, no fused launch."""
    n_calls = [0]
    orig = ops.cfg_ddpm_step

    def counted(*a, **k):
        n_calls[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(ops, "cfg_ddpm_step", counted)
    s = pc.make_sampler("10")
    z = torch.from_numpy(pc.gauss((1, 4, 4, 4), 2)).repeat(2, 1, 1, 1)
    zeros = torch.zeros((10,) + tuple(z.shape))
    zg, zeros_g = z.to(dev), zeros.to(dev)
    net = pc.analytic_net(True).to(dev)
    a = _loop(s, pc.analytic_cfg_model(True), zg, zeros_g, True, kw=dict(cfg_scale=CFG))[0]
    b = _loop(s, pc.analytic_net(True).forward_with_cfg, z, zeros, True, kw=_kwargs("cpu"))[0]
    c = _loop(s, net.forward_with_cfg, zg, zeros_g, False, kw=_kwargs(dev))[0]
    assert n_calls[0] == 0
    assert torch.equal(a, c) and a.shape == z.shape and b.shape == z.shape
    d = _loop(s, net.forward_with_cfg, zg, zeros_g, True, kw=_kwargs(dev))[0]
    assert n_calls[0] == 10 and torch.equal(d[:1], c[:1])
    # a model output the kernel does not take (bf16): the eager route continues from that first call
    calls = []
    bf = pc.analytic_net(False, calls).to(dev)
    inner = bf.forward
    bf.forward = lambda *a_, **k_: inner(*a_, **k_).bfloat16()
    e = _loop(s, bf.forward_with_cfg, zg, zeros_g, True, kw=_kwargs(dev))[0]
    assert n_calls[0] == 10 and len(calls) == 10
    assert torch.equal(e, _loop(s, bf.forward_with_cfg, zg, zeros_g, False, kw=_kwargs(dev))[0])


# ---------------------------------------------------------------------------------------------------- counter form
def test_counter_form_replays_one_captured_step(ops, dev):
    """{analytic forward, step(step=counter), advance} in one captured graph over 10 rows == the eager-launched fused loop
    with the same noise stack, bit for bit, at every step; the counter saturates at the last row; a second run() and a
    run from a generator reproduce the loop's."""
    n = 2
    z = torch.from_numpy(pc.gauss((n, 4, 8, 8), 31)).to(dev).repeat(2, 1, 1, 1)
    noise = torch.from_numpy(pc.gauss((10, 2 * n, 4, 8, 8), 32)).to(dev)
    for half, clip in ((True, False), (False, True)):
        s = pc.make_sampler("10")
        net = pc.analytic_net(half).to(dev)
        want, seen = _loop(s, net.forward_with_cfg, z, noise, True, clip, _kwargs(dev))
        sg = s.p_sample_graph(net.forward_with_cfg, z, clip_denoised=clip, model_kwargs=_kwargs(dev))
        t_seen, c_seen, got_seen = [], [], []
        got = sg.run(z, noise_steps=noise, step_callback=lambda i, v, x0: (
            t_seen.append(sg.t.clone()), c_seen.append(sg.step.clone()), got_seen.append((i, v, x0))))
        assert torch.equal(got, want), (half, clip)
        for k in range(10):
            assert got_seen[k][0] == seen[k][0] and torch.equal(got_seen[k][1], seen[k][1]), k
            assert torch.equal(got_seen[k][2], seen[k][2]), k
            assert t_seen[k].dtype == torch.float32 and bool((t_seen[k] == float(s.timestep_map[(9 - k) - 1])).all()), k
            assert int(c_seen[k]) == min(k + 1, 9)
        sg.graph.replay()                                  # one more: the counter stays on the last row
        torch.cuda.synchronize()
        assert int(sg.step) == 9 and bool(torch.isfinite(sg.x).all())
        assert torch.equal(sg.run(z, noise_steps=noise), want)          # run() resets latent, time and counter
        a = sg.run(z, generator=torch.Generator(device=dev).manual_seed(5))
        b = s.p_sample_loop(net.forward_with_cfg, tuple(z.shape), z, clip_denoised=clip, model_kwargs=_kwargs(dev),
                            fused=True, generator=torch.Generator(device=dev).manual_seed(5))
        assert torch.equal(a, b) and not torch.equal(a, want)

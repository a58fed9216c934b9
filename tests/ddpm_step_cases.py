"""Cases and a step-by-step CPU model for the fused IDDPM step (vq_cfg_ddpm_step, csrc/sampler.hip).

reference_step evaluates ONE fused step in the operation order include/viditq.h documents, every operation rounded on
its own (numpy never contracts), with the six fp16 roundings of an fp16 model output.  It stops in front of the exp:
it returns (x0, mean, h = 0.5 * lv, nonzero), and out = mean + (nonzero * exp(h)) * noise is left to the caller.

P1 (exact)   operands are multiples of 2^-4 with |.| <= 8 that encode (batch half, b, channel, inner position); cfg and
             the multipliers of the hand-made rows are powers of two, MIN_LOG = MAX_LOG = 0, so lv = 0 and expf(0) = 1.
             p1_prove shows that every intermediate is exact in fp16 (where the eager path rounds to fp16) and in fp32: the
             expected out and x0 do not depend on grouping or contraction; a wrong index, channel rule, batch half or
             clamp is a wrong number.  NONZERO 0 / 1, CLIP 0 / 1 (x0 lies on both sides of +-1), guided 3 / 1 / 0.
P2 (general) Gaussian eps / x / noise, variance channels uniform in [-1.2, 1.2], rows of the real "100" and "20"
             schedules: first, a middle and the last row.
Shapes       (n, C, inner) below, each with a dense model output and with a padded batch pitch.
"""
import numpy as np
import torch

ROW = 16
(CFG, A, B, C1, C2, MIN_LOG, MAX_LOG, NONZERO, CLIP) = range(9)
T_NEXT = 14

# (1, 4, 1) / (2, 3, 7): one element per access, odd inner; (2, 4, 1024): four per access, several blocks;
# (5, 4, 65536): 1.3 M elements, a second pass of the capped 1024 x 256 x 4 grid; (1, 3, 100003): a second pass of the
# one-element form (1024 x 256 threads)
SHAPES = [(1, 4, 1), (2, 3, 7), (2, 4, 1024), (5, 4, 65536), (1, 3, 100003)]


def _f16(v):
    return v.astype(np.float16).astype(np.float32)


def _tree(row, c, u, v, x, guided, r16, r32):
    """The documented expression tree on arrays of one type ([n, C, inner] each); r16 / r32 are applied where the kernel
    rounds to fp16 / fp32.  Returns {name: intermediate}."""
    s = [x.dtype.type(t) for t in row]
    one, half = x.dtype.type(1.0), x.dtype.type(0.5)
    P = {}
    P["d"] = r16(c - u)
    P["p"] = r16(s[CFG] * P["d"])
    P["g"] = r16(u + P["p"])
    ch = np.arange(x.shape[1])[None, :, None]
    e = P["e"] = np.where(ch < guided, P["g"], c)
    P["v1"] = r16(v + one)
    P["frac"] = r16(P["v1"] * half)
    P["rest"] = r16(one - P["frac"])
    P["lmax"] = r32(P["frac"] * s[MAX_LOG])
    P["lmin"] = r32(P["rest"] * s[MIN_LOG])
    P["lv"] = r32(P["lmax"] + P["lmin"])
    P["ax"] = r32(s[A] * x)
    P["be"] = r32(s[B] * e)
    x0 = P["x0"] = r32(P["ax"] - P["be"])
    if row[CLIP] != 0:
        x0 = P["x0"] = np.clip(x0, -one, one)
    P["m1"] = r32(s[C1] * x0)
    P["m2"] = r32(s[C2] * x)
    P["mean"] = r32(P["m1"] + P["m2"])
    P["h"] = r32(half * P["lv"])
    return P


def reference_step(row, eps, x, noise, eps_half, guided=3):
    """One fused step.  row: [ROW] fp32; eps: [2n, 2C, inner] cond | uncond (rounded to fp16 first when eps_half, else
    taken as fp32); x, noise: [n, C, inner] fp32.  Returns (x0, mean, h, nonzero): out = mean + (nonzero * exp(h)) * noise."""
    row = np.asarray(row, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, C = x.shape[:2]
    assert noise.shape == x.shape
    e = np.asarray(eps)
    e = _f16(e) if eps_half else e.astype(np.float32)
    assert e.shape == (2 * n, 2 * C, x.shape[2])
    c, u, v = e[:n, :C], e[n:, :C], e[:n, C:]
    ident = lambda t: t   # noqa: E731
    with np.errstate(all="ignore"):
        P = _tree(row, c, u, v, x, guided, _f16 if eps_half else ident, ident)
    for k in ("x0", "mean", "h"):
        assert P[k].dtype == np.float32
    return P["x0"], P["mean"], P["h"], np.float32(row[NONZERO])


# ------------------------------------------------------------------------------------------------ P1: exact cases
def _enc(shape, half, salt):
    """Multiples of 2^-4 in [-8, 8] that encode (half, b, channel, inner position), as dpm_step_cases._enc does."""
    n, C, inner = shape
    b = np.arange(n, dtype=np.int64)[:, None, None]
    ch = np.arange(C, dtype=np.int64)[None, :, None]
    j = np.arange(inner, dtype=np.int64)[None, None, :]
    v = (b * 37 + ch * 11 + j * 3 + half * 101 + salt * 53) % 257 - 128
    return (v.astype(np.float32) / 16.0)


def p1_row(nonzero, clip):
    """A hand-made row whose every multiplier is a power of two; MIN_LOG = MAX_LOG = 0."""
    r = np.zeros(ROW, dtype=np.float32)
    r[CFG], r[A], r[B], r[C1], r[C2] = 2.0, 0.5, 0.25, 0.5, 0.25
    r[NONZERO], r[CLIP], r[T_NEXT] = float(nonzero), float(clip), 750.0
    return r


class P1Case:
    def __init__(self, shape, nonzero, clip, guided):
        n, C, inner = shape
        self.shape, self.nonzero, self.clip, self.guided = shape, nonzero, clip, min(guided, C)
        self.name = "n%d_C%d_i%d_nz%d_clip%d_g%d" % (n, C, inner, nonzero, clip, self.guided)
        self.row = p1_row(nonzero, clip)
        wide = (n, 2 * C, inner)                                          # eps channels | variance channels
        self.eps = np.concatenate([_enc(wide, 0, 0), _enc(wide, 1, 0)])   # [2n, 2C, inner]: cond | uncond
        self.x = _enc(shape, 0, 1)
        self.noise = _enc(shape, 1, 2)

    def expected(self):
        """(out, x0) - exact (p1_prove), the same for an fp16 and an fp32 model output."""
        x0, mean, h, nz = reference_step(self.row, self.eps, self.x, self.noise, False, self.guided)
        assert not h.any()
        return mean + nz * self.noise, x0


P1_KINDS = [(1, 0, 3), (0, 1, 3), (1, 1, 1), (0, 0, 0)]               # (NONZERO, CLIP, guided)


def p1_cases(shapes=None):
    return [P1Case(shape, *kind) for shape in (shapes or SHAPES) for kind in P1_KINDS]


def p1_prove(case):
    """Evaluates the tree in fp64 and shows that every intermediate already IS an fp16 number (the six values the eager
    path rounds to fp16) or an fp32 number (all others), lv = 0, and mean + nonzero * noise is an fp32 number too: each
    operation's exact result is its rounded result, with or without a contraction.  Also: x0 lies on both sides of +-1.
    Returns the largest magnitude met."""
    x = case.x.astype(np.float64)
    n, C = x.shape[:2]
    e = case.eps.astype(np.float64)
    c, u, v = e[:n, :C], e[n:, :C], e[:n, C:]
    big = [0.0]

    def exact(kind):
        def f(t):
            assert np.isfinite(t).all()
            assert np.array_equal(t.astype(kind).astype(np.float64), t), case.name
            big[0] = max(big[0], float(np.abs(t).max()))
            return t
        return f
    for operand in (c, u, v):
        exact(np.float16)(operand)                                    # the inputs themselves are fp16 numbers
    unclipped = case.row.astype(np.float64)
    unclipped[CLIP] = 0
    raw = _tree(unclipped, c, u, v, x, case.guided, exact(np.float16), exact(np.float32))["x0"]
    if x.size >= 1024:                                                # (the two smallest shapes hold too few values)
        assert (raw > 1).any() and (raw < -1).any() and (np.abs(raw) < 1).any(), case.name
    P = _tree(case.row.astype(np.float64), c, u, v, x, case.guided, exact(np.float16), exact(np.float32))
    assert not P["lv"].any() and not P["h"].any()
    out = exact(np.float32)(P["mean"] + float(case.row[NONZERO]) * case.noise.astype(np.float64))
    if case.clip:
        assert np.abs(P["x0"]).max() <= 1.0
    for half in (True, False):                                        # the fp32 model computes the very same numbers
        x0, mean, h, nz = reference_step(case.row, case.eps, case.x, case.noise, half, case.guided)
        assert np.array_equal(x0.astype(np.float64), P["x0"]) and np.array_equal(mean.astype(np.float64), P["mean"])
    got, got0 = case.expected()
    assert np.array_equal(got.astype(np.float64), out) and np.array_equal(got0.astype(np.float64), P["x0"])
    return big[0]


# ------------------------------------------------------------------------------------------------ P2: general cases
def make_sampler(respacing="10"):
    import viditq_amd  # noqa: F401
    from viditq_amd.t2i.iddpm import IDDPM
    return IDDPM(respacing)


def p2_rows():
    """[(name, i, row, sampler)]: the first, a middle and the last row of the real "100" (clip off) and "20" (clip on)
    schedules at cfg 4.5; i is the loop index the row belongs to."""
    out = []
    for resp, clip in (("100", False), ("20", True)):
        s = make_sampler(resp)
        rows = s.step_rows(4.5, clip).numpy()
        steps = rows.shape[0]
        for k in (0, steps // 2, steps - 1):
            out.append(("r%s_k%d" % (resp, k), steps - 1 - k, rows[k].copy(), s))
    return out


def gauss(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).numpy()


def p2_inputs(shape, seed):
    """(eps [2n, 2C, inner] with the variance channels uniform in [-1.2, 1.2], x, noise) as float32 numpy."""
    n, C, inner = shape
    eps = gauss((2 * n, 2 * C, inner), seed)
    g = torch.Generator().manual_seed(seed + 1000)
    eps[:, C:] = (torch.rand(2 * n, C, inner, generator=g) * 2.4 - 1.2).numpy()
    return eps.astype(np.float32), gauss(shape, seed + 1).astype(np.float32), gauss(shape, seed + 2).astype(np.float32)


def p2_bound(mean, h, nonzero, noise, E):
    """(centre, bound) of |x_out - centre| in float64: expf's error of E ulp, the rounding of the product, the rounding of
    the sum (tests/test_ddpm_step_gpu.py states the formula's origin)."""
    s = np.exp(h.astype(np.float64)) * float(nonzero)
    sz = np.abs(s * noise.astype(np.float64))
    u = 2.0 ** -24 * (1 + 2.0 ** -20)
    centre = mean.astype(np.float64) + s * noise.astype(np.float64)
    return centre, sz * (2 * E + 1) * u + (np.abs(mean.astype(np.float64)) + sz) * u


# ------------------------------------------------------------------------------------------------ analytic models
def analytic_forward(half, calls=None):
    """forward(x2, t): a [2n, 2C, ...] output of adds and products only (the same bits on every CPU) that differs between
    the batch halves and moves with the model-input time; the variance channels stay within [-1.2, 1.2].  fp16 output
    when ``half`` (the fp16 roundings of the eager path), else fp32."""
    def forward(x2, t):
        if calls is not None:
            calls.append((t.detach().float().cpu().clone(), x2.detach().float().cpu().clone()))
        n = x2.shape[0] // 2
        z = x2.half() if half else x2.float()
        shape = (-1,) + (1,) * (z.dim() - 1)
        g = (0.1 + t.to(z.dtype) / 20000.0).reshape(shape)
        f = torch.cat([torch.full((n,), 1.0, dtype=z.dtype, device=z.device),
                       torch.full((n,), 1.3, dtype=z.dtype, device=z.device)]).reshape(shape)
        return torch.cat([z * g * f, (z * 0.4 * f).clamp(-1.2, 1.2)], dim=1)
    return forward


def analytic_cfg_model(half, calls=None):
    """``model(x, timestep=..., cfg_scale=...)`` with forward_with_cfg's data flow around analytic_forward, written out so
    that the imported reference and this package are driven by the same callable on the CPU."""
    fwd = analytic_forward(half, calls)

    def model(x, timestep, cfg_scale, **kw):
        h = x[: len(x) // 2]
        out = fwd(torch.cat([h, h], dim=0), timestep)
        eps, rest = out[:, :3], out[:, 3:]
        cond_eps, uncond_eps = torch.split(eps, len(eps) // 2, dim=0)
        half_eps = uncond_eps + cfg_scale * (cond_eps - uncond_eps)
        return torch.cat([torch.cat([half_eps, half_eps], dim=0), rest], dim=1)
    return model


def analytic_net(half, calls=None):
    """A net of the package (the fused route asks for one) whose forward is analytic_forward."""
    import viditq_amd  # noqa: F401
    from viditq_amd.t2i import PixArtMS

    class AnalyticNet(PixArtMS):
        def forward(self, x, timestep, y, mask=None, **kw):
            return analytic_forward(half, calls)(x, timestep)
    return AnalyticNet(input_size=4, depth=1, hidden_size=16, num_heads=2, model_max_length=2, caption_channels=4)


def run_table(sampler, x_dup, noise_steps, cfg_scale, clip, half):
    """The CPU model driven through step_rows: x0 and mean of every step of what the fused route computes for the kept
    half, with out taken from the eager expression's own exp (torch, CPU): [(x0, mean, out)] per step."""
    rows = sampler.step_rows(cfg_scale, clip).numpy()
    n = x_dup.shape[0] // 2
    xs = x_dup[:n].numpy().reshape(n, x_dup.shape[1], -1)
    fwd = analytic_forward(half)
    t_in = float(sampler.timestep_map[-1])
    out = []
    for k in range(rows.shape[0]):
        xt = torch.from_numpy(xs.reshape((n,) + tuple(x_dup.shape[1:])))
        eps = fwd(torch.cat([xt, xt]), torch.full((2 * n,), t_in)).float().numpy().reshape(2 * n, 2 * xs.shape[1], -1)
        z = noise_steps[k][:n].numpy().reshape(xs.shape)
        x0, mean, h, nz = reference_step(rows[k], eps, xs, z, half)
        xs = (torch.from_numpy(mean) + torch.from_numpy(nz * np.ones_like(h)) * torch.exp(torch.from_numpy(h))
              * torch.from_numpy(z)).numpy()
        out.append((x0, mean, xs))
        t_in = float(rows[k][T_NEXT])
    return out

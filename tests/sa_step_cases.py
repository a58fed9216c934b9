"""Cases and a step-by-step CPU model for the SA-Solver port (viditq_amd/t2i/sa_solver.py) and its fused step
(vq_cfg_sa_step, csrc/sampler.hip).

reference_step evaluates ONE fused step in the operation order include/viditq.h documents, every operation rounded on its
own (numpy never contracts), with the three fp16 roundings of an fp16 model output.  Families:

P1 (exact)   operands are multiples of 2^-4 with |.| <= 8 that encode (batch half, b, channel, inner position); cfg, sigma,
             alpha and the coefficients of the hand-made rows are powers of two (or zero).  p1_prove shows in float64 that
             every intermediate is exact in fp16 (the guidance) and in fp32 (all others): the expected outputs do not depend
             on grouping or contraction; a wrong index, column, history slot, noise slot, order branch or batch half is a
             wrong number.  Rows: every coefficient set; one-hot in each of CX, CG0, CG1, CN, PX, PG0, PG1, PN; OC = 0;
             orders 1.  Each at an even and an odd k (both ring parities).
P2 (general) Gaussian operands with every row of a real 6-step table (eta = 1: tau is 1 inside the window, 0 outside).
Shapes       (n, C, inner) below, each with a dense model output and with a padded batch pitch.

TRAJECTORIES, TIME_LISTS, TAUS and the seeds name what tests/golden/make_golden_sa_solver.py records from the reference.
"""
import numpy as np
import torch

from dpm_step_cases import analytic_model, gauss  # noqa: F401  (the forward_with_dpmsolver-shaped analytic model)

ROW = 16
(CFG, SIGMA, ALPHA, OC, CX, CG0, CG1, CN, OP, PX, PG0, PG1, PN) = range(13)
T_NEXT = 14

# (1, 4, 1) / (2, 3, 7): one element per access, odd inner; (2, 4, 1024): four per access, several blocks;
# (5, 4, 65536): 1.3 M elements, a second pass of the capped 1024 x 256 x 4 grid; (1, 3, 100003): a second pass of the
# one-element form (1024 x 256 threads)
SHAPES = [(1, 4, 1), (2, 3, 7), (2, 4, 1024), (5, 4, 65536), (1, 3, 100003)]

# ------------------------------------------------------------------------------------------------ what the golden file holds
SEED, GUIDE, LATENT = 11, 4.5, (1, 4, 8, 8)
# name -> (mode, steps, predictor, corrector, pc_mode, skip_type, eta, fp16 model output)
TRAJECTORIES = {
    "few_p2c2": ("few_steps", 6, 2, 2, "PEC", "time", 1, False),
    "few_p2c2_f16": ("few_steps", 6, 2, 2, "PEC", "time", 1, True),
    "few_p2c2_eta0": ("few_steps", 6, 2, 2, "PEC", "time", 0, False),
    "few_p3c4": ("few_steps", 6, 3, 4, "PEC", "time", 1, False),
    "few_p2c2_pece": ("few_steps", 5, 2, 2, "PECE", "time", 1, False),
    "few_p2c0": ("few_steps", 6, 2, 0, "PEC", "time", 1, False),
    "more_p3c4": ("more_steps", 6, 3, 4, "PEC", "time", 1, False),
    "few_p2c2_logsnr": ("few_steps", 6, 2, 2, "PEC", "logSNR", 1, False),
    "few_p2c2_karras": ("few_steps", 6, 2, 2, "PEC", "karras", 1, False),
}
KERNEL_TRAJECTORIES = ("few_p2c2", "few_p2c2_f16", "few_p2c2_eta0")      # what the fused step serves
# previous times in loop order (the last one is the step's start) and the time stepped to
TIME_LISTS = [([0.9, 0.7, 0.55, 0.4], 0.3), ([0.35, 0.2, 0.1, 0.05], 0.02)]
TAUS = [0, 0.5, 1]
UPDATES = ("adams_bashforth_update", "adams_moulton_update", "adams_bashforth_update_few_steps",
           "adams_moulton_update_few_steps")
GRID_N = (5, 25)
SKIPS = ("time", "logSNR", "karras")


def tau_window(eta):
    """tau_t of sa_sampler.py:90."""
    return lambda t: eta if 0.2 <= t <= 0.8 else 0


def start_latent(seed=SEED):
    return torch.from_numpy(gauss(LATENT, seed))


def noise_stack(seed, steps):
    """The 1 + steps draws ``randn_like`` makes after ``torch.manual_seed(seed)`` (the first is never used)."""
    torch.manual_seed(seed)
    return torch.stack([torch.randn(*LATENT) for _ in range(1 + steps)])


def update_inputs(li):
    """(x, [four model outputs], noise) of the direct update calls on time list ``li``."""
    x = torch.from_numpy(gauss(LATENT, 100 + li))
    models = [torch.from_numpy(gauss(LATENT, 110 + 10 * li + j)) for j in range(4)]
    return x, models, torch.from_numpy(gauss(LATENT, 150 + li))


def make_solver(cfg_scale=GUIDE, model=None):
    import viditq_amd  # noqa: F401
    from viditq_amd.t2i.sa_solver import SASolver
    y = torch.zeros(1, 1, 2, 4)
    return SASolver(model, y, y.clone(), cfg_scale)


# ------------------------------------------------------------------------------------------------ the CPU model
def _f16(v):
    return v.astype(np.float16).astype(np.float32)


def _tree(row, u, c, x, xp, m1, zc, zp, r16, r32):
    """The documented expression tree on arrays of one type; r16 / r32 are applied where the kernel rounds to fp16 / fp32.
    Returns (xc, xq, m_k, {name: intermediate})."""
    oc, op = int(row[OC]), int(row[OP])
    assert oc in (0, 1, 2) and op in (0, 1, 2)
    s = [x.dtype.type(v) for v in row]
    P = {}
    P["d"] = r16(c - u)
    P["p"] = r16(s[CFG] * P["d"])
    P["e"] = r16(u + P["p"])
    P["se"] = r32(s[SIGMA] * P["e"])
    P["t"] = r32(xp - P["se"])
    m = P["m"] = r32(P["t"] / s[ALPHA])
    v = x
    if oc >= 1:
        g = P["g0"] = r32(s[CG0] * m)
        if oc == 2:
            P["g1"] = r32(s[CG1] * m1)
            g = P["g"] = r32(g + P["g1"])
        P["ca"] = r32(s[CX] * v)
        P["cag"] = r32(P["ca"] + g)
        P["cnz"] = r32(s[CN] * zc)
        v = P["xc"] = r32(P["cag"] + P["cnz"])
    xc = v
    if op >= 1:
        q = P["q0"] = r32(s[PG0] * m)
        if op == 2:
            P["q1"] = r32(s[PG1] * m1)
            q = P["q"] = r32(q + P["q1"])
        P["pa"] = r32(s[PX] * v)
        P["paq"] = r32(P["pa"] + q)
        P["pnz"] = r32(s[PN] * zp)
        v = P["xq"] = r32(P["paq"] + P["pnz"])
    return xc, v, m, P


def reference_step(row, eps, x, xp, hist, noise, k, eps_half):
    """One fused step number k.  row: [ROW] fp32; eps: [2n, C, inner] uncond | cond (rounded to fp16 first when eps_half,
    else taken as fp32); x, xp: [n, C, inner] fp32; hist, noise: [2, n*C*inner] fp32.  Returns (x_out, xp_out, hist_new)."""
    row = np.asarray(row, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    xp = np.ascontiguousarray(xp, dtype=np.float32).reshape(x.shape)
    n = x.shape[0]
    e = np.asarray(eps)
    e = _f16(e) if eps_half else e.astype(np.float32)
    u, c = e[:n].reshape(x.shape), e[n:].reshape(x.shape)
    hist = np.array(hist, dtype=np.float32, copy=True).reshape(2, -1)
    noise = np.asarray(noise, dtype=np.float32).reshape(2, -1)
    m1 = hist[(k - 1) % 2].reshape(x.shape)
    zc, zp = noise[k % 2].reshape(x.shape), noise[(k + 1) % 2].reshape(x.shape)
    ident = lambda v: v   # noqa: E731
    with np.errstate(all="ignore"):
        xc, xq, m, _ = _tree(row, u, c, x, xp, m1, zc, zp, _f16 if eps_half else ident, ident)
    assert xc.dtype == np.float32 and xq.dtype == np.float32 and m.dtype == np.float32
    hist[k % 2] = m.reshape(-1)
    return xc, xq, hist


# ------------------------------------------------------------------------------------------------ P1: exact cases
def _enc(shape, half, salt):
    """Multiples of 2^-4 in [-8, 8] that encode (half, b, channel, inner position), as dpm_step_cases._enc does."""
    n, C, inner = shape
    b = np.arange(n, dtype=np.int64)[:, None, None]
    ch = np.arange(C, dtype=np.int64)[None, :, None]
    j = np.arange(inner, dtype=np.int64)[None, None, :]
    v = (b * 37 + ch * 11 + j * 3 + half * 101 + salt * 53) % 257 - 128
    return (v.astype(np.float32) / 16.0)


COEFS = (CX, CG0, CG1, CN, PX, PG0, PG1, PN)
COEF_NAMES = dict(zip(COEFS, ("CX", "CG0", "CG1", "CN", "PX", "PG0", "PG1", "PN")))


def p1_row(kind):
    """A hand-made row: cfg 2, sigma = alpha = 1/2 (the division by 1/2 is exact), T_NEXT 750.  ``kind``: 'all' (eight
    distinct powers of two, orders 2 / 2), 'o11' (the same, orders 1 / 1), 'oc0' (no corrector, predictor order 2), or one
    of COEFS: that coefficient 2 and the other seven 0, orders 2 / 2."""
    r = np.zeros(ROW, dtype=np.float32)
    r[CFG], r[SIGMA], r[ALPHA], r[T_NEXT] = 2.0, 0.5, 0.5, 750.0
    if kind in COEFS:
        r[OC], r[OP], r[kind] = 2, 2, 2.0
        return r
    r[CX], r[CG0], r[CG1], r[CN] = 0.5, 0.25, -0.5, 2.0
    r[PX], r[PG0], r[PG1], r[PN] = 2.0, -0.125, 0.25, 0.5
    r[OC], r[OP] = {"all": (2, 2), "o11": (1, 1), "oc0": (0, 2)}[kind]
    return r


class P1Case:
    def __init__(self, shape, kind, k):
        self.shape, self.kind, self.k = shape, kind, k
        self.name = "n%d_C%d_i%d_%s_k%d" % (*shape, COEF_NAMES.get(kind, kind), k)
        self.row = p1_row(kind)
        self.eps = np.concatenate([_enc(shape, 0, 0), _enc(shape, 1, 0)])            # [2n, C, inner]: uncond | cond
        self.x, self.xp = _enc(shape, 0, 1), _enc(shape, 1, 1)
        self.hist = np.stack([_enc(shape, 0, 2 + s).reshape(-1) for s in range(2)])  # two distinguishable slots
        self.noise = np.stack([_enc(shape, 1, 4 + s).reshape(-1) for s in range(2)])

    def expected(self, half=False):
        """(x_out, xp_out, hist) - exact (p1_prove), the same for an fp16 and an fp32 model output."""
        return reference_step(self.row, self.eps, self.x, self.xp, self.hist, self.noise, self.k, half)


P1_KINDS = ("all", "o11", "oc0") + COEFS


def p1_cases(shapes=None):
    """Every kind at an even and an odd k on the shapes of up to 2^13 elements; on the two large ones 'all' at both
    parities and the one-hot rows in turn (each of them once, parities alternating)."""
    out = []
    for shape in shapes or SHAPES:
        if shape[0] * shape[1] * shape[2] <= 8192:
            out += [P1Case(shape, kind, k) for kind in P1_KINDS for k in (2, 3)]
        else:
            out += [P1Case(shape, "all", 4), P1Case(shape, "all", 5)]
            out += [P1Case(shape, kind, 2 + (i + shape[1]) % 2) for i, kind in enumerate(COEFS)]
    return out


def p1_prove(case):
    """Evaluates the tree in fp64 and shows that every intermediate already IS an fp16 number (the three values the eager
    path rounds to fp16) or an fp32 number (all others): each operation's exact result is its rounded result, with or
    without a contraction.  Returns the largest magnitude met."""
    x, xp = case.x.astype(np.float64), case.xp.astype(np.float64)
    n = x.shape[0]
    u, c = case.eps[:n].astype(np.float64), case.eps[n:].astype(np.float64)
    m1 = case.hist[(case.k - 1) % 2].reshape(x.shape).astype(np.float64)
    zc = case.noise[case.k % 2].reshape(x.shape).astype(np.float64)
    zp = case.noise[(case.k + 1) % 2].reshape(x.shape).astype(np.float64)
    big = [0.0]

    def exact(kind):
        def f(v):
            assert np.isfinite(v).all()
            assert np.array_equal(v.astype(kind).astype(np.float64), v), case.name
            big[0] = max(big[0], float(np.abs(v).max()))
            return v
        return f
    for operand in (u, c):
        exact(np.float16)(operand)                                # the inputs themselves are fp16 numbers
    xc, xq, m, P = _tree(case.row.astype(np.float64), u, c, x, xp, m1, zc, zp, exact(np.float16), exact(np.float32))
    assert set(P) >= {"d", "p", "e", "se", "t", "m"}
    for half in (True, False):                                    # the fp32 model computes the very same numbers
        got_c, got_q, hist = case.expected(half)
        assert np.array_equal(got_c.astype(np.float64), xc) and np.array_equal(got_q.astype(np.float64), xq), case.name
        assert np.array_equal(hist[case.k % 2].astype(np.float64), m.reshape(-1)), case.name
        assert np.array_equal(hist[(case.k + 1) % 2], case.hist[(case.k + 1) % 2])
    return big[0]


# ------------------------------------------------------------------------------------------------ P2: general cases
P2_SHAPE = (2, 4, 1056)


def p2_rows(steps=6, eta=1):
    """[(name, k, row)]: every row of the real ``steps``-step P2 / C2 table at cfg 4.5."""
    rows = make_solver().pec_rows(tau_window(eta), steps).numpy()
    return [("s%d_eta%s_k%d" % (steps, eta, k), k, rows[k].copy()) for k in range(steps)]


def p2_inputs(seed=40):
    """(eps [2n, C, inner], x, xp, hist [2, .], noise [2, .]) as float32 numpy."""
    n, C, inner = P2_SHAPE
    tot = n * C * inner
    f = lambda shape, s: gauss(shape, seed + s).astype(np.float32)   # noqa: E731
    return f((2 * n, C, inner), 0), f(P2_SHAPE, 1), f(P2_SHAPE, 2), f((2, tot), 3), f((2, tot), 4)


def run_table(solver, x, noise_steps, tau, steps, half):
    """The CPU model driven through pec_rows: what the fused route computes, without a GPU.  Returns ([x after loop step
    0 .. steps], model-input times seen)."""
    rows = solver.pec_rows(tau, steps).numpy()
    n = x.shape[0]
    shape3 = (n, x.shape[1], -1)
    xs = x.numpy().reshape(shape3)
    xp = xs.copy()
    hist = np.zeros((2, xs.size), dtype=np.float32)
    ring = np.full((2, xs.size), np.nan, dtype=np.float32)
    ts = solver.get_time_steps("time", solver.ns.T, 1.0 / solver.ns.total_N, steps)
    t_in, seen, mid = solver._t_val(ts[0]), [], [xs.reshape(x.shape)]
    for k in range(steps):
        ring[(k + 1) % 2] = noise_steps[k + 1].numpy().reshape(-1)
        xt = torch.from_numpy(xp.reshape(x.shape))
        seen.append(t_in)
        eps = solver.model(torch.cat([xt, xt]), torch.full((2 * n,), t_in, dtype=torch.float32), None)
        xs, xp, hist = reference_step(rows[k], eps.float().numpy().reshape(2 * n, x.shape[1], -1), xs, xp, hist, ring, k, half)
        if k > 0:
            mid.append(xs.reshape(x.shape))
        t_in = float(rows[k][T_NEXT])
    mid.append(xp.reshape(x.shape))
    return mid, seen

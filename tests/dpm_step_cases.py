"""Cases and a step-by-step CPU model for the fused DPM-Solver++ step (vq_cfg_dpmpp_step, csrc/sampler.hip).

reference_step evaluates ONE fused step in the operation order include/viditq.h documents, every operation rounded on
its own (numpy never contracts), with the four fp16 roundings of an fp16 model output.  Families:

D1 (exact)   operands are multiples of 2^-4 with |.| <= 8 that encode (batch half, b, c, inner position); cfg, the
             multipliers and the factors of the hand-made rows are powers of two.  d1_prove shows that every intermediate
             is exact in fp16 (where the eager path rounds to fp16) and in fp32, so the expected output does not depend on
             grouping, contraction or the form of the division; a wrong index, history slot, order branch or batch half is
             a wrong number.
D2 (general) Gaussian eps / x with rows of real 5- and 20-step schedules: first row, a middle row, the last row (where
             sigma_t and alpha_t are extreme).
D3 (shapes)  (n, C, inner) below, each with a dense model output and with the 2 * C * inner pitch of
             forward_with_dpmsolver's chunk(2, dim=1)[0] view.
"""
import numpy as np
import torch

ROW = 16
(ORDER, TAYLOR, CFG, SIGMA, ALPHA, INV_ALPHA, AX, BM, C1, C2, INV_R0, INV_R1, R0_FRAC, INV_R01, T_NEXT) = range(15)

# (1, 4, 1) / (2, 3, 7): one element per access, odd inner; (2, 4, 1024): four per access, several blocks;
# (5, 4, 65536): 1.3 M elements, a second pass of the 1024 x 256 x 4 grid; (1, 3, 100003): a second pass of the
# one-element form (1024 x 256 threads)
D3_SHAPES = [(1, 4, 1), (2, 3, 7), (2, 4, 1024), (5, 4, 65536), (1, 3, 100003)]


def _f16(v):
    return v.astype(np.float16).astype(np.float32)


def _tree(row, u, c, x, m1, m2, r16, r32, div_form):
    """The documented expression tree on arrays of one type; r16 / r32 are applied where the kernel rounds to fp16 / fp32.
    Returns (x_out, m_k, {name: intermediate})."""
    order, taylor = int(row[ORDER]), bool(row[TAYLOR] != 0)
    s = [x.dtype.type(v) for v in row]
    P = {}
    P["d"] = r16(c - u)
    P["p"] = r16(s[CFG] * P["d"])
    P["e"] = r16(u + P["p"])
    P["se"] = r16(s[SIGMA] * P["e"])
    P["t"] = r32(x - P["se"])
    if div_form == "divide":
        P["m"] = r32(P["t"] / s[ALPHA])
    else:
        assert div_form == "reciprocal"
        P["m"] = r32(P["t"] * s[INV_ALPHA])
    m = P["m"]
    P["ax"] = r32(s[AX] * x)
    P["bm"] = r32(s[BM] * m)
    o = P["o1"] = r32(P["ax"] - P["bm"])
    if order == 2:
        P["dm0"] = r32(m - m1)
        P["D1_0"] = r32(s[INV_R0] * P["dm0"])
        P["cd"] = r32(s[C1] * P["D1_0"])
        o = P["o2"] = r32(o + P["cd"]) if taylor else r32(o - P["cd"])
    elif order == 3:
        P["dm0"] = r32(m - m1)
        P["D1_0"] = r32(s[INV_R0] * P["dm0"])
        P["dm1"] = r32(m1 - m2)
        P["D1_1"] = r32(s[INV_R1] * P["dm1"])
        P["dd"] = r32(P["D1_0"] - P["D1_1"])
        P["fd"] = r32(s[R0_FRAC] * P["dd"])
        P["D1"] = r32(P["D1_0"] + P["fd"])
        P["D2"] = r32(s[INV_R01] * P["dd"])
        P["p2"] = r32(s[C1] * P["D1"])
        P["p3"] = r32(s[C2] * P["D2"])
        P["o2"] = r32(o + P["p2"])
        o = P["o3"] = r32(P["o2"] - P["p3"])
    else:
        assert order == 1
    return o, m, P


def reference_step(row, eps, x, hist, k, eps_half, div_form):
    """One fused step number k.  row: [ROW] fp32; eps: [2n, C, inner] (any float type: rounded to fp16 first when
    eps_half, else taken as fp32); x: [n, C, inner] fp32; hist: [3, n*C*inner] fp32.  Returns (x_out, hist_new)."""
    row = np.asarray(row, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    e = np.asarray(eps)
    e = _f16(e) if eps_half else e.astype(np.float32)
    u, c = e[:n].reshape(x.shape), e[n:].reshape(x.shape)
    hist = np.array(hist, dtype=np.float32, copy=True)
    m1 = hist[(k - 1) % 3].reshape(x.shape)
    m2 = hist[(k - 2) % 3].reshape(x.shape)
    ident = lambda v: v   # noqa: E731
    with np.errstate(all="ignore"):
        out, m, _ = _tree(row, u, c, x, m1, m2, _f16 if eps_half else ident, ident, div_form)
    assert out.dtype == np.float32 and m.dtype == np.float32
    hist[k % 3] = m.reshape(-1)
    return out, hist


# ------------------------------------------------------------------------------------------------ D1: exact cases
def _enc(shape, half, salt):
    """Multiples of 2^-4 in [-8, 8] that encode (half, b, c, inner position)."""
    n, C, inner = shape
    b = np.arange(n, dtype=np.int64)[:, None, None]
    ch = np.arange(C, dtype=np.int64)[None, :, None]
    j = np.arange(inner, dtype=np.int64)[None, None, :]
    v = (b * 37 + ch * 11 + j * 3 + half * 101 + salt * 53) % 257 - 128
    return (v.astype(np.float32) / 16.0)


def d1_row(order, taylor):
    """A hand-made row whose every scalar is a power of two (alpha_t = 1/2: its reciprocal is exactly 2)."""
    r = np.zeros(ROW, dtype=np.float32)
    r[ORDER], r[TAYLOR], r[CFG], r[SIGMA], r[ALPHA], r[INV_ALPHA] = order, float(taylor), 2.0, 0.5, 0.5, 2.0
    r[AX], r[BM], r[C1], r[C2] = 0.5, 0.25, 0.5, 0.25
    r[INV_R0], r[INV_R1], r[R0_FRAC], r[INV_R01], r[T_NEXT] = 2.0, 4.0, 0.5, 0.25, 750.0
    return r


class D1Case:
    def __init__(self, shape, order, taylor, k):
        self.shape, self.order, self.taylor, self.k = shape, order, taylor, k
        self.name = "n%d_C%d_i%d_o%d%s_k%d" % (*shape, order, "t" if taylor else "d", k)
        self.row = d1_row(order, taylor)
        n = shape[0]
        self.eps = np.concatenate([_enc(shape, 0, 0), _enc(shape, 1, 0)])            # [2n, C, inner]: uncond | cond
        self.x = _enc(shape, 0, 1)
        self.hist = np.stack([_enc(shape, 0, 2 + s).reshape(-1) for s in range(3)])  # three distinguishable slots
        assert self.eps.shape[0] == 2 * n


D1_KINDS = [(1, False), (2, False), (2, True), (3, False)]


def d1_cases(shapes=None):
    """Every order / solver type, with k walking through the three history slots."""
    out = []
    for si, shape in enumerate(shapes or D3_SHAPES):
        for oi, (order, taylor) in enumerate(D1_KINDS):
            out.append(D1Case(shape, order, taylor, k=order - 1 + (si + oi) % 3 + (3 if shape[2] == 7 else 0)))
    return out


def d1_prove(case):
    """Evaluates the tree in fp64 and shows that every intermediate already IS an fp16 number (the four values the eager
    path rounds to fp16) or an fp32 number (all others): each operation's exact result is its rounded result, with or
    without a contraction, and dividing by 1/2 equals multiplying by 2.  Returns the largest magnitude met."""
    x = case.x.astype(np.float64)
    n = x.shape[0]
    u, c = case.eps[:n].astype(np.float64), case.eps[n:].astype(np.float64)
    m1 = case.hist[(case.k - 1) % 3].reshape(x.shape).astype(np.float64)
    m2 = case.hist[(case.k - 2) % 3].reshape(x.shape).astype(np.float64)
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
    outs = []
    for form in ("divide", "reciprocal"):
        o, m, P = _tree(case.row.astype(np.float64), u, c, x, m1, m2, exact(np.float16), exact(np.float32), form)
        outs.append((o, m))
        assert set(P) >= {"d", "p", "e", "se", "t", "m", "ax", "bm", "o1"}
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    # ... and the fp32 model computes the very same numbers, with either eps type
    for half in (True, False):
        got, hist = reference_step(case.row, case.eps, case.x, case.hist, case.k, half, "reciprocal")
        assert np.array_equal(got.astype(np.float64), outs[0][0]), case.name
        assert np.array_equal(hist[case.k % 3].astype(np.float64), outs[0][1].reshape(-1)), case.name
    return big[0]


# ------------------------------------------------------------------------------------------------ D2: general cases
def make_solver(cfg_scale=4.5, model=None):
    import viditq_amd  # noqa: F401
    from viditq_amd.t2i.dpm_solver import DPMSolverPP
    y = torch.zeros(1, 1, 2, 4)
    return DPMSolverPP(model, y, y.clone(), cfg_scale)


def d2_rows():
    """[(name, k, row, (steps, order, solver_type, lower_order_final))]: first / middle / last rows of real 5- and
    20-step schedules, orders 1 - 3 and 'taylor'."""
    s = make_solver()
    out = []
    for steps in (5, 20):
        for order, st in ((2, "dpmsolver"), (3, "dpmsolver"), (2, "taylor"), (1, "dpmsolver")):
            rows = s.multistep_rows(steps, order, "time_uniform", None, None, True, st).numpy()
            for k in (0, steps // 2, steps - 1):
                out.append(("s%d_o%d_%s_k%d" % (steps, order, st, k), k, rows[k].copy(), (steps, order, st, True)))
            if order == 3:                                        # no lower_order_final: a third-order last row
                rows = s.multistep_rows(steps, order, "time_uniform", None, None, False, st).numpy()
                out.append(("s%d_o3_nolower_k%d" % (steps, steps - 1), steps - 1, rows[steps - 1].copy(),
                            (steps, order, st, False)))
    return out


def gauss(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).numpy()


# ------------------------------------------------------------------------------------------------ analytic models
def analytic_model(half, calls=None):
    """model(x2, t, y): a noise prediction that differs between the batch halves and moves with the model-input time;
    fp16 output when ``half`` (the four fp16 roundings of the eager path), else fp32."""
    def model(x2, t, y, **kw):
        if calls is not None:
            calls.append(t.detach().float().cpu().clone())
        n = x2.shape[0] // 2
        z = x2.half() if half else x2.float()
        g = (0.1 + t.to(z.dtype) / 20000.0).reshape(-1, *([1] * (z.dim() - 1)))
        f = torch.cat([torch.full((n,), 1.0, dtype=z.dtype, device=z.device),
                       torch.full((n,), 1.3, dtype=z.dtype, device=z.device)]).reshape(g.shape)
        return z * g * f
    return model


def run_table(solver, x, steps, order, lower_order_final, solver_type, half, div_form="divide"):
    """The CPU model driven through multistep_rows: what the fused route computes, without a GPU."""
    rows = solver.multistep_rows(steps, order, "time_uniform", None, None, lower_order_final, solver_type).numpy()
    ts = solver.time_steps("time_uniform", solver.ns.T, 1.0 / solver.ns.total_N, steps)
    n = x.shape[0]
    xs = x.numpy().reshape(n, x.shape[1], -1)
    hist = np.zeros((3, xs.size), dtype=np.float32)
    t_in = solver._t_val(ts[0])
    for k in range(steps):
        xt = torch.from_numpy(xs.reshape(x.shape))
        eps = solver.model(torch.cat([xt, xt]), torch.full((2 * n,), t_in, dtype=torch.float32), None)
        xs, hist = reference_step(rows[k], eps.float().numpy().reshape(2 * n, x.shape[1], -1), xs, hist, k, half, div_form)
        t_in = float(rows[k][T_NEXT])
    return torch.from_numpy(xs.reshape(x.shape))

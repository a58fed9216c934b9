"""Operands for the kernels that run OUTSIDE the 28 blocks whose output is known per element: the FP edge Linear
(vq_linear_f16, csrc/fp_linear.hip), the sampler update (vq_cfg_ddim_step, csrc/sampler.hip) and the AdaLN table
(vq_adaln_table, csrc/rowquant.hip).  For the kernel tests of test_fp_edge_exact_gpu.py and the CPU checks of
test_fp_edge_cases_cpu.py.  Every builder is plain torch on the CPU and seeded.

vq_linear_f16:  out[m, n] = half(act_out(sum_k half(act_in(x[m, k])) w[n, k] + b[n])), fp32 accumulation.
L1  address: one-hot rows x[m, k(m)] = v(m), k(m) = (a m + K - 1 + a M phase) mod K (row 0 of phase 0 meets K - 1, the
    last k of a partial k-step), v in +-{1, 2, 3}, w[n, k] an integer function of (n, k) with |w| <= 30 that differs
    between k and k ^ 8 and between n and n + 1: out[m, n] = v(m) w[n, k(m)], an integer below 2048, names (m, n, k).
L2  exact accumulation and the fp16 store: x = xi sx[m], w = wi sw[n] with integers |xi|, |wi| <= 8 and power-of-two
    scales that move with the index, bias a multiple of every q = sx[m] sw[n].  ``prove_exact`` shows in int64 that every
    product and every partial sum is a multiple of q below 2^24 q: exact in fp32 in ANY order, fused or not, so the
    expectation is exact.half(), bitwise.  ``l2_landing`` puts outputs on chosen values: column n of class (e, ct) has
    q = 2^e and bias ct q; row m is a pattern r[k] that every weight row cancels (r[2j] = -r[2j + 1], w[n, 2j] =
    w[n, 2j + 1] = z(j, n): partial sums up to 32 K q that end at 0) plus v(m) at k(m), so out = q (ct + v z) with v z
    from -24 to 24 - ties between fp16 neighbours of both parities (q = a quarter ulp of the bias), 65504 + 15 and + 16
    (-> 65504 and inf), 2^-25 (-> 0), 2^-24 and the ties between subnormals, 0 by cancellation from both signs.
L3  activation sweeps: all 63488 finite fp16 values as x [992, 64] against w = I_64, so that the accumulator is x itself
    (the other 63 products are exact zeros): act_in = SiLU gives half(silu(x)); act_out = SiLU / GELU(tanh) act on
    fl32(x + b[n]).  fp64 reference, bound = one fp16 ulp of the reference (floor 2^-24) + the formula's relative error
    (gemm_cases.G5_REL for GELU; SILU_REL below).
L4  pitches and frames: L1 / L2 operands inside arenas with row pitches ldx > K, ldw > K, ldo > N whose gap columns and
    rows beyond M / N hold NaN (the kernel clamps to row M - 1 / N - 1: it has no business reading them).

vq_cfg_ddim_step:
S1  exact: operands multiples of 2^-4 with |.| <= 8 that encode (b, c, inner), parameters whose every intermediate is
    exact (``s1_prove``), the unused sigma half of cond / uncond NaN.  Bitwise.
S2  general: Gaussian operands at schedule values from both ends; fp64 reference; per-element bound (``s2``).
S3  S1 operands at the shapes that reach the second pass of the grid-stride loop, C = 3 (no pass-through channel),
    C = 8 (five) and a single element.

vq_adaln_table:
A1  fp16 table and t0 with +-65504 against 2^-24 (the fp32 sum rounds) and 65504 + 65504: one IEEE add per element.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

import gemm_cases as gc

TWO24 = 2 ** 24
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
NAN = float("nan")

# (M, N, K): K <= 32 takes the kernel without the k split (four row tiles per workgroup: M = 17 and 65 leave waves that
# return at once, 130 is a third workgroup); K > 32 the split (504 / 512 / 520: one round of 16 k-steps less a step,
# exactly, and plus an 8-wide tail on wave 0; 40, 72, 136: tails of 8 on waves 1, 2 and 0)
NOSPLIT_SHAPES = [(1, 4, 8), (16, 12, 16), (17, 16, 24), (63, 20, 32), (64, 36, 8), (65, 4, 24), (130, 36, 32), (130, 20, 16)]
SPLIT_SHAPES = [(1, 4, 40), (2, 12, 72), (15, 16, 128), (16, 20, 136), (17, 36, 504), (77, 36, 512), (77, 36, 520),
                (2, 16, 1152), (77, 12, 4096), (17, 4, 520), (1, 36, 4096), (15, 20, 1152), (77, 36, 72), (77, 20, 40)]
LIN_SHAPES = NOSPLIT_SHAPES + SPLIT_SHAPES
L4_SHAPES = [(77, 36, 72), (130, 36, 32), (17, 16, 24), (77, 36, 520), (1, 4, 8), (15, 20, 1152), (65, 4, 24)]
L4_PITCHES = [(8, 16, 4), (24, 16, 12)]          # (ldx - K, ldw - K, ldo - N)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.as_tensor(e).double())


@dataclass
class Case:
    name: str
    family: str
    catches: str                        # what the family is there to catch
    M: int
    N: int
    K: int
    x: torch.Tensor                     # [M, K] fp16
    w: torch.Tensor                     # [N, K] fp16
    bias: Optional[torch.Tensor]        # [N] fp16
    act_in: int = ACT_NONE
    act_out: int = ACT_NONE
    exact: Optional[torch.Tensor] = None    # [M, N] fp64: the value before the fp16 store
    bound: Optional[torch.Tensor] = None    # [M, N] fp64 on |out - exact|; None: bitwise against expect_half()
    extra: dict = field(default_factory=dict)

    def expect_half(self):
        """exact.half() for the exact families: the fp64 value is an fp32 number, so one rounding."""
        e32 = self.exact.float()
        assert torch.equal(e32.double(), self.exact)
        return e32.half()


def _exact_case(name, family, catches, xi, wi, sx, sw, bi_q, extra=None):
    """x = xi sx[m], w = wi sw[n], bias = bi_q sw[n] max(sx) (None: no bias)."""
    M, K = xi.shape
    N = wi.shape[0]
    sx, sw = sx.double().expand(M).contiguous(), sw.double().expand(N).contiguous()
    x = (xi.double() * sx[:, None]).half()
    w = (wi.double() * sw[:, None]).half()
    b = None if bi_q is None else (bi_q.double() * sw * float(sx.max()))
    acc = (xi.double() @ wi.double().t())                   # integers far below 2^53: exact
    exact = acc * sx[:, None] * sw[None, :] + (0.0 if b is None else b[None, :])
    ex = dict(xi=xi.long(), wi=wi.long(), sx=sx, sw=sw)
    ex.update(extra or {})
    return Case(name, family, catches, M, N, K, x, w, None if b is None else b.half(), exact=exact, extra=ex)


def prove_exact(c: Case):
    """int64 proof that out of ``c`` is exact in fp32 however the products are grouped and summed.  Returns the largest
    sum of term magnitudes in units of q (<= 2^24)."""
    xi, wi, sx, sw = c.extra["xi"], c.extra["wi"], c.extra["sx"], c.extra["sw"]
    assert c.act_in == ACT_NONE and c.act_out == ACT_NONE
    assert gc.is_pow2(sx) and gc.is_pow2(sw)
    # the operands the kernel is given ARE xi sx and wi sw (fp16 holds them), normal numbers or zero
    assert torch.equal(c.x.double(), xi.double() * sx[:, None]) and torch.equal(c.w.double(), wi.double() * sw[:, None])
    for t in (c.x, c.w) + (() if c.bias is None else (c.bias,)):
        nz = t[t != 0].double().abs()
        assert nz.numel() == 0 or (float(nz.min()) >= 2.0 ** -14 and float(nz.max()) <= 65504.0)
    q = sx[:, None] * sw[None, :]
    if c.bias is None:
        bq = torch.zeros(c.M, c.N, dtype=torch.long)
    else:
        r = c.bias.double()[None, :] / q                    # exact: a power-of-two divisor
        assert torch.equal(r, r.round())                    # the bias is a multiple of every q
        bq = r.long()
    total = (xi.abs().double() @ wi.abs().double().t()).long() + bq.abs()
    assert int(total.max()) <= TWO24, (c.name, int(total.max()))
    assert torch.equal(c.exact, q * ((xi.double() @ wi.double().t()) + bq.double()))
    assert float(q.max()) * TWO24 < 2.0 ** 127 and float(q.min()) >= 2.0 ** -100       # every term a normal fp32 number
    assert torch.equal(c.exact.float().double(), c.exact)
    return int(total.max())


# --------------------------------------------------------------------------------------------------------------- L1
L1_V = (1, -1, 2, -2, 3, -3)


def l1_phases(M, K, cap=64):
    """Launches of M rows needed for k(m) to meet every k (capped: one row against K = 4096 would be 4096)."""
    return min((K + M - 1) // M, cap)


def l1_k(M, K, phase=0):
    m = torch.arange(M) + phase * M
    return (gc.g1_stride(K) * m + (K - 1)) % K


def l1_v(M, phase=0):
    m = torch.arange(M) + phase
    return torch.tensor(L1_V)[(m % 6)]


def l1_weights(N, K):
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    return (7 * n + 3 * k + 5 * (k // 8) + 11 * (k // 32) + 13 * (k // 128)) % 61 - 30


def l1(M, N, K, phase=0, bias=False):
    kk, v = l1_k(M, K, phase), l1_v(M, phase)
    xi = torch.zeros(M, K, dtype=torch.long)
    xi[torch.arange(M), kk] = v
    bi = ((torch.arange(N) * 5) % 11 - 5) if bias else None
    return _exact_case("l1_%dx%dx%d_p%d%s" % (M, N, K, phase, "_b" if bias else ""), "L1",
                       "a wrong row, column or k: clamps, the k tail, the deal of k-steps to waves, lane groups",
                       xi, l1_weights(N, K), torch.ones(1), torch.ones(1), bi, {"k": kk, "v": v})


# --------------------------------------------------------------------------------------------------------------- L2
def l2(M, N, K, seed=0, bias=True):
    g = _gen(1000 * seed + M + 3 * N + 7 * K)
    xi = torch.randint(-8, 9, (M, K), generator=g)
    wi = torch.randint(-8, 9, (N, K), generator=g)
    sx = _pow2(-((torch.arange(M) * 5) % 4))                 # 1 .. 2^-3, neighbours differ
    sw = _pow2(-(4 + (torch.arange(N) * 3) % 5))             # 2^-4 .. 2^-8
    bi = torch.randint(-1024, 1025, (N,), generator=g) if bias else None
    c = _exact_case("l2_%dx%dx%d%s" % (M, N, K, "_b" if bias else ""), "L2",
                    "a dropped or doubled term of the sum, a missing or shifted bias, a lossy accumulator",
                    xi, wi, sx, sw, bi)
    prove_exact(c)
    return c


# (e, ct): q = 2^e, bias = ct q.  Ties: ct = 4 mant with mant in [1024, 2047] - the bias is an fp16 number whose ulp is 4 q.
L2_CLASSES = [(-12, 4 * 1101), (-12, -4 * 1102), (-2, 4 * 1024), (-2, -4 * 2047), (-20, 4 * 1500), (0, 4 * 1301),
              (0, 65504), (0, -65504),                      # + 15 -> 65519 -> 65504; + 16 -> 65520 -> inf
              (-25, 0), (-25, 2048), (-25, -2048),          # 2^-25 -> 0, 2^-24, ties between subnormals
              (-6, 5), (-6, -5), (-9, 24), (-9, -24), (-14, 16)]     # 0 by cancellation from both signs
L2_SX = -12           # x = xi 2^-12 and w = wi 2^(e + 12): both normal fp16 numbers for every class


def l2_landing(M, N, K, classes=L2_CLASSES):
    assert K % 2 == 0
    kk = l1_k(M, K)
    m, n, j = torch.arange(M), torch.arange(N), torch.arange(K // 2)
    v = torch.tensor(L1_V)[(m + m // 6) % 6]
    a = (3 * j) % 4 + 1
    r = torch.stack([a, -a], 1).reshape(K)
    xi = r[None, :].repeat(M, 1)
    xi[m, kk] += v                                           # |xi| <= 7
    z = (5 * j[None, :] + 3 * (n[:, None] // len(classes)) + n[:, None]) % 17 - 8
    wi = z.repeat_interleave(2, dim=1)
    cls = n % len(classes)
    e = torch.tensor([c[0] for c in classes])[cls]
    ct = torch.tensor([c[1] for c in classes], dtype=torch.long)[cls]
    c = _exact_case("l2land_%dx%dx%d" % (M, N, K), "L2",
                    "a store that truncates or rounds half away, a flushed subnormal, a finite value for 65520",
                    xi, wi, _pow2(L2_SX), _pow2(e - L2_SX), ct, {"k": kk, "v": v, "cls": cls, "d": v[:, None] * z[:, kk // 2].t()})
    assert torch.equal(c.exact, _pow2(e)[None, :] * (ct[None, :] + c.extra["d"]).double())
    prove_exact(c)
    return c


def landing_census(cases):
    """How many outputs of ``cases`` land on each of the values the family is there for."""
    n = dict(tie_to_even_mantissa_up=0, tie_to_even_mantissa_down=0, max_65504=0, v65519=0, v65520_to_inf=0,
             two_m24=0, two_m25_to_zero=0, subnormal_tie=0, zero_from_positive_bias=0, zero_from_negative_bias=0)
    for c in cases:
        y = c.exact
        h = c.expect_half()
        hb = h.view(torch.int16).long() & 0xFFFF
        tie = (h.double() != y) & torch.isfinite(h)
        # a tie: y is half way between h and its other neighbour
        step = _pow2(torch.floor(torch.log2(h.double().abs().clamp(min=2.0 ** -14))) - 10)
        is_tie = tie & ((h.double() - y).abs() * 2 == step)
        up = is_tie & (h.double().abs() > y.abs())
        n["tie_to_even_mantissa_up"] += int(up.sum())
        n["tie_to_even_mantissa_down"] += int((is_tie & ~up).sum())
        assert bool((hb[is_tie] % 2 == 0).all())
        n["max_65504"] += int((y.abs() == 65504).sum())
        n["v65519"] += int((y.abs() == 65519).sum())
        n["v65520_to_inf"] += int(((y.abs() == 65520) & torch.isinf(h)).sum())
        n["two_m24"] += int((y.abs() == 2.0 ** -24).sum())
        n["two_m25_to_zero"] += int(((y.abs() == 2.0 ** -25) & (h == 0)).sum())
        n["subnormal_tie"] += int((is_tie & (h.double().abs() < 2.0 ** -14)).sum())
        bias = c.bias.double()[None, :].expand_as(y)
        n["zero_from_positive_bias"] += int(((y == 0) & (bias > 0)).sum())
        n["zero_from_negative_bias"] += int(((y == 0) & (bias < 0)).sum())
    return n


# --------------------------------------------------------------------------------------------------------------- L3
# relative error of the kernel's SiLU, y = v rcp(1 + exp2(w)), w = -log2(e) v - derived as gemm_cases.G5_REL:
#   w: the rounded constant and the product, 2^-24 each: |dw| <= 2 2^-24 |w|, and d(2^w) / 2^w = ln 2 dw <= ln 2 * 2 2^-24 *
#   126 (beyond |w| ~ 126 the exponential is 0 or inf and drops out); v_exp_f32 and v_rcp_f32: 1 ulp = 2^-23 each; 1 + e and
#   the final product: 2^-24 each.
SILU_REL = math.log(2) * 2 * 2.0 ** -24 * 126 + 2 * 2.0 ** -23 + 2 * 2.0 ** -24
L3_BIAS_NONE, L3_BIAS_MIXED = 0, 1


def all_finite_halves():
    """[992, 64]: bit patterns 0x0000 .. 0x7BFF, then 0x8000 .. 0xFBFF."""
    b = torch.cat([torch.arange(0, 0x7C00), torch.arange(0x8000, 0xFC00)]).to(torch.int32)
    assert b.numel() == 63488
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(torch.float16).reshape(992, 64)


def l3_bias(kind):
    if kind == L3_BIAS_NONE:
        return None
    n = torch.arange(64)
    return (((n * 7) % 13 - 6).double() * _pow2(-((n * 3) % 9))).half()      # 0 and +-2^-8 .. +-6: small mixed values


def silu_ref(v):
    v = v.double()
    return v / (1.0 + torch.exp(-v))


def silu_formula_fp32(v):
    """fpl_act<FPL_SILU> step by step in fp32 torch."""
    x = v.float()
    return x * (1.0 / (1.0 + torch.exp2(x * -1.4426950408889634)))


def act_ref(act, v):
    return v.double() if act == ACT_NONE else silu_ref(v) if act == ACT_SILU else gc.gelu_ref(v)


def act_formula_fp32(act, v):
    return v.float() if act == ACT_NONE else silu_formula_fp32(v) if act == ACT_SILU else gc.gelu_formula_fp32(v)


def act_bound(act, ref):
    """one fp16 ulp of the reference (floor 2^-24) + the formula's relative error."""
    if act == ACT_GELU:
        return gc.g5_bound(ref)
    assert act == ACT_SILU
    return gc.g5_bound(ref) + (SILU_REL - gc.G5_REL) * ref.abs()


def l3(act_in, act_out, bias_kind=L3_BIAS_NONE):
    """extra["v"]: the activation's fp32 argument per output (x, or fl32(x + b[n]): one IEEE add, the same on any
    hardware - the accumulator is x exactly)."""
    assert (act_in != ACT_NONE) != (act_out != ACT_NONE)
    x = all_finite_halves()
    b = l3_bias(bias_kind)
    if act_in != ACT_NONE:
        assert b is None
        v = x.float()
        act = act_in
    else:
        v = x.float() + (0.0 if b is None else b.float()[None, :])
        act = act_out
    ref = act_ref(act, v)
    return Case("l3_in%d_out%d_b%d" % (act_in, act_out, bias_kind), "L3",
                "an activation that is skipped, applied on the wrong side or a few fp32 ulps off; NaN or a wrong sign in the tails",
                992, 64, 64, x, torch.eye(64, dtype=torch.float16), b, act_in, act_out, ref, act_bound(act, ref),
                {"v": v, "act": act})


L3_CASES = [(ACT_SILU, ACT_NONE, L3_BIAS_NONE), (ACT_NONE, ACT_SILU, L3_BIAS_NONE), (ACT_NONE, ACT_SILU, L3_BIAS_MIXED),
            (ACT_NONE, ACT_GELU, L3_BIAS_NONE), (ACT_NONE, ACT_GELU, L3_BIAS_MIXED)]


def l3_sign_violations(out, c):
    """Tolerance-free: every output finite; act(+-0) = +-0 or +0; a non-zero output has its argument's sign."""
    v = c.extra["v"]
    o = out.float()
    bad = ~torch.isfinite(o)
    zero_in = v == 0
    bad |= zero_in & (o != 0)
    bad |= zero_in & ~torch.signbit(v) & torch.signbit(o)               # +0 never gives -0
    bad |= (o != 0) & (torch.signbit(o) != torch.signbit(v))
    return bad


# ------------------------------------------------------------------------------------------------ L4 and the reference
def arena(t, ld, extra_rows, fill=NAN):
    """[rows + extra_rows, ld] filled with ``fill``, ``t`` in its leading corner."""
    a = torch.full((t.shape[0] + extra_rows, ld), fill, dtype=t.dtype)
    a[:t.shape[0], :t.shape[1]] = t
    return a


LINEAR_MUTANTS = ("row_m1", "col_n1", "droptail", "dropwave", "kswap", "nobias", "bias_n1", "rtz", "act_skipped", "pitch")
LINEAR_MUTANT_FAMILY = {"row_m1": "L1", "col_n1": "L1", "droptail": "L1", "dropwave": "L1", "kswap": "L1", "nobias": "L2",
                        "bias_n1": "L2", "rtz": "L2", "act_skipped": "L3", "pitch": "L4"}


def _fragment(flat, rows, ld, K, nst):
    """[len(rows), nst, 4, 8] fp64: what lane row ``rows[i]`` loads in k-step s and lane group g - 8 consecutive halves at
    rows[i] ld + 32 s + 8 g, or zeros when that k is at or beyond K."""
    k = torch.arange(nst * 32)
    idx = rows[:, None] * ld + k[None, :]
    ok = (k < K)[None, :].expand_as(idx)
    vals = flat[torch.where(ok, idx, torch.zeros_like(idx))].double()
    return torch.where(ok, vals, torch.zeros_like(vals)).reshape(len(rows), nst, 4, 8)


def reference(c: Case, mutant=None, xa=None, wa=None):
    """out [M, N] fp64 before the store, recomputed the way fp_linear_kernel reads its operands: from flat arenas with
    their pitches (``xa`` / ``wa``; default: the dense operands), by 16 x 16 output tiles whose lane rows are clamped to
    M - 1 / N - 1, in 32-wide k-steps of four 8-wide lane groups, the k-steps dealt round-robin to four waves when K > 32
    (their sums added at the end), four row tiles per workgroup (a wave past M returns) when K <= 32.  ``mutant``: one
    wrong kernel (LINEAR_MUTANTS)."""
    M, N, K = c.M, c.N, c.K
    xa = c.x if xa is None else xa
    wa = c.w if wa is None else wa
    ldx, ldw = (K if mutant == "pitch" else xa.shape[1]), wa.shape[1]
    xf, wf = xa.reshape(-1), wa.reshape(-1)
    split = K > 32
    nst = (K + 31) // 32
    if mutant == "droptail" and K % 32:
        nst_used = nst - 1
    else:
        nst_used = nst
    mt, nt = (M + 15) // 16, (N + 15) // 16
    out = torch.full((M, N), NAN, dtype=torch.float64)
    bias = None if (c.bias is None or mutant == "nobias") else c.bias.double()
    act_in = ACT_NONE if mutant == "act_skipped" else c.act_in
    act_out = ACT_NONE if mutant == "act_skipped" else c.act_out
    lq = torch.arange(16)
    # w fragments once per column tile
    wfr = []
    for tn in range(nt):
        nr = (tn * 16 + lq).clamp(max=N - 1)
        if mutant == "col_n1":
            nr = torch.where(lq % 4 == 3, (nr + 1).clamp(max=N - 1), nr)
            if tn == nt - 1:
                nr = torch.where(tn * 16 + lq == N - 1, torch.full_like(nr, max(N - 2, 0)), nr)
        f = _fragment(wf, nr, ldw, K, nst)
        if mutant == "kswap":
            f = f[:, :, [1, 0, 3, 2], :]
        wfr.append(f)
    # K <= 32: row tile tm is wave tm % 4 of workgroup tm // 4 (the waves of the last workgroup whose tile would start at or
    # beyond M return: there is no such tm); K > 32: row tile tm is workgroup tm, whose four waves share the k-steps
    for tm in range(mt):
        m0 = tm * 16
        mr = (m0 + lq).clamp(max=M - 1)
        if mutant == "row_m1":
            mr = torch.where((lq == 15) | (m0 + lq == M - 1), (mr - 1).clamp(min=0), mr)
        xfr = _fragment(xf, mr, ldx, K, nst)
        if act_in != ACT_NONE:
            xfr = act_ref(act_in, xfr).half().double()   # rounded to fp16 before the contraction; act(0) = 0
        for tn in range(nt):
            acc = torch.zeros(16, 16, dtype=torch.float64)
            for wv in range(4 if split else 1):
                steps = [s for s in range(nst_used) if (s % 4 == wv if split else True)]
                if mutant == "dropwave" and split and wv == 3:
                    continue
                if steps:
                    a = xfr[:, steps].reshape(16, -1)
                    b = wfr[tn][:, steps].reshape(16, -1)
                    acc = acc + a @ b.t()
            y = acc
            if bias is not None:
                bn = (tn * 16 + lq).clamp(max=N - 1)
                if mutant == "bias_n1":
                    bn = torch.where(lq % 4 == 3, (bn + 1).clamp(max=N - 1), bn)
                    bn = torch.where(tn * 16 + lq == N - 1, torch.full_like(bn, max(N - 2, 0)), bn)
                y = y + bias[bn][None, :]
            y = y.float().double()                       # the fp32 accumulator (identity for the exact families)
            y = act_ref(act_out, y)
            mm, nn = min(16, M - m0), min(16, N - tn * 16)
            out[m0:m0 + mm, tn * 16:tn * 16 + nn] = y[:mm, :nn]
    return out


def reference_half(c, mutant=None, xa=None, wa=None):
    y = reference(c, None if mutant == "rtz" else mutant, xa, wa)
    return gc.rtz_half(y) if mutant == "rtz" else y.float().half()


def first_mismatch(bad, c: Case):
    """Name the first wrong element of a boolean [M, N] map by the kernel's own coordinates."""
    idx = torch.nonzero(bad)
    m, n = int(idx[0, 0]), int(idx[0, 1])
    s = "%d wrong of %d; first (m=%d, n=%d): tile (%d, %d), lane %d, element %d" % (
        idx.shape[0], bad.numel(), m, n, m // 16, n // 16, (n % 16 // 4) * 16 + m % 16, n % 4)
    if "k" in c.extra:
        k = int(c.extra["k"][m])
        s += ", k(m)=%d (k-step %d%s, lane group %d)" % (k, k // 32, ", wave %d" % (k // 32 % 4) if c.K > 32 else "", k % 32 // 8)
    return s


# ---------------------------------------------------------------------------------------------------------- sampler
@dataclass
class SCase:
    name: str
    family: str
    catches: str
    n: int
    C: int
    inner: int
    cond: torch.Tensor                  # [n, 2 C, inner] fp32
    uncond: torch.Tensor
    x: torch.Tensor                     # [n, C, inner] fp32
    cfg: float
    one_plus_k: float
    A: float
    Bc: float
    abar_prev: float
    exact: Optional[torch.Tensor] = None    # fp64 [n, C, inner]
    bound: Optional[torch.Tensor] = None    # None: bitwise against exact.float()

    def params(self):
        return self.cfg, self.one_plus_k, self.A, self.Bc, self.abar_prev


SAMPLER_MUTANTS = ("cfg_all_channels", "sigma_half", "no_k", "second_pass_missing", "cond_uncond_swapped")
SAMPLER_MUTANT_FAMILY = {"cfg_all_channels": "S1", "sigma_half": "S1", "no_k": "S1", "second_pass_missing": "S3",
                         "cond_uncond_swapped": "S1"}
FIRST_PASS = 4096 * 256                 # elements one pass of the grid-stride loop covers


def sampler_reference(s: SCase, mutant=None, dtype=torch.float64, parts=False):
    """x_out [n, C, inner] recomputed from the flat arrays with the kernel's index arithmetic, one line of cfg_ddim_kernel
    per line, every operation rounded to ``dtype`` (fp64 = exact for S1; no contraction).  ``parts``: also the
    intermediates."""
    n, C, inner = s.n, s.C, s.inner
    total = n * C * inner
    t = lambda v: torch.tensor(v, dtype=dtype)
    cfg, opk, A, Bc, abp = (t(float(torch.tensor(v, dtype=torch.float32))) for v in s.params())    # passed as fp32
    sa, sb = torch.sqrt(abp), torch.sqrt(t(1.0) - abp)
    i = torch.arange(total)
    in_ = i % inner
    c = (i // inner) % C
    b = i // (inner * C)
    mo = (b * 2 * C + c) * inner + in_
    if mutant == "sigma_half":
        mo = mo + C * inner
    cf, uf = s.cond.reshape(-1).to(dtype), s.uncond.reshape(-1).to(dtype)
    if mutant == "cond_uncond_swapped":
        cf, uf = uf, cf
    cv, uv = cf[mo], uf[mo]
    if mutant != "no_k":
        cv, uv = cv / opk, uv / opk
    d = cv - uv
    g = cfg * d
    guided = uv + g
    e = guided if mutant == "cfg_all_channels" else torch.where(c < 3, guided, cv)
    xv = s.x.reshape(-1).to(dtype)
    ax = A * xv
    be = Bc * e
    x0 = ax - be
    r = ax - x0
    e2 = r / Bc
    p1, p2 = x0 * sa, sb * e2
    out = p1 + p2
    if mutant == "second_pass_missing":
        out = torch.where(i < FIRST_PASS, out, torch.full_like(out, NAN))
    out = out.reshape(n, C, inner)
    if parts:
        return out, dict(cv=cv, uv=uv, d=d, g=g, guided=guided, ax=ax, be=be, x0=x0, r=r, e2=e2, p1=p1, p2=p2, c=c, sa=sa, sb=sb)
    return out


def _s_operands(n, C, inner):
    b = torch.arange(n)[:, None, None]
    i = torch.arange(inner)[None, None, :]
    c2 = torch.arange(2 * C)[None, :, None]
    c1 = c2[:, :C]
    cond = (((37 * b + 11 * c2 + 3 * i + 5 * (i // 61)) % 257 - 128).float() / 16).expand(n, 2 * C, inner).clone()
    unc = (((29 * b + 7 * c2 + 5 * i + 3 * (i // 53) + 64) % 257 - 128).float() / 16).expand(n, 2 * C, inner).clone()
    x = (((17 * b + 23 * c1 + 7 * i + (i // 47) + 100) % 257 - 128).float() / 16).expand(n, C, inner).clone()
    cond[:, C:] = NAN                   # the sigma half: never read
    unc[:, C:] = NAN
    return cond, unc, x


S1_PARAMS = [(cfg, opk, A, Bc, abp) for opk in (1.0, 2.0, 0.5) for cfg in (4.0, 7.5) for A in (1.0, 2.0, 1.5)
             for Bc in (0.5, 2.0) for abp in (1.0, 0.0)]
S3_SHAPES = [(5, 4, 65536), (1, 4, 1), (2, 3, 7), (2, 8, 1024)]


def s1(n, C, inner, params, family="S1"):
    cond, unc, x = _s_operands(n, C, inner)
    s = SCase("%s_%dx%dx%d_cfg%g_k%g_A%g_B%g_ap%g" % ((family.lower(), n, C, inner) + tuple(params)), family,
              "guidance on the wrong channels, the sigma half, a skipped 1 + k, swapped operands, elements no pass reaches",
              n, C, inner, cond, unc, x, *params)
    s.exact = sampler_reference(s)
    return s


def s1_prove(s: SCase):
    """Every intermediate of the fp64 evaluation is a multiple of 2^-10 below 2^13: 23 bits, exact in fp32 and fp64, so
    each operation's exact result is its rounded result - with or without contraction (a fused multiply-add rounds the
    same exact value once) - and both square roots are exact (abar_prev is 0 or 1)."""
    assert s.abar_prev in (0.0, 1.0)
    out, p = sampler_reference(s, parts=True)
    for name in ("cv", "uv", "d", "g", "guided", "ax", "be", "x0", "r", "e2", "p1", "p2"):
        v = p[name]
        assert bool(torch.isfinite(v).all()), name
        assert torch.equal(v * 1024, (v * 1024).round()) and float(v.abs().max()) < 2.0 ** 13, (s.name, name)
    assert torch.equal(p["r"], p["be"])                       # A x - x0 gives Bc e back
    assert bool(torch.isfinite(out).all()) and torch.equal(out.float().double(), out)
    return float(max(p[k].abs().max() for k in ("g", "guided", "be", "x0")))


S2_ABAR = [0.9999, 0.99, 0.9, 0.5, 0.05, 1e-3, 4.6e-5]
S2_PREV = [1.0, 0.9999, 0.99, 0.9, 0.5, 0.05, 1e-3]
S2_PARAMS = [(cfg, (0.8, 1.0, 1.37)[(i + j) % 3], (1.0 / ab) ** 0.5, (1.0 / ab - 1.0) ** 0.5, S2_PREV[i])
             for i, ab in enumerate(S2_ABAR) for j, cfg in enumerate((0.0, 1.0, 4.0, 7.0))]


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# Roundings on the longest path of cfg_ddim_kernel (16): cond / (1 + k), uncond / (1 + k) [2], cv - uv, cfg *, uv + [3],
# Bc e, A x, x0 = their difference [3], A x - x0 and the division by Bc [2], 1 - abar_prev, its square root and sb e2 [3],
# the square root of abar_prev, x0 sa and the final sum [3].  Each is at most 2^-24 of a magnitude bounded by T = |A x| +
# |Bc| E (E: the sum of the magnitudes that make e), carried to the output by sa (through x0) and sb / |Bc| (through e2).
S2_ROUNDINGS = 16


def s2(n, C, inner, params, seed=0):
    g = _gen(700 + seed)
    cond = torch.randn(n, 2 * C, inner, generator=g)
    unc = torch.randn(n, 2 * C, inner, generator=g)
    x = torch.randn(n, C, inner, generator=g)
    params = tuple(_f32(v) for v in params)
    s = SCase("s2_%dx%dx%d_cfg%g_k%.3g_A%.4g_B%.4g_ap%.4g" % ((n, C, inner) + params), "S2",
              "a formula that is rearranged into a lossier one; an error that only shows at one end of the schedule",
              n, C, inner, cond, unc, x, *params)
    out, p = sampler_reference(s, parts=True)
    cfg, opk, A, Bc, abp = params
    E = torch.where(p["c"] < 3, p["uv"].abs() + abs(cfg) * (p["cv"].abs() + p["uv"].abs()), p["cv"].abs())
    T = p["ax"].abs() + abs(Bc) * E
    s.exact = out
    s.bound = (S2_ROUNDINGS * 2.0 ** -24 * T * (p["sa"] + p["sb"] / abs(Bc))).reshape(n, C, inner)
    return s


# ------------------------------------------------------------------------------------------------------------ AdaLN
A1_SHAPES = [(2, 168, 1152), (1, 6, 1152), (3, 6, 8), (2, 12, 64)]


def a1(B, J, C, seed=0):
    """(table [J, C] fp16, t0 [B, J C] fp16, expected mod [J, B, C] fp32 = one IEEE fp32 add per element)."""
    g = _gen(900 + seed + B + J + C)
    table = torch.randn(J, C, generator=g).half()
    t0 = (torch.randn(B, J * C, generator=g) * 3).half()
    big, tiny = 65504.0, 2.0 ** -24
    plant = [(0, 0, big, tiny), (0, 1, -big, tiny), (0, 2, big, -tiny), (0, 3, tiny, -big), (J - 1, C - 1, big, big),
             (J - 1, C - 2, -big, -big), (J // 2, C // 2, big, -big), (J - 1, 0, tiny, tiny), (1, 4, 0.0, -tiny)]
    for j, c, tv, sv in plant:
        table[j, c] = tv
        t0[B - 1, j * C + c] = sv
    want = (table.float()[:, None, :] + t0.float().reshape(B, J, C).permute(1, 0, 2)).contiguous()
    assert want[0, B - 1, 0] == 65504.0 and want[J - 1, B - 1, C - 1] == 131008.0       # rounds; exceeds fp16
    return table, t0, want

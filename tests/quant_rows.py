"""Quantizer inputs whose rows sit where the shortcuts of csrc/vq_common.h could differ from the reference arithmetic
clamp(round_half_even(RN(x / delta)) + zp, 0, qmax): for the kernel tests of test_quantizer_edges_gpu.py and the CPU
checks of test_quant_rows_cpu.py.

Every builder is plain torch on the CPU, seeded, and returns x [B, n_tok, C] fp16 (grids are shared over B, as in the
reference: a "row" of the quantizer is the B * C values of one token).  Rows cycle through the family's values, so any C
(a multiple of 8) is filled.

Q1  exact ties: delta = 2^-k exactly (row range [lo d, hi d], hi - lo = qmax), every other value (m + 0.5) d.
Q2  near ties: Q1 rows behind a smoothing vector s = 1 + j 2^-23 (s = 1 on the channels of the row's min and max): x / s
    sits |m + 0.5| |j| 2^-23 from its tie, from 1e-6 to 1e-3, on both sides.
Q3  symmetric rows max = -min = m over the fp16 magnitudes: the true -min / delta is qmax / 2 = x.5.
Q4  one-sided rows [0, m] with m every fp16 value round qmax * 1e-6: the eps threshold straddled.
Q5  fp16 extremes: +-65504 together and alone, subnormals alone and beside one normal value, -0.0 entries.
Q6  a Gaussian row whose unique minimum / maximum sits at a chosen channel (and, for B = 2, in a chosen sample).
"""
import math

import torch

EPS = 1.0e-6
Q1_EXPONENTS = (0, 4, 8)        # delta = 2^-k; every value (2m + 1) 2^-(k+1), |2m + 1| <= 511, is an fp16 number
Q2_S1_LO, Q2_S1_HI = 3, -5      # channels of the row minimum / maximum of Q1 rows built with fixed=True (s = 1 there)
BOUND, GUARD = 5.3e-5, 1.0e-4   # vq_common.h: the claimed error of fma(x, inv, zp) and the tie guard 0.5 - 0.4999
Q2_BAND_MIN = 32                # elements per row in each of the three bands (1e-6, BOUND), [BOUND, GUARD), [GUARD, 1e-3)
Q4_WINDOW = {8: (2.4e-4, 2.7e-4), 6: (5.9e-5, 6.7e-5)}
Q6_VALUE = 9.0                  # the planted extremum; the Gaussian interior is clamped to +-6


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def fp16_positive():
    """Every positive finite fp16 value, ascending (31743 of them, subnormals first)."""
    return torch.arange(1, 0x7C00, dtype=torch.int32).to(torch.int16).view(torch.float16)


def q1_variants(n_bits):
    """(lo, hi) of the integer range of a row: zero point -lo odd, even, 0 and qmax."""
    qmax = 2 ** n_bits - 1
    h = qmax // 2
    return [(-h, h + 1), (-h - 1, h), (0, qmax), (-qmax, 0)]


def q1_row_spec(t, n_bits):
    """Token t of a Q1 launch: (lo, hi, k)."""
    var = q1_variants(n_bits)
    return var[t % 4] + (Q1_EXPONENTS[(t // 4) % 3],)


def q1(B, n_tok, C, n_bits, seed=0, fixed=False):
    """Exact ties.  Token t has range [lo, hi] * 2^-k (q1_row_spec); its B * C values are lo d, hi d and the ties
    (m + 0.5) d, m cycling through lo .. hi - 1 from a start that moves with t (so both parities of m are in every row
    and every m is met over the tokens).  The minimum / maximum sit at a channel and sample that move with t, or - with
    ``fixed`` (Q2) - at channels Q2_S1_LO / Q2_S1_HI of sample 0 / B - 1."""
    x = torch.empty(B, n_tok, C, dtype=torch.float64)
    ar = torch.arange(B * C)
    for t in range(n_tok):
        lo, hi, k = q1_row_spec(t, n_bits)
        d = 2.0 ** -k
        m = lo + (ar + 37 * t) % (hi - lo)
        row = ((m.double() + 0.5) * d).reshape(B, C)
        if fixed:
            p_lo, p_hi = (0, Q2_S1_LO % C), (B - 1, Q2_S1_HI % C)
        else:
            a, b = (11 * t) % (B * C), (11 * t + 1 + (7 * t) % (B * C - 1)) % (B * C)
            p_lo, p_hi = divmod(a, C), divmod(b, C)
        row[p_lo] = lo * d
        row[p_hi] = hi * d
        x[:, t] = row
    h = x.half()
    assert torch.equal(h.double(), x)                      # every value is an fp16 number
    return h


def q2_smooth(C, seed=0):
    """s [C] fp32 = 1 + j_c 2^-23 with j_c signed and log-spaced over 1 .. 2^11 (shuffled over the channels), 1 on the two
    channels that hold the minimum / maximum of q1(..., fixed=True) rows.  (1 - 2^-23 and every other value here has a
    significand that is not all ones: vq_smooth_reciprocal accepts the vector.)"""
    g = _gen(1000 + seed)
    mag = torch.round(2.0 ** (torch.arange(C).double() * (11.0 / max(1, C - 1)))).long()
    j = mag * (1 - 2 * (torch.arange(C) % 2))
    j = j[torch.randperm(C, generator=g)]
    j[Q2_S1_LO % C] = 0
    j[Q2_S1_HI % C] = 0
    s = (1.0 + j.double() * 2.0 ** -23).float()
    assert torch.equal(s.double(), 1.0 + j.double() * 2.0 ** -23)
    return s


def q3_magnitudes(stride=7):
    """Every ``stride``-th positive finite fp16 value (4535 for stride 7)."""
    return fp16_positive()[::stride]


def q3(B, C, mags, seed=0):
    """Symmetric rows: token t has max = +mags[t], min = -mags[t] (at channels and samples that move with t), the rest
    uniform in [-m, m] rounded to fp16."""
    g = _gen(2000 + seed)
    n = mags.numel()
    m = mags.double().reshape(1, n, 1)
    x = ((torch.rand(B, n, C, generator=g, dtype=torch.float64) * 2 - 1) * m).half()
    x = torch.minimum(torch.maximum(x, -mags.reshape(1, n, 1)), mags.reshape(1, n, 1))
    t = torch.arange(n)
    a, b = (13 * t) % (B * C), (13 * t + 1 + (5 * t) % (B * C - 1)) % (B * C)
    x[a // C, t, a % C] = mags
    x[b // C, t, b % C] = -mags
    return x


def q4_magnitudes(n_bits=8):
    lo, hi = Q4_WINDOW[n_bits]
    h = fp16_positive()
    return h[(h.double() > lo) & (h.double() < hi)]


def q4(B, C, n_bits=8, seed=0):
    """One-sided rows [0, m], m every fp16 value of Q4_WINDOW (143 at 8 bits): delta = m / qmax straddles 1e-6."""
    g = _gen(4000 + seed)
    mags = q4_magnitudes(n_bits)
    n = mags.numel()
    x = (torch.rand(B, n, C, generator=g, dtype=torch.float64) * mags.double().reshape(1, n, 1)).half()
    x = torch.minimum(x, mags.reshape(1, n, 1))
    t = torch.arange(n)
    a, b = (17 * t) % (B * C), (17 * t + 1 + (3 * t) % (B * C - 1)) % (B * C)
    x[a // C, t, a % C] = mags
    x[b // C, t, b % C] = 0.0
    return x


Q5_ROWS = ("both_65504", "both_65504_small_interior", "pos_65504", "neg_65504", "subnormals", "subnormals_neg",
           "normal_and_subnormals", "neg_normal_and_subnormals", "minus_zeros", "minus_zeros_and_one", "max_subnormal_pair",
           "min_normal_pair")
Q5_FLAGGED = {8: ("subnormals", "subnormals_neg", "max_subnormal_pair", "min_normal_pair"),     # rows with delta < 1e-6
              6: ("subnormals_neg",)}


def q5(B, C, seed=0):
    """fp16 extremes, one token per name of Q5_ROWS."""
    g = _gen(5000 + seed)
    big, sub, tiny = 65504.0, 2.0 ** -24, 2.0 ** -14
    n = len(Q5_ROWS)
    u = torch.rand(B, n, C, generator=g, dtype=torch.float64)
    sgn = u * 2 - 1
    subs = torch.randint(1, 1024, (B, n, C), generator=g).double() * sub            # every subnormal magnitude
    x = torch.zeros(B, n, C, dtype=torch.float64)
    for i, name in enumerate(Q5_ROWS):
        if name == "both_65504":
            r = sgn[:, i] * big
        elif name == "both_65504_small_interior":
            r = sgn[:, i] * 3.0
        elif name == "pos_65504":
            r = u[:, i] * big
        elif name == "neg_65504":
            r = -u[:, i] * big
        elif name == "subnormals":
            r = subs[:, i] * torch.sign(sgn[:, i])
        elif name == "subnormals_neg":
            r = -subs[:, i]
        elif name in ("normal_and_subnormals", "neg_normal_and_subnormals"):
            r = subs[:, i] * torch.sign(sgn[:, i])
        elif name in ("minus_zeros", "minus_zeros_and_one"):
            r = sgn[:, i] * 2.0
        else:
            r = torch.zeros(B, C, dtype=torch.float64)
        x[:, i] = r
    x = x.half()
    i = Q5_ROWS.index
    x[0, i("both_65504"), 5 % C], x[B - 1, i("both_65504"), C - 2] = big, -big
    x[B - 1, i("both_65504_small_interior"), 0], x[0, i("both_65504_small_interior"), C - 1] = big, -big
    x[0, i("pos_65504"), C // 2] = big
    x[:, i("pos_65504"), 1] = 0.0
    x[B - 1, i("neg_65504"), C // 2 - 1] = -big
    x[0, i("normal_and_subnormals"), 9 % C] = 1.0
    x[B - 1, i("neg_normal_and_subnormals"), C - 8] = -0.5
    x[:, i("minus_zeros"), ::3] = -0.0
    x[:, i("minus_zeros_and_one")] = -0.0
    x[0, i("minus_zeros_and_one"), 7 % C] = 1.0
    x[0, i("max_subnormal_pair"), 0], x[B - 1, i("max_subnormal_pair"), C - 1] = 1023 * sub, -1023 * sub
    x[0, i("min_normal_pair"), C - 1], x[B - 1, i("min_normal_pair"), 0] = tiny, -tiny
    return x


def q6_positions(C):
    """Channels where the extremum is planted: 0, 7, C - 1, the first channel of the second half of the row, the last of
    the first half, and the two sides of a lane's 8-channel group."""
    return [0, 7, C - 1, C // 2, C // 2 - 1, 8, C - 8]


def q6_specs(B, C):
    """(which, channel, sample of the planted extremum, sample of the other extremum)."""
    out = []
    for p in q6_positions(C):
        for which in ("min", "max"):
            for sb in range(B):
                out.append((which, p, sb, B - 1 - sb))
                if B > 1:
                    out.append((which, p, sb, sb))
    return out


def q6(B, C, seed=0):
    """Gaussian rows (sd 2, clamped to +-6) with the unique minimum -Q6_VALUE and maximum +Q6_VALUE planted per q6_specs;
    the other extremum sits at a channel that moves with the token."""
    g = _gen(6000 + seed)
    specs = q6_specs(B, C)
    n = len(specs)
    x = (torch.randn(B, n, C, generator=g) * 2.0).clamp(-6.0, 6.0).half()
    for t, (which, p, sb, so) in enumerate(specs):
        po = (p + 1 + (29 * t) % (C - 1)) % C
        v = -Q6_VALUE if which == "min" else Q6_VALUE
        x[sb, t, p] = v
        x[so, t, po] = -v
    return x


Q4U_CHANNELS = (40, 41, 42)


def q4u_scales(n_bits):
    """Three fp32 smoothing scales S with RN(RN(1 / S) / qmax) = the fp32 number just below 1e-6, 1e-6 itself and the one
    just above (found by walking the neighbours of 1 / (qmax * 1e-6); all three are normal numbers with plain
    significands): no fp16 row reaches the threshold to the ulp, a smoothed one does."""
    e = torch.tensor(EPS, dtype=torch.float32)
    qmax = torch.tensor(float(2 ** n_bits - 1))
    out = []
    for target in (torch.nextafter(e, torch.tensor(0.0)), e, torch.nextafter(e, torch.tensor(1.0))):
        up = dn = (1.0 / (target.double() * qmax.double())).float()
        found = None
        for _ in range(400):
            for cand in (up, dn):
                if found is None and float((torch.tensor(1.0) / cand) / qmax) == float(target):
                    found = cand
            up, dn = torch.nextafter(up, torch.tensor(math.inf)), torch.nextafter(dn, torch.tensor(0.0))
        assert found is not None
        out.append(float(found))
    return out


def q4u_vector(s, n_bits):
    """A copy of the smoothing vector s with q4u_scales() on Q4U_CHANNELS."""
    s = s.clone()
    for c, v in zip(Q4U_CHANNELS, q4u_scales(n_bits)):
        s[c] = v
    return s


def q4u(B, C):
    """Three tokens for a q4u_vector(): 1.0 on one of Q4U_CHANNELS (sample 0), +0 elsewhere - one-sided rows whose delta
    behind the vector is 1e-6 to the ulp: one below (flagged), equal and one above (both clean: the test is delta < 1e-6)."""
    x = torch.zeros(B, 3, C, dtype=torch.float16)
    for i, c in enumerate(Q4U_CHANNELS):
        x[0, i, c] = 1.0
    return x


# ----------------------------------------------------------------------------- reference views (the oracle only)
def smoothed(x, s=None):
    """The quantizer's fp32 input: x, or the IEEE quotients x / s."""
    xf = x.float()
    return xf if s is None else xf / s


def row_deltas(x, n_bits, s=None):
    """The oracle's own delta per token BEFORE any eps fill: [n_tok] fp32."""
    xf = smoothed(x, s)
    B, n, C = xf.shape
    r = xf.permute(1, 0, 2).reshape(n, B * C)
    lo = r.min(-1).values.clamp(max=0.0)
    hi = r.max(-1).values.clamp(min=0.0)
    return (hi - lo) / (2 ** n_bits - 1)


def split_eps(x, n_bits, s=None):
    """Token indices (good, flagged): delta >= 1e-6 / delta < 1e-6 by the oracle's own fp32 delta."""
    d = row_deltas(x, n_bits, s)
    small = d < EPS
    return (~small).nonzero()[:, 0], small.nonzero()[:, 0]


def tie_distance(x, n_bits, s=None):
    """fp64 distance of x / s / delta from the nearest half-integer, delta the oracle's fp32 one: [B, n_tok, C]."""
    d = row_deltas(x, n_bits, s).double().reshape(1, -1, 1)
    q = x.double() / (1.0 if s is None else s.double()) / d
    return ((q - torch.floor(q)) - 0.5).abs()


def families(B, C, n_bits, q3_stride=7, seed=0, fixed=False, ulp=False):
    """{name: x} of every family at this shape (Q1 with 48 tokens: each variant at each exponent four times; ``ulp``: plus
    the q4u() rows, for a launch behind a q4u_vector())."""
    fam = {"Q1": q1(B, 48, C, n_bits, seed, fixed=fixed), "Q3": q3(B, C, q3_magnitudes(q3_stride), seed),
           "Q4": q4(B, C, n_bits, seed), "Q5": q5(B, C, seed), "Q6": q6(B, C, seed)}
    if ulp:
        fam["Q4u"] = q4u(B, C)
    return fam


def launch_sets(B, C, n_bits, s=None, q3_stride=7, seed=0, fixed=False, n_flagged=4, ulp=False):
    """What one route of test_quantizer_edges_gpu.py runs at one shape.  Returns (exact, flagged, names):
    exact   x [B, n, C]: every family's rows whose oracle delta (behind ``s``) is >= 1e-6, concatenated along n_tok and
            made odd in length - one launch that must come back with status 0 and bit-exact;
    flagged a list of x [B, 65, C]: rows of ``exact`` plus ONE row with delta < 1e-6 in the middle - the
            ``n_flagged`` Q4 rows nearest the threshold, the largest and the smallest flagged Q3 row, and every flagged Q5
            (and Q4u) row;
            each launch must set VQ_ST_EPSFILL;
    names   the family of every token of ``exact``."""
    fam = families(B, C, n_bits, q3_stride, seed, fixed, ulp)
    good, names, flagged_rows = [], [], []
    for name, x in fam.items():
        gi, fi = split_eps(x, n_bits, s)
        good.append(x[:, gi])
        names += [name] * int(gi.numel())
        if fi.numel() == 0:
            continue
        d = row_deltas(x, n_bits, s)[fi]
        order = fi[torch.argsort(d, descending=True)]              # nearest the threshold first
        pick = order[:n_flagged] if name == "Q4" else order[:1] if name == "Q3" else order
        if name == "Q3":
            pick = torch.cat([pick, order[-1:]])                   # and the smallest magnitude (one fp16 subnormal step)
        flagged_rows += [x[:, i:i + 1] for i in pick.tolist()]
    exact = torch.cat(good, 1)
    if exact.shape[1] % 2 == 0:
        exact = torch.cat([exact, exact[:, :1]], 1)
        names.append(names[0])
    filler = exact[:, torch.linspace(0, exact.shape[1] - 1, 64).long()]
    flagged = [torch.cat([filler[:, :32], r, filler[:, 32:]], 1) for r in flagged_rows]
    return exact.contiguous(), flagged, names


def thin(x, n_tok):
    """``n_tok`` tokens of x, evenly spaced (every family of a launch_sets() launch stays represented)."""
    return x[:, torch.linspace(0, x.shape[1] - 1, n_tok).long()].contiguous()


def static_rows(B, n_tok, C, n_bits, per_token, seed=0):
    """Q1 rows for a static grid, with values outside the grid so that both clamps act.  Returns x, delta [n], zp [n]
    (n = n_tok, or 1 when the launch has one grid: then every row is of q1_row_spec(0))."""
    if per_token:
        x = q1(B, n_tok, C, n_bits, seed)
        spec = [q1_row_spec(t, n_bits) for t in range(n_tok)]
    else:
        x = q1(B, 4 * 3 * n_tok, C, n_bits, seed)[:, ::12].contiguous()       # tokens 0, 12, 24, ...: all of one spec
        spec = [q1_row_spec(0, n_bits)] * n_tok
    for t, (lo, hi, k) in enumerate(spec):
        d = 2.0 ** -k
        # beyond both ends: just past the last tie (lo - 0.5 and hi + 0.5 are ties themselves), far out, and fp16's largest
        x[0, t, (3 * t + 2) % C] = (lo - 0.5) * d
        x[B - 1, t, (3 * t + 9) % C] = (hi + 0.5) * d
        x[0, t, (3 * t + 17) % C] = (lo - 40) * d
        x[B - 1, t, (3 * t + 30) % C] = (hi + 300.5) * d
        x[0, t, (3 * t + 41) % C] = 65504.0 if t % 2 else -65504.0
    delta = torch.tensor([2.0 ** -k for _, _, k in spec], dtype=torch.float32)
    zp = torch.tensor([float(-lo) for lo, _, _ in spec], dtype=torch.float32)
    return (x, delta, zp) if per_token else (x, delta[:1], zp[:1])


def one_hot_qk(n, T, H, D, scale, seed):
    """Queries and keys of one-hot temporal attention whose hot key is the SAME for every head of a query row (so that
    the output row is one whole V row): q, k [n, T, H, D] fp16 and hot [n, T] (a permutation of the keys per sequence).
    Built from attn_regimes' nearly orthogonal keys and score constants."""
    import attn_regimes as ar
    g = _gen(seed)
    lam = ar.R1_SCORE / (D * scale * ar.LOG2E)
    q = torch.zeros(n, T, H, D, dtype=torch.float64)
    k = torch.zeros(n, T, H, D, dtype=torch.float64)
    hot = torch.zeros(n, T, dtype=torch.long)
    for s in range(n):
        hot[s] = (torch.arange(T) * (3 if T % 3 else 5 if T % 5 else 7) + s) % T
        for h in range(H):
            k[s, :, h] = ar._unit_keys(T, D, g)
            q[s, :, h] = lam * k[s, hot[s], h]
    return q.half(), k.half(), hot


def ulp_step(v, up):
    """fp32 v moved by one ulp towards +inf (up) or -inf."""
    return torch.nextafter(v, torch.full_like(v, math.inf if up else -math.inf))


# ----------------------------------------------------------------------------- LayerNorm + modulate in front of the quantizer
LN_FAMILIES = ("Q3", "Q5", "Q6")


def ln_inputs(name, B, C, seed=0):
    """x [B, n, C] fp16 of one family plus AdaLN shift / scale [B, C] fp32 (N(0, 0.3^2), fp16 values) for the
    LayerNorm + modulate + quantizer kernels.  Exact ties cannot be placed behind a LayerNorm computed on the GPU, so only
    Q3 / Q5 / Q6 come here; rows whose modulated activation the oracle would eps-fill (a constant row, a row of
    subnormals: LayerNorm's own eps keeps them tiny) are left out."""
    import torch.nn.functional as F
    g = _gen(7000 + seed)
    x = {"Q3": lambda: q3(B, C, q3_magnitudes(49), seed), "Q5": lambda: q5(B, C, seed), "Q6": lambda: q6(B, C, seed)}[name]()
    shift = (torch.randn(B, C, generator=g) * 0.3).half().float()
    scale = (torch.randn(B, C, generator=g) * 0.3).half().float()
    xm = F.layer_norm(x.float(), (C,), None, None, 1e-6) * (1 + scale[:, None, :]) + shift[:, None, :]
    good = (row_deltas(xm, 8) >= 10 * EPS).nonzero()[:, 0]
    return x[:, good].contiguous(), shift, scale

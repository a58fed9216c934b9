"""GELU(tanh) in front of fc2's per-token quantizer (rq_gelu_tanh of csrc/rowquant_shared.h at every call site), pinned over
all 63 488 finite fp16 inputs: the fp64 reference, the error model of the kernel's fp32 evaluation, the rows that make a
one-ulp error of the fp16 GELU value visible in the int8 codes, the expectation and the checker - for
test_gelu_rowquant_exact_gpu.py (the kernels) and test_gelu_cases_cpu.py (the properties claimed below, that wrong GELUs fail
and that a correct fp32 evaluation cannot).  numpy / torch on the CPU; imports no GPU code.

Reference.  g64(x) = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) in fp64 for every finite fp16 x, evaluated in the
identical form x / (1 + exp(-2u)) (0.5 (1 + tanh u) = 1 / (1 + exp(-2u)); the tanh form cancels for x < -3).  g_rn(x) is its
correctly rounded fp16 value; both fp16 neighbours are kept, and the two rounding boundaries around g_rn.

Error model.  The kernel computes, on fp32 copies of the fp16 x (u = 2^-24, W = x (C2 + C1 x^2) the true exponent,
C2 = -2 sqrt(2/pi) log2(e), C1 = 0.044715 C2, so that g = x / (1 + 2^W)):
  c2 = fl(-2.302208198), c1 = fl(fl(-0.044715) fl(2.302208198))   |dc2| <= u, |dc1| <= 3u (two literals and a product; the
                                                                  decimal 2.302208198 is within 5e-11 of C2: inside 3u - the
                                                                  CPU test measures both constants against these bounds)
  xx = x x                        exact: 22 significant bits
  p  = fma(xx, c1, c2)            both terms negative, no cancellation: |dp| <= 3u + u
  w  = x p                        |dw / W| <= 5u
  e  = v_exp_f32(w)               1 ulp = 2u, and 2^(w - W) - 1 = ln 2 |W| 5u through the exponent: |de| <= 2u + 5 ln 2 |W| u
  d  = 1 + e                      both positive: |dd| <= sigma |de| + u, sigma = 2^W / (1 + 2^W)
  r  = v_rcp_f32(d)               1 ulp: 2u
  g  = x r                        u
so the fp32 value before the conversion to fp16 is g64 (1 + t), |t| <= E(x) = (4 + sigma (2 + 5 ln 2 |W|)) 2^-24 to first
order: 3.6e-7 at most for x > 0, 6.0e-6 at x = -5.29 (W = 27.4, the last input whose GELU is not -0), far less than that
for most inputs.  Past W = 126 e overflows or r is flushed: the kernel's value is -0 or below 2^-120 in size where g64 is
below 2^-120 too - the margin carries 2^-100 absolute for it.
The margin is FACTOR E |g64| + 2^-100 with FACTOR = 4 as in ln_cases.py (second-order terms, an exp / rcp of 2 ulp).  An
input is PINNED when g64 is farther than the margin from both boundaries: the kernel's fp16 GELU must be g_rn exactly.  An
unpinned input has two admissible values, g_rn and the neighbour across the near boundary.

Rows.  Codes are the only observable, and the oracle's grid always contains zero, so the step is at least |extreme| / qmax:
the choice of the row's extreme - the ANCHOR, a pinned input whose output is the row's max (rows of positive outputs) or min
(rows of negative outputs; the signs never share a row) - decides which elements sit next to a rounding tie of the grid.
For an output of size v and an anchor of size M in [v, 2v] the fraction of v / fl(M / qmax) moves with M; plan() covers,
greedily over the pinned anchors of each binade of M (largest binade first), every output size with one anchor under
which its larger neighbour takes another oracle code than v itself and one under which its smaller neighbour does (the
two placements of an input).  An input may sit under an anchor only if neither of its admissible values exceeds it.
Inputs no anchor resolves are appended to an anchor above them, so that every input is met.  Sizes below the smallest
anchor the oracle does not eps-fill (step >= 1e-6), and with them every input of |g_rn| <= the FINE anchor - +-0,
subnormals, the large negative inputs whose GELU is -0 or subnormal - go under the fine anchor, the largest one whose step
is below 2e-6: the finest grid there is; their condition is coverage and finiteness.  (The one-ulp condition is claimed
from |g_rn| = 2^-9 up, SENS_MIN; the fine anchor lies below it - 5.1e-4 at 8 bits, 1.26e-4 at 6 - and the sizes in between
are planned with the one-ulp placements like the rest.)
rows(): a placement's inputs are dealt into rows of C - 1 (C = 4608: 511, so that every input also fills one of the 512
columns of the split kernel's 4-wide tail chunk, a call site of its own) and repeated to the width, the anchor's lane
cycles through anchor_lanes() (first / last chunk, both sides of the middle of the row and of a 512-channel chunk);
B = 2: both samples of a token hold the inputs, in opposite lane orders, the anchor in sample token % 2.

Expectation: the oracle's fq.dyn_act_quant of the fp32 copy of the g_rn rows (divided by s where given).  check() holds
sx, zx (zpf) bit for bit on every row, the codes bit for bit on every pinned element, one of the two admissible values'
oracle codes on an unpinned one, R to the kernel's own codes and - on rows without unpinned elements - to the oracle's,
zero pads, status 0, finite steps.  Nothing else is excused.

Figures (test_gelu_cases_cpu.py prints them; FACTOR 4):
  constants                    |dc1| = 0.89 u, |dc2| = 0.09 u;  E at most 6.01e-6 (x = -5.285, W = 27.4), 3.5e-7 for x > 0;
                               the fp32 emulation with exp2 / rcp within 1 ulp stays within 0.83 E
  unpinned inputs              185 of 63488 (0.29 %; a flat relative margin of 1e-5 would leave 1.77 %, 2e-5 3.59 %)
  8 bits: one-ulp sensitivity  positive 99.97 %, negative 98.41 % of the inputs with |g_rn| >= 2^-9;  805 placements
  6 bits: one-ulp sensitivity  positive 99.90 %, negative 96.57 %;                                   2892 placements
                               (what stays unresolved on the negative side lies above 0.15 in size: GELU's minimum is
                               -0.17, hundreds of inputs share the few output values next to it and no anchor lies beyond)
  tokens per launch, 8 bits    C = 4608: 860, C = 4600: 810, C = 1152: 826, C = 320: 907 (rows: twice that at B = 2)
  tokens per launch, 6 bits    C = 4608: 2932, C = 4600: 2895, C = 1152: 2909
  g_rn one ulp off at ONE input (400 sampled, through the oracle quantizer and check()): 399 caught at 8 bits, C = 320;
                               398 at 6 bits, B = 2, C = 1152
Generation: tables 0.1 s, plan 1 s per code width, rows under 0.3 s per launch set.
"""
import functools
import math

import numpy as np
import torch

from oracle import fakequant as fq

FACTOR = 4.0
ABS_FLOOR = 2.0 ** -100
SENS_MIN = 2.0 ** -9             # the one-ulp condition is claimed from here up
MAX_PICKS = {8: 60, 6: 150}      # anchors kept per binade and sign at most
MIN_GAIN = 2                     # ... and none that resolves fewer inputs than this
UNPINNED_CAP = 0.05
SENS_SHARE = 0.95
EPS = np.float32(1.0e-6)

C2 = -2.0 * math.sqrt(2.0 / math.pi) * math.log2(math.e)
C1 = 0.044715 * C2


# ----------------------------------------------------------------------------- tables over the 65536 bit patterns
def _f16(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16)


def _bits(h):
    return np.asarray(h, dtype=np.float16).view(np.uint16)


def gelu64(x, c=0.044715):
    """fp64 GELU(tanh) of an fp64 array, as x / (1 + exp(-2u))."""
    with np.errstate(over="ignore", invalid="ignore"):
        u2 = 2.0 * math.sqrt(2.0 / math.pi) * (x + c * x * x * x)
        return x / (1.0 + np.exp(-u2))


def round16(g):
    """fp64 -> correctly rounded fp16 (numpy converts directly, one rounding)."""
    with np.errstate(over="ignore"):
        return g.astype(np.float16)


class Tables:
    """Everything that depends on the input alone, indexed by the fp16 bit pattern (entries of non-finite patterns unused)."""

    def __init__(self, factor=FACTOR):
        b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        x16 = _f16(b)
        self.finite = np.isfinite(x16)
        x = np.where(self.finite, x16.astype(np.float64), 0.0)
        self.x = x
        self.g64 = gelu64(x)
        self.g_rn = round16(self.g64)
        with np.errstate(over="ignore"):
            self.up = np.nextafter(self.g_rn, np.float16(np.inf))
            self.dn = np.nextafter(self.g_rn, np.float16(-np.inf))
        g = self.g_rn.astype(np.float64)
        up64 = np.where(np.isinf(self.up), 65536.0, self.up.astype(np.float64))      # the boundary to overflow: 65520
        dn64 = np.where(np.isinf(self.dn), -65536.0, self.dn.astype(np.float64))
        self.b_up, self.b_dn = 0.5 * (g + up64), 0.5 * (g + dn64)
        W = x * (C2 + C1 * x * x)
        with np.errstate(over="ignore"):
            sigma = 1.0 / (1.0 + np.exp2(-W))
        self.W = W
        with np.errstate(invalid="ignore", over="ignore"):
            self.E = (4.0 + sigma * (2.0 + 5.0 * math.log(2.0) * np.abs(W))) * 2.0 ** -24
            self.margin = factor * self.E * np.abs(self.g64) + ABS_FLOOR
        self.margin = np.where(np.isfinite(self.margin), self.margin, ABS_FLOOR)     # (W = 3e13 times g64 = 0)
        dist = np.minimum(np.abs(self.g64 - self.b_up), np.abs(self.g64 - self.b_dn))
        self.pinned = (dist > self.margin) | ~self.finite
        lean_up = self.g64 > g
        self.alt = np.where(self.pinned, self.g_rn, np.where(lean_up, self.up, self.dn)).astype(np.float16)
        assert bool(np.isfinite(self.alt[self.finite]).all())
        self.neg = np.signbit(self.g_rn)                                               # the row class of an input
        self.mag = np.abs(self.g_rn)
        self.vmax = np.maximum(self.mag, np.abs(self.alt))                             # no admissible value is larger
        self.g_rn_bits, self.alt_bits = _bits(self.g_rn), _bits(self.alt)
        self.g_rn_f32 = self.g_rn.astype(np.float32)
        self.alt_f32 = self.alt.astype(np.float32)

    def unpinned_share(self):
        return float((~self.pinned[self.finite]).mean())


@functools.lru_cache(maxsize=2)
def tables(factor=FACTOR):
    return Tables(factor)


# ----------------------------------------------------------------------------- the oracle's codes of sizes under an anchor
def _codes(v, M, qmax):
    """Oracle code of the sizes v [nt] (fp32) in a one-sided row whose extreme is M [nc] (fp32): [nc, nt] fp32, zero point
    left out (0 in rows of positive outputs, a constant of the row in the others)."""
    delta = (M / np.float32(qmax)).astype(np.float32)[:, None]
    return np.minimum(np.rint((v[None, :] / delta).astype(np.float32)), np.float32(qmax))


def anchor_ok(M, qmax):
    """The oracle does not eps-fill a row of extreme size M (fp32 array)."""
    return (M / np.float32(qmax)).astype(np.float32) >= EPS


class Plan:
    """placements: [(anchor input bits, input bits [k] uint16, neg)], and per input whether a placement resolves its
    larger / smaller neighbour (res_up, res_dn over the 65536 patterns, in size)."""

    def __init__(self, n_bits):
        t = tables()
        self.n_bits, self.qmax = n_bits, 2 ** n_bits - 1
        self.placements = []
        self.res_up = np.zeros(65536, dtype=bool)
        self.res_dn = np.zeros(65536, dtype=bool)
        self.placed = np.zeros(65536, dtype=bool)
        for neg in (False, True):
            self._sign(t, neg)
        assert bool(self.placed[t.finite].all())

    def _sign(self, t, neg):
        qmax = self.qmax
        ids = np.nonzero(t.finite & (t.neg == neg))[0]
        # distinct (size, largest admissible size): the unit of the cover
        key = (_bits(t.mag[ids]).astype(np.int64) << 16) | _bits(t.vmax[ids]).astype(np.int64)
        ukey, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        uv = _f16((ukey >> 16).astype(np.uint16)).astype(np.float32)
        uvmax = _f16((ukey & 0xFFFF).astype(np.uint16)).astype(np.float32)
        with np.errstate(over="ignore"):
            h = _f16((ukey >> 16).astype(np.uint16))
            uv_hi = np.nextafter(h, np.float16(np.inf)).astype(np.float32)            # (inf above 65504: clamps to qmax)
            uv_lo = np.nextafter(h, np.float16(-np.inf)).astype(np.float32)           # (-2^-24 below 0: never a target here)
        # anchors: sizes with a pinned input, the oracle's step at 1e-6 or more
        pin_ids = ids[t.pinned[ids]]
        cand = np.unique(t.mag[pin_ids]).astype(np.float32)
        cand = cand[anchor_ok(cand, qmax)]
        assert cand.size
        fine_all = cand[(cand / np.float32(qmax)).astype(np.float32) < np.float32(2.0e-6)]
        assert fine_all.size
        fine = fine_all[-1]
        anchor_input = {}
        for i in pin_ids:                                   # the first pinned input of every size (ascending bit pattern)
            anchor_input.setdefault(float(t.mag[i]), int(i))
        need_up = uv >= cand[0]                             # sizes an anchor can sit above with M <= 2v or so
        need_dn = need_up.copy()
        chosen = []                                         # (M, member mask over the distinct units)
        uexp = np.frexp(uv)[1]
        cexp = np.frexp(cand)[1]
        for k in sorted(set(cexp.tolist()), reverse=True):
            ck = cand[cexp == k]                             # every pinned output size of the binade is tried
            w = np.nonzero((uexp >= k - 1) & (uexp <= k) & (uv >= cand[0]))[0]
            if w.size == 0:
                continue
            ok = uvmax[w][None, :] <= ck[:, None]
            c0 = _codes(uv[w], ck, qmax)
            up = ok & (_codes(uv_hi[w], ck, qmax) != c0)
            dn = ok & (_codes(uv_lo[w], ck, qmax) != c0)
            wt = cnt[w].astype(np.float32)                   # (inputs per unit: sums stay exact integers in fp32)
            upf, dnf = up.astype(np.float32), dn.astype(np.float32)
            gain = upf @ (wt * need_up[w]) + dnf @ (wt * need_dn[w])
            for _ in range(MAX_PICKS[self.n_bits]):
                j = int(np.argmax(gain))
                if gain[j] < MIN_GAIN:
                    break
                hit_up, hit_dn = up[j] & need_up[w], dn[j] & need_dn[w]
                member = np.zeros(uv.size, dtype=bool)
                member[w[hit_up | hit_dn]] = True
                need_up[w[hit_up]] = False
                need_dn[w[hit_dn]] = False
                gain -= upf[:, hit_up] @ wt[hit_up] + dnf[:, hit_dn] @ wt[hit_dn]
                chosen.append((float(ck[j]), member))
        # what no anchor resolved (and what lies between the fine anchor and the sizes planned above) goes under the
        # smallest chosen anchor that admits it; everything up to the fine anchor goes under the fine anchor as well
        in_some = np.zeros(uv.size, dtype=bool)
        for _, m in chosen:
            in_some |= m
        chosen.sort(key=lambda c: c[0])
        Ms = np.array([c[0] for c in chosen], dtype=np.float32)
        rest = np.nonzero(~in_some & (uvmax > fine))[0]
        top = None
        for i in rest:
            j = int(np.searchsorted(Ms, uvmax[i], side="left"))
            if j < len(chosen):
                chosen[j][1][i] = True
            else:
                if top is None:
                    assert uvmax[i] <= cand[-1], "an input above every pinned anchor"
                    top = (float(cand[-1]), np.zeros(uv.size, dtype=bool))
                top[1][i] = True
        if top is not None:
            chosen.append(top)
        chosen.append((float(fine), uvmax <= fine))
        # per input: resolved by a placement?  (recomputed from the final membership, the appended inputs included)
        for M, member in chosen:
            u = np.nonzero(member)[0]
            Mf = np.array([M], dtype=np.float32)
            c0 = _codes(uv[u], Mf, qmax)[0]
            r_up = _codes(uv_hi[u], Mf, qmax)[0] != c0
            r_dn = _codes(uv_lo[u], Mf, qmax)[0] != c0
            sel = member[inv]
            members = ids[sel]
            pos = np.searchsorted(u, inv[sel])
            self.res_up[members] |= r_up[pos]
            self.res_dn[members] |= r_dn[pos]
            self.placed[members] = True
            self.placements.append((anchor_input[M], members.astype(np.uint16), neg))

    def sensitivity(self, neg):
        """Share of the inputs of one sign with |g_rn| >= 2^-9 that have a placement resolving the larger neighbour and one
        resolving the smaller."""
        t = tables()
        cls = t.finite & (t.neg == neg) & (t.mag.astype(np.float64) >= SENS_MIN)
        return float((self.res_up & self.res_dn)[cls].mean())


@functools.lru_cache(maxsize=2)
def plan(n_bits):
    return Plan(n_bits)


# ----------------------------------------------------------------------------- rows
def anchor_lanes(C):
    """Lanes of the anchor, by row: first and last chunk, both sides of the middle of the row (the partner waves of the
    split kernel) and of a 512-channel chunk, and the two sides of a lane's 8 channels."""
    out = []
    for p in (0, C - 1, C // 2 - 1, C // 2, 511, 512, 7, 8, C - 8, C // 2 + 255, C // 2 + 256):
        if 0 <= p < C and p not in out:
            out.append(p)
    return out


def tail_columns(C):
    """The columns that reach a call site of their own: at C = 4608 (rowquant_split_kernel) the 4-wide TAIL8 chunk of either
    half row, rq_gelu_tanh<4>; every other column of every kernel goes through rq_gelu_tanh<8>."""
    if C != 4608:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.arange(2048, 2304), np.arange(4352, 4608)])


@functools.lru_cache(maxsize=4)
def rows(n_bits, B, C):
    """x [B, n_tok, C] fp16 of one launch set.  A row takes as many of a placement's inputs as fit BOTH kinds of column
    (tail_columns() and the rest, each filled by repetition), so that every input meets every call site."""
    assert B in (1, 2)
    lanes = anchor_lanes(C)
    tail = tail_columns(C)
    order = np.concatenate([tail, np.setdiff1d(np.arange(C), tail)])       # the tail columns are dealt first
    per = tail.size - 1 if tail.size else C - 1
    out = [[] for _ in range(B)]
    tok = 0
    for anchor, members, _ in plan(n_bits).placements:
        for a in range(0, members.size, per):
            part = members[a:a + per]
            p = lanes[tok % len(lanes)]
            row = np.empty(C, dtype=np.uint16)
            row[order[order != p]] = np.resize(part, C - 1)
            row[p] = anchor
            if B == 1:
                out[0].append(row)
            else:
                other = np.empty(C, dtype=np.uint16)
                other[order] = np.resize(part[::-1], C)
                out[tok % 2].append(row)
                out[1 - tok % 2].append(other)
            tok += 1
    x = np.stack([np.stack(r) for r in out])
    return torch.from_numpy(x.view(np.int16)).view(torch.float16)


def _xbits(x):
    return x.contiguous().view(torch.int16).numpy().view(np.uint16)


# ----------------------------------------------------------------------------- expectation, a stand-in kernel, the checker
def _quantize(g, n_bits, s, C, Kp):
    """The oracle's dynamic quantizer of the fp16 GELU values g [B, n, C] (fp32 tensor) in the kernels' output layout."""
    B, n, _ = g.shape
    v = g if s is None else g / s
    codes, _, delta, zp, eps_fill = fq.dyn_act_quant(v, n_bits)
    cx = 128 if n_bits == 8 else 0
    xq = torch.zeros(B * n, Kp, dtype=torch.int8)
    xq[:, :C] = (codes.int() - cx).reshape(B * n, C).to(torch.int8)
    zx = (zp.reshape(1, n).expand(B, n).reshape(-1).int() - cx).contiguous()
    return {"xq": xq, "sx": delta.reshape(1, n).expand(B, n).reshape(-1).contiguous(), "zx": zx,
            "zpf": zp.reshape(1, n).expand(B, n).reshape(-1).contiguous(), "R": (xq.int().sum(-1) - C * zx).int(),
            "status": int(eps_fill)}, delta, zp


def expected(x, n_bits, s=None):
    """What a correct kernel writes for x [B, n, C] fp16 (s: the value of every entry of the smoothing vector, or None):
    the oracle's outputs for the g_rn rows, plus ``pinned`` [B n, C] and the oracle codes ``alt`` of the other admissible
    value of every element on the row's grid."""
    t = tables()
    B, n, C = x.shape
    Kp = (C + 127) // 128 * 128
    bits = _xbits(x)
    out, delta, zp = _quantize(torch.from_numpy(t.g_rn_f32[bits]), n_bits, s, C, Kp)
    va = torch.from_numpy(t.alt_f32[bits])
    cx = 128 if n_bits == 8 else 0
    alt = fq.quant_codes(va if s is None else va / s, delta, zp, n_bits)
    out["alt"] = (alt.int() - cx).reshape(B * n, C).to(torch.int8)
    out["pinned"] = torch.from_numpy(t.pinned[bits]).reshape(B * n, C)
    out["C"], out["n_bits"] = C, n_bits
    return out


def stand_in(x, n_bits, table_bits, s=None):
    """The outputs of a kernel whose fp16 GELU is ``table_bits`` (uint16 [65536], bit pattern -> bit pattern) and whose
    quantizer is the oracle's."""
    B, n, C = x.shape
    g = _f16(table_bits).astype(np.float32)[_xbits(x)]
    return _quantize(torch.from_numpy(g), n_bits, s, C, (C + 127) // 128 * 128)[0]


def _where(bad):
    return "%d bad, first at %s" % (int(bad.sum()), bad.nonzero()[0].tolist())


def check(exp, got, what=""):
    """``got``: xq [rows, Kp] int8, sx, zx, R [rows], status (int), zpf [rows] or None - CPU tensors."""
    C = exp["C"]
    assert got["status"] == 0, "%s: status %d" % (what, got["status"])
    assert bool(torch.isfinite(got["sx"]).all()), what + ": a step is not finite"
    for f in ("sx", "zx") + (("zpf",) if got.get("zpf") is not None else ()):
        bad = got[f] != exp[f]
        assert not bool(bad.any()), "%s %s: %s: kernel %r, oracle %r" % (what, f, _where(bad), got[f][bad][0].item(),
                                                                          exp[f][bad][0].item())
    xq = got["xq"]
    assert xq.shape == exp["xq"].shape, what
    assert bool((xq[:, C:] == 0).all()), what + ": pad columns are not zero"
    code, pinned = xq[:, :C], exp["pinned"]
    bad = (code != exp["xq"][:, :C]) & (pinned | (code != exp["alt"]))
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s codes: %s: kernel %d, oracle %d%s" % (
            what, _where(bad), int(code[i]), int(exp["xq"][i]),
            " (pinned)" if bool(pinned[i]) else " or %d" % int(exp["alt"][i])))
    R = xq.int().sum(-1) - C * got["zx"].int()
    bad = got["R"].int() != R
    assert not bool(bad.any()), "%s R: %s: kernel %d, sum(xq) - C zx = %d" % (what, _where(bad), int(got["R"][bad][0]), int(R[bad][0]))
    bad = pinned.all(-1) & (got["R"].int() != exp["R"])
    assert not bool(bad.any()), "%s R of a row without unpinned elements: %s" % (what, _where(bad))

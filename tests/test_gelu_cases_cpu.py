"""gelu_cases.py on the CPU: the properties its docstring claims of the reference, the plan and the launch sets; that the
checker fails wrong GELUs pushed through the oracle quantizer in place of the kernel (teeth); and that it admits an fp32
evaluation in the kernel's expression order with exp2 and the reciprocal anywhere within 1 ulp."""
import math

import numpy as np
import pytest
import torch

import gelu_cases as gc
from oracle import fakequant as fq

# (n_bits, B, C) of every launch set test_gelu_rowquant_exact_gpu.py runs
LAUNCH_SETS = [(8, 1, 4608), (8, 1, 4600), (8, 1, 1152), (8, 1, 320), (8, 2, 4608), (8, 2, 1152), (6, 1, 4608), (6, 1, 4600),
               (6, 2, 1152)]
F16 = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def test_reference_and_error_model():
    t = gc.tables()
    assert int(t.finite.sum()) == 63488
    # the stable form equals the textbook tanh form where that one is well conditioned
    x = t.x[t.finite & (t.x > -3.0)]
    tanh_form = 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    assert float(np.max(np.abs(tanh_form - gc.gelu64(x)) / np.maximum(np.abs(tanh_form), 1e-300))) < 1e-12
    # the kernel's two constants against the bounds of the derivation
    u = 2.0 ** -24
    c1 = np.float32(-0.044715) * np.float32(2.302208198)
    c2 = np.float32(-2.302208198)
    assert isinstance(c1, np.float32)
    d1, d2 = abs(float(c1) / gc.C1 - 1.0), abs(float(c2) / gc.C2 - 1.0)
    print("constants: |dc1| = %.2f u, |dc2| = %.2f u" % (d1 / u, d2 / u))
    assert d1 <= 3 * u and d2 <= u
    live = t.finite & (t.g_rn != 0)
    Emax = float(t.E[live].max())
    i = int(np.argmax(np.where(live, t.E, 0.0)))
    print("E: at most %.3g (x = %g, W = %.2f); x > 0: at most %.3g" % (Emax, t.x[i], t.W[i], float(t.E[t.finite & (t.x > 0)].max())))
    assert 4 * u <= float(t.E[live].min()) and Emax <= 6.1e-6
    # g_rn is the nearest fp16 value, the admissible pair brackets g64
    g = t.g_rn.astype(np.float64)
    assert bool(((t.g64 <= t.b_up) & (t.g64 >= t.b_dn))[t.finite].all())
    unp = t.finite & ~t.pinned
    a = t.alt.astype(np.float64)
    assert bool((np.minimum(g, a) <= t.g64)[unp].all()) and bool((t.g64 <= np.maximum(g, a))[unp].all())
    assert bool((np.abs(t.alt_bits.astype(np.int32) - t.g_rn_bits.astype(np.int32))[unp & (t.g_rn != 0)] == 1).all())
    share = t.unpinned_share()
    print("unpinned inputs: %d of 63488 (%.2f %%)" % (int(unp.sum()), 100 * share))
    assert share <= gc.UNPINNED_CAP
    # what a flat relative margin would leave unpinned, for comparison
    for m in (1e-5, 2e-5):
        flat = np.minimum(np.abs(t.g64 - t.b_up), np.abs(t.g64 - t.b_dn)) <= m * np.abs(t.g64)
        print("flat relative margin %g: %.2f %% unpinned" % (m, 100 * float(flat[t.finite].mean())))
    # +-0, +-65504, subnormals, the large negative inputs: finite values, pinned where it matters
    for v in (0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24):
        b = int(np.float16(v).view(np.uint16))
        assert np.isfinite(t.g_rn[b]) and np.isfinite(t.alt[b])
    assert t.g_rn[int(np.float16(65504.0).view(np.uint16))] == np.float16(65504.0)
    assert gc._bits(t.g_rn[int(np.float16(-65504.0).view(np.uint16))]) == 0x8000


@pytest.mark.parametrize("n_bits", [8, 6])
def test_plan_resolves_one_ulp(n_bits):
    t, p = gc.tables(), gc.plan(n_bits)
    assert bool(p.placed[t.finite].all())
    for neg in (False, True):
        share = p.sensitivity(neg)
        print("%d bits, %s outputs: %.2f %% of the inputs with |g_rn| >= 2^-9 have both placements"
              % (n_bits, "negative" if neg else "positive", 100 * share))
        assert share >= gc.SENS_SHARE
    print("%d bits: %d placements" % (n_bits, len(p.placements)))
    # _codes (the planner's restatement) is the oracle's quantizer on a one-sided row
    g = torch.Generator().manual_seed(n_bits)
    for neg in (False, True):
        v = (torch.rand(4, 64, generator=g) * torch.tensor([1e-3, 0.17, 0.1, 0.01]).reshape(4, 1)).half().float()
        M = v.max(-1).values
        want = gc._codes(v.reshape(-1).numpy(), M.numpy(), p.qmax)
        codes, _, _, zp, eps = fq.dyn_act_quant((-v if neg else v)[None], n_bits)
        assert not eps
        got = (codes[0] - zp[0]).abs()
        for r in range(4):
            assert np.array_equal(want[r, 64 * r:64 * r + 64], got[r].numpy())


@pytest.mark.parametrize("n_bits,B,C", LAUNCH_SETS)
def test_launch_sets_cover_every_input_under_pinned_extremes(n_bits, B, C):
    t = gc.tables()
    x = gc.rows(n_bits, B, C)
    assert x.shape[0] == B and x.shape[2] == C and x.dtype == torch.float16
    print("%d bits, B = %d, C = %d: %d tokens" % (n_bits, B, C, x.shape[1]))
    assert x.shape[1] <= 4000
    bits = gc._xbits(x)
    seen = np.zeros(65536, dtype=bool)
    for a in range(0, bits.shape[1], 256):
        seen[np.unique(bits[:, a:a + 256])] = True
    assert bool(seen[t.finite].all()) and not bool(seen[~t.finite].any())
    tail = gc.tail_columns(C)
    if tail.size:                                                 # ... and in the columns of either call site
        for cols in (tail, np.setdiff1d(np.arange(C), tail)):
            seen = np.zeros(65536, dtype=bool)
            for a in range(0, bits.shape[1], 256):
                seen[np.unique(bits[:, a:a + 256][:, :, cols])] = True
            assert bool(seen[t.finite].all())
    # one sign per token; the extreme is reached by pinned elements only and no admissible value exceeds it
    n = x.shape[1]
    tok = bits.transpose(1, 0, 2).reshape(n, B * C)
    neg = t.neg[tok]
    assert bool((neg == neg[:, :1]).all())
    mag = t.mag[tok].astype(np.float32)
    ext = mag.max(-1, keepdims=True)
    assert bool(t.pinned[tok][mag == ext].all())
    assert bool((t.vmax[tok].astype(np.float32) <= ext).all())
    # anchors: sample token % 2 at B = 2; lanes of the first and last chunk and both halves of the row
    lanes = set()
    for i in range(min(n, 64)):
        first = np.nonzero(mag[i] == ext[i])[0]
        lanes.add(int(first[0]) % C)
        if B == 2 and (mag[i] == ext[i]).sum() == 1:
            assert int(first[0]) // C == i % 2
    assert {0, C - 1, C // 2 - 1, C // 2} <= lanes
    for s in (None, 0.5):
        if s is not None and (B, C) not in ((1, 4608), (1, 1152), (1, 320), (2, 4608), (2, 1152)):
            continue
        e = gc.expected(x, n_bits, s)
        assert e["status"] == 0                                   # no row the oracle would eps-fill
        assert float(e["sx"].min()) >= 1e-6
        if s is not None:                                         # the plan carries over behind s = 0.5: values doubled
            e1 = gc.expected(x, n_bits, None)
            assert torch.equal(e["xq"], e1["xq"]) and torch.equal(e["sx"], 2 * e1["sx"]) and torch.equal(e["alt"], e1["alt"])


# ----------------------------------------------------------------------------- teeth
def _fails(x, n_bits, table, s=None):
    try:
        gc.check(gc.expected(x, n_bits, s), gc.stand_in(x, n_bits, gc._bits(table), s), "stand-in")
    except AssertionError:
        return True
    return False


def _trunc16(g64):
    h = gc.round16(g64)
    over = np.abs(h.astype(np.float64)) > np.abs(g64)
    return np.where(over, np.nextafter(h, np.float16(0.0)), h).astype(np.float16)


def _move(t, sel, up):
    with np.errstate(over="ignore"):
        return np.where(sel, t.up if up else t.dn, t.g_rn).astype(np.float16)


TEETH_SETS = [(8, 1, 320, None), (8, 2, 1152, 0.5), (6, 1, 1152, None)]


@pytest.mark.parametrize("n_bits,B,C,s", TEETH_SETS)
def test_wrong_gelus_fail(n_bits, B, C, s):
    t = gc.tables()
    x = gc.rows(n_bits, B, C)
    assert not _fails(x, n_bits, t.g_rn, s)                      # the checker passes g_rn itself, and any admissible mix
    assert not _fails(x, n_bits, t.alt, s)
    assert not _fails(x, n_bits, np.where(np.arange(65536) % 2 == 0, t.g_rn, t.alt), s)
    erf = 0.5 * t.x * (1.0 + torch.special.erf(torch.from_numpy(t.x) / math.sqrt(2.0)).numpy())
    wrong = {"0.0447 for 0.044715": gc.round16(gc.gelu64(t.x, 0.0447)), "erf GELU": gc.round16(erf),
             "truncation to fp16": _trunc16(t.g64)}
    for name, table in wrong.items():
        assert int((gc._bits(table) != t.g_rn_bits)[t.finite].sum()) > 0
        assert _fails(x, n_bits, table, s), name
    # one ulp on a single binade of the output, every binade from 2^-9 up, both signs, both directions
    ex = np.frexp(t.mag.astype(np.float64))[1]
    for neg in (False, True):
        cls = t.finite & (t.neg == neg) & (t.mag.astype(np.float64) >= gc.SENS_MIN)
        for k in sorted(set(ex[cls].tolist())):
            for up in (True, False) if n_bits == 8 and B == 1 else (bool(k % 2),):
                assert _fails(x, n_bits, _move(t, cls & (ex == k), up), s), (neg, k, up)


def test_one_ulp_on_one_input_is_caught():
    """g_rn moved by one ulp at ONE input (a seeded sample of 400 inputs with |g_rn| >= 2^-9, either direction in turn):
    the rows that hold the input, through the oracle quantizer and check()."""
    t = gc.tables()
    for n_bits, B, C, floor in ((8, 1, 320, 0.95), (6, 2, 1152, 0.95)):
        x = gc.rows(n_bits, B, C)
        bits = gc._xbits(x)
        pool = np.nonzero(t.finite & (t.mag.astype(np.float64) >= gc.SENS_MIN))[0]
        sample = pool[np.random.RandomState(5).permutation(pool.size)[:400]]
        caught = 0
        for j, b in enumerate(sample):
            rows_ = np.nonzero((bits == b).any(axis=(0, 2)))[0]
            assert rows_.size
            sel = np.zeros(65536, dtype=bool)
            sel[b] = True
            caught += _fails(x[:, torch.from_numpy(rows_)], n_bits, _move(t, sel, j % 2 == 0))
        print("%d bits, B = %d, C = %d: %d of %d single-input one-ulp errors caught" % (n_bits, B, C, caught, sample.size))
        assert caught >= floor * sample.size


# ----------------------------------------------------------------------------- a correct kernel passes
def emulate(de, dr):
    """rq_gelu_tanh in numpy fp32, expression by expression (the fma rounded once), exp2 and the reciprocal correctly
    rounded and then moved by ``de`` / ``dr`` ulp (2^-23 relative): fp16 [65536]."""
    f32, f64 = np.float32, np.float64
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        x = np.where(np.isfinite(F16), F16, np.float16(0)).astype(f32)
        c1, c2 = f32(-0.044715) * f32(2.302208198), f32(-2.302208198)
        xx = x * x
        p = (xx.astype(f64) * f64(c1) + f64(c2)).astype(f32)
        w = x * p
        e = (np.exp2(w.astype(f64)) * (1.0 + de * 2.0 ** -23)).astype(f32)
        d = e + f32(1.0)
        r = ((1.0 / d.astype(f64)) * (1.0 + dr * 2.0 ** -23)).astype(f32)
        return (x * r).astype(np.float16)


def test_a_correct_kernel_passes():
    t = gc.tables()
    for de in (-1, 0, 1):                                        # per input: g_rn where pinned, else one of the two
        for dr in (-1, 0, 1):
            h = emulate(de, dr)
            ok = (h == t.g_rn) | (~t.pinned & (h == t.alt))
            assert bool(ok[t.finite].all()), (de, dr, int((~ok[t.finite]).sum()))
    for n_bits, B, C, s in TEETH_SETS:                           # and through the rows and check()
        x = gc.rows(n_bits, B, C)
        for de, dr in ((-1, -1), (1, 1), (-1, 1), (0, 0)):
            assert not _fails(x, n_bits, emulate(de, dr), s), (n_bits, B, C, de, dr)


def test_fp32_error_stays_inside_the_model():
    """The emulation's fp32 value before the fp16 conversion against g64, exp2 and the reciprocal within 1 ulp of the true
    value (2^-24 relative, then rounded: 2u in all, the model's figure): inside E(x) at every input, and so FACTOR times
    inside the margin.  (test_a_correct_kernel_passes moves the ROUNDED values by a whole ulp, 3u in all: the factor's job.)"""
    f32, f64 = np.float32, np.float64
    t = gc.tables()
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        x = t.x.astype(f32)
        c1, c2 = f32(-0.044715) * f32(2.302208198), f32(-2.302208198)
        p = ((x * x).astype(f64) * f64(c1) + f64(c2)).astype(f32)
        w = x * p
        worst = 0.0
        for de in (-1, 1):
            for dr in (-1, 1):
                e = (np.exp2(w.astype(f64)) * (1.0 + de * 2.0 ** -24)).astype(f32)
                r = ((1.0 / (e + f32(1.0)).astype(f64)) * (1.0 + dr * 2.0 ** -24)).astype(f32)
                g = (x * r).astype(f64)
                live = t.finite & (np.abs(t.g64) > 2.0 ** -90)
                ratio = np.abs(g - t.g64)[live] / (t.E[live] * np.abs(t.g64[live]))
                worst = max(worst, float(ratio.max()))
    print("fp32 emulation: error at most %.2f E" % worst)
    assert worst <= 1.0

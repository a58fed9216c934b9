"""Every LayerNorm + modulate + quantizer kernel under the margin-exact rule of ln_cases.py: one launch, then
ln_cases.check_launch / check_static - codes, zero point and the fp16 activation exact wherever the fp64 reference is not
within a proven margin of a rounding boundary (there: one of the two neighbours), the step within its bound on every row of
every sample, R from the kernel's own codes, zero pads, status 0.  test_ln_cases_cpu.py proves on the CPU that no correct
fp32 evaluation can fail these checks and that the listed wrong ones do.

Rows are ln_cases.mixed(): every family (L1 - L4, Q3 / Q5 / Q6) dealt into one launch.  Row counts: 1 (the half-wave's
partner row is dead; at B = 1 the block widths fall back to one row per wave), 2 (one wave), 9 (a partial last workgroup of
the four- and eight-wave kernels), 37 (odd: at B = 2 row 37 starts sample 1, so a wave's two rows straddle the samples in
the generic layouts).  eps is 1e-6 at 37 and 2 rows and 1e-5 at 9 and 1 (row 0 is an L3 row: its variance is about eps).

No route query exists for vq_ln_modulate_rowquant; the kernel named beside each case is derived from the dispatch code
(rowquant.hip: vq_ln_modulate_rowquant; rowquant_fast.hip: vq_lnq_fast, vq_lnq_pair_fast; rowquant_static.hip:
rqs_dispatch).  ops.rowquant_multi_shared_ok / rowquant_static_ok mirror their entry points' refusals and are asserted."""
import functools

import pytest

import ln_cases as lc

pytestmark = pytest.mark.gpu

ROWS_EPS = ((37, 1e-6), (9, 1e-5), (2, 1e-6), (1, 1e-5))


@functools.lru_cache(maxsize=3)
def _base(B, n, C, eps):
    """The launch's inputs and its reference (the modulated part: shared by every case of the shape, left unchanged)."""
    x, shift, scale, names = lc.mixed(B, n, C)
    return x, shift, scale, lc.Reference(x, shift, scale, eps, 8, [None], names=names)


def _smooth(C, n_vec, plain_first=False):
    vec = lc.smooth_vectors(C, 3)
    return ([None] + vec[1:n_vec]) if plain_first else vec[:n_vec]


def _cpu(qa, st, xm):
    return {"xq": qa.xq.cpu(), "sx": qa.sx.cpu(), "zx": qa.zx.cpu(), "R": qa.R.cpu(),
            "status": 0 if st is None else int(st.item()), "xm": None if xm is None else xm.cpu()}


def _sorted(cases):
    """x ROWS_EPS, launches of one shape next to each other (they share a reference)."""
    out = [pytest.param(*c, n, eps, id="-".join(str(v) for v in c) + "-n%d" % n) for c in cases for n, eps in ROWS_EPS]
    return sorted(out, key=lambda p: (p.values[1], p.values[2], p.values[-2]))


# ----------------------------------------------------------------------------- ops.ln_modulate_rowquant
# kernel (derived from the dispatch; "fast<M, N>" = ln_modulate_rowquant_fast_kernel<MAXCH = M, NOUT = N>, which every B = 1
# launch of one row takes as well), B, C, smoothing vectors, want_xm, fast_div, n_bits
LNQ = [
    ("fast<1,1>", 1, 64, 0, True, True, 8), ("fast<1,2>", 1, 64, 2, True, True, 8),
    ("fast<3,1>", 1, 1408, 0, True, True, 8), ("fast<3,3>", 1, 1408, 3, True, True, 8),
    ("half<6>", 1, 768, 0, False, True, 8), ("half<8>", 1, 1024, 0, False, True, 8),
    ("half<9>", 1, 1152, 0, False, True, 8), ("half<10>", 1, 1280, 0, False, True, 8),
    ("fast<3,1>", 1, 1152, 0, True, True, 8),                       # the fp16 output at B = 1: one row per wave
    ("half<9,PAIR>", 2, 1152, 0, False, True, 8), ("half<9,PAIR,XM>", 2, 1152, 0, True, True, 8),
    ("half<6,PAIR>", 2, 768, 0, False, True, 8), ("half<6,PAIR,XM>", 2, 768, 0, True, True, 8),
    ("smooth_multi<LN,1>", 1, 1152, 1, True, True, 8), ("smooth_multi<LN,3>", 1, 1152, 3, True, True, 8),
    ("smooth_multi<LN,2>", 1, 768, 2, True, True, 8),
    ("smooth_half<LN,PAIR>", 2, 1152, 1, False, True, 8),           # vq_lnq_pair_fast with a vector and its reciprocal
    ("fast<3,3> IEEE division", 1, 1152, 3, True, False, 8),
    ("generic<1> IEEE division", 2, 1152, 1, True, False, 8), ("generic<3>", 2, 1152, 3, True, True, 8),
    ("generic<1>", 1, 4608, 0, True, True, 8), ("generic<2>", 2, 4608, 2, False, True, 8),
    ("generic<1>", 3, 96, 0, True, True, 8),
    # sub-8-bit codes (the clamp of RQ_BY_WIDTH's other arm) through every form
    ("fast<1,2>", 1, 64, 2, True, True, 6), ("fast<3,3>", 1, 1408, 3, True, True, 4),
    ("half<9>", 1, 1152, 0, False, True, 6), ("half<9>", 1, 1152, 0, False, True, 4),
    ("half<9,PAIR,XM>", 2, 1152, 0, True, True, 6), ("half<6,PAIR>", 2, 768, 0, False, True, 4),
    ("smooth_multi<LN,1>", 1, 1152, 1, True, True, 4), ("smooth_multi<LN,3>", 1, 1152, 3, True, True, 6),
    ("smooth_half<LN,PAIR>", 2, 1152, 1, False, True, 6), ("smooth_half<LN,PAIR>", 2, 1152, 1, False, True, 4),
    ("generic<3>", 2, 1152, 3, True, True, 6), ("generic<1>", 1, 4608, 0, True, True, 4),
]


@pytest.mark.parametrize("kernel,B,C,n_vec,want_xm,fast_div,n_bits,n_tok,eps", _sorted(LNQ))
def test_ln_modulate_rowquant_margin_exact(ops, dev, kernel, B, C, n_vec, want_xm, fast_div, n_bits, n_tok, eps):
    x, shift, scale, base = _base(B, n_tok, C, eps)
    # (the kernels without reciprocals take any mix of plain and smoothed outputs: output 0 plain where there are several)
    smooth = _smooth(C, n_vec, plain_first=kernel.startswith(("fast", "generic")) and n_vec > 1) if n_vec else [None]
    ref = base.rebits(n_bits, smooth)
    sd = [None if s is None else s.to(dev) for s in smooth]
    if fast_div:
        assert all(ops.smooth_rcp(s) is not None for s in sd if s is not None)
    st = ops.new_status(dev)
    outs = ops.ln_modulate_rowquant(x.to(dev), shift.to(dev), scale.to(dev), eps, smooth=sd, n_bits=n_bits, status=st,
                                    want_xm=want_xm, fast_div=fast_div)
    outs, xm = outs if want_xm else (outs, None)
    assert len(outs) == len(smooth)
    for j, qa in enumerate(outs):
        assert qa.xq.shape == (B * n_tok, ops.pad128(C))
        shares = lc.check_launch(ref, j, _cpu(qa, st, xm), "%s B%d C%d n%d b%d out%d" % (kernel, B, C, n_tok, n_bits, j))
        print("%s B%d C%d n%d b%d out%d: shares inside a margin %s" % (kernel, B, C, n_tok, n_bits, j, shares))


# ----------------------------------------------------------------------------- ops.rowquant_multi_shared (joint B = 2)
# smooth_rowquant_multi_kernel<NIT, LN, NOUT, .., PAIR>
SHARED = [("smooth_multi<LN,%d,PAIR>" % g, 2, C, g, 8) for C in (768, 1152) for g in (1, 2, 3)] + \
         [("smooth_multi<LN,3,PAIR>", 2, 1152, 3, 6), ("smooth_multi<LN,2,PAIR>", 2, 768, 2, 4)]


@pytest.mark.parametrize("kernel,B,C,n_vec,n_bits,n_tok,eps", _sorted(SHARED))
def test_rowquant_multi_shared_margin_exact(ops, dev, kernel, B, C, n_vec, n_bits, n_tok, eps):
    x, shift, scale, base = _base(B, n_tok, C, eps)
    smooth = _smooth(C, n_vec)
    ref = base.rebits(n_bits, smooth)
    sd = [s.to(dev) for s in smooth]
    assert all(ops.smooth_rcp(s) is not None for s in sd)
    assert ops.rowquant_multi_shared_ok(B, n_tok, C, ops.pad128(C), n_bits, n_vec)
    st = ops.new_status(dev)
    outs = ops.rowquant_multi_shared(x.to(dev), sd, n_bits=n_bits, status=st, shift=shift.to(dev), scale=scale.to(dev), eps=eps)
    assert outs is not None and len(outs) == n_vec
    for j, qa in enumerate(outs):
        lc.check_launch(ref, j, _cpu(qa, st, None), "%s C%d n%d b%d out%d" % (kernel, C, n_tok, n_bits, j))


# ----------------------------------------------------------------------------- ops.rowquant_static behind LayerNorm + modulate
# rowquant_static_kernel<L, RQS_LN, NOUT>: L = RqHalf<NIT> at B = 2 and a block width (two rows or more), else RqWave<MAXCH>
# lane map, B, C, per_token, outputs, want_xm, n_bits
STATIC = [
    ("RqWave<1>", 1, 96, True, 1, True, 8), ("RqWave<1>", 2, 96, False, 2, False, 8),
    ("RqWave<3>", 1, 768, False, 3, True, 8), ("RqHalf<6>", 2, 768, True, 1, True, 8),
    ("RqWave<3>", 1, 1152, True, 2, True, 8), ("RqHalf<9>", 2, 1152, False, 3, True, 8), ("RqHalf<9>", 2, 1152, True, 1, False, 8),
    ("RqWave<9>", 1, 4608, True, 1, True, 8), ("RqWave<9>", 2, 4608, False, 3, False, 8),
    ("RqHalf<9>", 2, 1152, True, 2, True, 6), ("RqHalf<9>", 2, 1152, False, 3, True, 4),
    ("RqWave<3>", 1, 1152, False, 2, True, 4), ("RqWave<9>", 1, 4608, True, 2, True, 6),
]


@pytest.mark.parametrize("lane_map,B,C,per_token,n_out,want_xm,n_bits,n_tok,eps", _sorted(STATIC))
def test_rowquant_static_layernorm_arm_margin_exact(ops, dev, lane_map, B, C, per_token, n_out, want_xm, n_bits, n_tok, eps):
    x, shift, scale, base = _base(B, n_tok, C, eps)
    smooth = _smooth(C, n_out, plain_first=True)
    ref = base.rebits(n_bits, smooth)
    ds, zs = lc.static_grids(ref, per_token, n_out)
    sd = [None if s is None else s.to(dev) for s in smooth]
    assert all(ops.smooth_rcp(s) is not None for s in sd if s is not None)
    assert ops.rowquant_static_ok(C, ops.pad128(C), n_bits, n_out, ln=True)
    outs = ops.rowquant_static(x.to(dev), [d.to(dev) for d in ds], [z.to(dev) for z in zs], n_bits=n_bits, smooth=sd,
                               shift=shift.to(dev), scale=scale.to(dev), eps=eps, want_xm=want_xm)
    outs, xm = outs if want_xm else (outs, None)
    qmax = 2 ** n_bits - 1
    for j, qa in enumerate(outs):
        lc.check_static(ref, j, _cpu(qa, None, xm), ds[j], zs[j], "%s B%d C%d n%d b%d out%d" % (lane_map, B, C, n_tok, n_bits, j))
    codes = outs[0].xq[:, :C].int() + (128 if n_bits == 8 else 0)      # the narrow grid (0.8 of the range, centred) clamps at both ends
    assert bool((codes == 0).any()) and bool((codes == qmax).any())

"""The int8 GEMM per output element, on operands whose result is known without a GPU library (gemm_cases.py; the
builders are proven by test_gemm_cases_cpu.py).

G1 (address), G2 (exact dequantisation), G4 (fp16 store, residual and gate epilogues) are compared BITWISE with the CPU
expectation; G3 (saturation) and G5 (GELU) per element against the bounds derived in gemm_cases.py - never a norm.
Every case runs through ops.gemm_i8 for the library's own choice and for the pinned kernels 11 (256 x 288 tile), 16
(128 x 288 tile) and 19 (interior form; refused, as it must be, on anything but interior shapes).  Ragged cases launch
into a view of a larger, sentinel-filled buffer, from operand views whose rows beyond M / N hold poison: nothing outside
[0, M) x [0, N) may change and nothing outside the operands may be read into a result.  All memory touched is allocated.
"""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

VARIANTS = [-1, 11, 16, 19]
SENTINEL = 0x5AA5       # fp16 bit pattern of a finite value (212.6) no case produces by the row
INT_MAX = 2 ** 31 - 1
BITS = [(8, 8), (8, 6), (8, 4), (6, 8), (6, 6), (6, 4)]


def _is_interior(M, N, K, ldo, gate_rows=0):
    return M % 256 == 0 and N % 288 == 0 and ldo % 8 == 0 and (gate_rows == 0 or gate_rows % 256 == 0)


def _poisoned(t, extra, fill, dev):
    """``t`` as the leading slice of a buffer ``extra`` rows longer whose tail holds ``fill``."""
    big = torch.empty((t.shape[0] + extra,) + tuple(t.shape[1:]), dtype=t.dtype)
    big[:t.shape[0]] = t
    big[t.shape[0]:] = fill
    return big.to(dev)[:t.shape[0]]


def _upload(ops, dev, c, poison):
    """(QAct, PackedWeight, bias) of a case on the GPU; poison: every array is a view of a longer one whose rows at and
    beyond M / N hold code 127, NaN and INT_MAX."""
    if poison:
        a = ops.QAct(_poisoned(c.xq, 5, 127, dev), _poisoned(c.sx, 5, float("nan"), dev), _poisoned(c.zx, 5, INT_MAX, dev),
                     _poisoned(c.R, 5, INT_MAX, dev), c.K, c.a_bits)
        w = ops.PackedWeight(_poisoned(c.wq, 5, 127, dev), _poisoned(c.sw, 5, float("nan"), dev),
                             _poisoned(c.zw, 5, INT_MAX, dev), _poisoned(c.cs, 5, INT_MAX, dev), c.N, c.K, c.Kp, c.w_bits)
        b = None if c.bias is None else _poisoned(c.bias, 5, float("nan"), dev)
    else:
        a = ops.QAct(c.xq.to(dev), c.sx.to(dev), c.zx.to(dev), c.R.to(dev), c.K, c.a_bits)
        w = ops.PackedWeight(c.wq.to(dev), c.sw.to(dev), c.zw.to(dev), c.cs.to(dev), c.N, c.K, c.Kp, c.w_bits)
        b = None if c.bias is None else c.bias.to(dev)
    return a, w, b


def _framed(M, N, pad, dev, inner=None):
    """(buffer [M + 3, N + pad] of sentinels - or holding ``inner`` in its [0, M) x [0, N) corner -, its [M, N] view)."""
    buf = torch.full((M + 3, N + pad), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)
    if inner is not None:
        buf[:M, :N] = inner.to(dev)
    return buf, buf[:M, :N]


def _frame_untouched(buf, M, N):
    b = buf.view(torch.int16)
    return bool((b[M:] == SENTINEL).all()) and bool((b[:M, N:] == SENTINEL).all())


def _launches(ops, dev, c, gate_rows=0, epilogue=None, resid=None, gate=None):
    """Yield (variant, out [M, N] on the GPU, BM) for every kernel that accepts the case; ragged cases are poisoned,
    framed (row pitch N + 8 = 4 mod 8 and N + 4 = 0 mod 8 for the ragged N used here) and checked for ownership."""
    M, N = c.M, c.N
    ragged = not _is_interior(M, N, c.K, N)
    a, w, b = _upload(ops, dev, c, poison=ragged)
    kw = {}
    if epilogue is not None:
        kw["epilogue"] = epilogue
    if gate is not None:
        kw.update(gate=gate.to(dev), rows_per_gate=gate_rows)
    for vi, variant in enumerate(VARIANTS):
        pad = (8, 4)[vi % 2] if ragged else 0
        buf = rbuf = None
        if ragged:
            buf, out = _framed(M, N, pad, dev)
            if resid is not None:
                rbuf, kw["resid"] = _framed(M, N, pad, dev, resid)
        else:
            out = torch.full((M, N), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)
            if resid is not None:
                kw["resid"] = resid.to(dev)
        if variant == 19 and not _is_interior(M, N, c.K, N + pad, gate_rows):
            with pytest.raises(Exception):
                ops.gemm_i8(a, w, bias=b, out=out, variant=19, **kw)
            continue
        ops.gemm_i8(a, w, bias=b, out=out, variant=variant, **kw)
        torch.cuda.synchronize()
        if ragged:
            assert _frame_untouched(buf, M, N), "%s variant %d: wrote outside [0, M) x [0, N) (pitch N + %d)" % (c.name, variant, pad)
            if rbuf is not None:
                assert _frame_untouched(rbuf, M, N)
        yield variant, out, 128 if variant == 16 else 256


def _assert_bits(out, expect, what, BM):
    e = expect.to(out.device)
    if torch.equal(out.view(torch.int16), e.view(torch.int16)):
        return
    bad = (out.view(torch.int16) != e.view(torch.int16)).cpu()
    idx = torch.nonzero(bad)[0]
    m, n = int(idx[0]), int(idx[1])
    raise AssertionError("%s: %s; got %r (0x%04x), expected %r (0x%04x)" % (
        what, gc.first_mismatch(bad, BM), float(out[m, n]), int(out.view(torch.int16)[m, n]) & 0xFFFF,
        float(expect[m, n]), int(expect.view(torch.int16)[m, n]) & 0xFFFF))


def _assert_bound(out, ref, bound, what, BM):
    o = out.cpu().double()
    assert not bool(torch.isnan(o).any()), what + ": NaN"
    diff = (o - ref.double()).abs()
    bad = ~(diff <= bound)
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0]
        m, n = int(idx[0]), int(idx[1])
        raise AssertionError("%s: %s; got %r, reference %r, bound %.3e, worst excess %.3e" % (
            what, gc.first_mismatch(bad, BM), float(o[m, n]), float(ref[m, n]), float(bound[m, n]),
            float((diff - bound).max())))


# ------------------------------------------------------------------------------------------------------------ G1
# (6-bit weights travel as int8 like 8-bit ones: the benchmark sizes run at 8 and 4 bits)
@pytest.mark.parametrize("M,N,K,w_bits", [s + (b,) for s in gc.BENCH_SHAPES for b in (8, 4)] +
                         [s + (b,) for s in gc.RAGGED_SHAPES + gc.INTERIOR_SHAPES for b in (8, 6, 4)])
def test_g1_every_output_names_its_row_channel_and_k(ops, dev, M, N, K, w_bits):
    c = gc.g1(M, N, K, w_bits)
    expect = c.exact.to(dev).half()               # integers up to 7 * 128
    for variant, out, BM in _launches(ops, dev, c):
        _assert_bits(out, expect, "%s variant %d" % (c.name, variant), BM)


# ------------------------------------------------------------------------------------------------------------ G2
@pytest.mark.parametrize("ab,wb", BITS)
@pytest.mark.parametrize("M,N,K", gc.RAGGED_SHAPES + gc.INTERIOR_SHAPES)
def test_g2_dequantisation_is_exact(ops, dev, M, N, K, ab, wb):
    c = gc.g2(M, N, K, ab, wb, zw_span=gc.g2_zw_span(K, ab, wb), bias=(M + wb) % 3 != 0)
    expect = c.expect_half()
    for variant, out, BM in _launches(ops, dev, c):
        _assert_bits(out, expect, "%s variant %d" % (c.name, variant), BM)


def _g2_sets(M, N, K, wb, n):
    """n G2 weight sets (different codes, zero points, scales, biases) for the activation of set 0."""
    c0 = gc.g2(M, N, K, 8, wb, seed=0)
    out = [c0]
    for s in range(1, n):
        cs = gc.g2(M, N, K, 8, wb, seed=s)
        sw = cs.sw.double() * 2.0 ** s
        c = gc.assemble("%s_set%d" % (c0.name, s), c0.x_raw, c0.zx_raw, 8, cs.w_raw, cs.zw_raw, wb, c0.sx.double(), sw,
                        cs.bias.double() * 2.0 ** s)
        gc.prove_exact(c)
        out.append(c)
    return out


@pytest.mark.parametrize("M,N,K", [(130, 580, 200), (256, 288, 128), (1024, 1152, 256)])
def test_g2_batched_launch_against_the_cpu_expectation(ops, dev, M, N, K):
    sets = _g2_sets(M, N, K, 8, 3)
    assert not torch.equal(sets[0].sw, sets[1].sw) and not torch.equal(sets[1].zw, sets[2].zw)
    a, _, _ = _upload(ops, dev, sets[0], poison=False)
    pws = [_upload(ops, dev, c, poison=False)[1] for c in sets]
    st = ops.stack_packed(pws, [c.bias.to(dev) for c in sets])
    got = ops.gemm_i8_batched(a, st)
    for b, c in enumerate(sets):
        _assert_bits(got[b], c.expect_half(), "%s batched set %d" % (c.name, b), 256)


@pytest.mark.parametrize("M,N,K,wb", [(300, 292, 200, 8), (130, 580, 200, 4), (512, 576, 256, 8)])
def test_g2_grouped_launch_against_the_cpu_expectation(ops, dev, M, N, K, wb):
    cases = [gc.g2(M, N, K, 8, wb, seed=s, bias=s != 1) for s in range(3)]          # middle bias None
    ups = [_upload(ops, dev, c, poison=False) for c in cases]
    buf, out = _framed(M, 3 * N, 8, dev)
    ops.gemm_i8_grouped([u[0] for u in ups], [u[1] for u in ups], [u[2] for u in ups], out=out)
    torch.cuda.synchronize()
    assert _frame_untouched(buf, M, 3 * N)
    for g, c in enumerate(cases):
        _assert_bits(out[:, g * N:(g + 1) * N], c.expect_half(), "%s group %d" % (c.name, g), 256)


@pytest.mark.parametrize("M,N,K", [(300, 580, 200), (512, 576, 256)])
def test_g2_stamped_launch_against_the_cpu_expectation(ops, dev, M, N, K):
    c = gc.g2(M, N, K, 8, 8)
    a, w, b = _upload(ops, dev, c, poison=False)
    out, stamps = ops.gemm_i8_stamped(a, w, bias=b)
    _assert_bits(out, c.expect_half(), c.name + " stamped", 256)


@pytest.mark.parametrize("ab,wb", BITS)
def test_g2_operands_are_what_the_product_quantizers_make(ops, dev, ab, wb):
    """Builder vs product packer: the dequantised G2 operands (code - zp) delta are fp16 numbers on a power-of-two grid
    that holds both range ends in every row, so weight_minmax + pack_weight and rowquant must give the builder's fields
    back bit for bit - the hand-made operands are what the model path produces."""
    M, N, K = 130, 580, 200
    c = gc.g2(M, N, K, ab, wb)
    W = gc.dequantised(c.w_raw, c.zw_raw, c.sw).to(dev)
    d, z = ops.weight_minmax(W, wb)
    assert torch.equal(d.cpu(), c.sw) and torch.equal(z.cpu(), c.zw_raw.float())
    pw = ops.pack_weight(W, d, z, wb)
    assert pw.wq.dtype == c.wq.dtype and torch.equal(pw.wq.cpu(), c.wq)
    assert torch.equal(pw.sw.cpu(), c.sw) and torch.equal(pw.zw.cpu(), c.zw) and torch.equal(pw.cs.cpu(), c.cs)
    x = gc.dequantised(c.x_raw, c.zx_raw, c.sx).to(dev)
    st = ops.new_status(dev)
    qa = ops.rowquant(x[None], n_bits=ab, status=st)
    assert int(st.item()) == 0
    assert torch.equal(qa.xq.cpu(), c.xq) and torch.equal(qa.sx.cpu(), c.sx)
    assert torch.equal(qa.zx.cpu(), c.zx) and torch.equal(qa.R.cpu(), c.R)
    # and the product's operands through the GEMM land on the builder's expectation
    _assert_bits(ops.gemm_i8(qa, pw, bias=c.bias.to(dev)), c.expect_half(), c.name + " product operands", 256)


# ------------------------------------------------------------------------------------------------------------ G3
@pytest.mark.parametrize("w_bits", [8, 4])
@pytest.mark.parametrize("K", [4608, 16380])
@pytest.mark.parametrize("M,N", [(130, 292), (256, 288)])
def test_g3_saturated_codes_stay_inside_the_stated_bound(ops, dev, M, N, K, w_bits):
    c = gc.g3(M, N, K, w_bits)
    ref, bound = gc.g3_bound(c)
    for variant, out, BM in _launches(ops, dev, c):
        _assert_bound(out, ref, bound, "%s variant %d" % (c.name, variant), BM)


# ------------------------------------------------------------------------------------------------------------ G4
G4_SHAPES = [(1, 4, 1, 8), (5, 292, 72, 8), (300, 292, 200, 8), (513, 580, 72, 8), (130, 580, 200, 8), (256, 288, 128, 8),
             (512, 576, 256, 8), (300, 292, 200, 4), (257, 1156, 1100, 4), (300, 292, 1100, 4), (512, 576, 256, 4),
             (1024, 1152, 1152, 4), (130, 580, 200, 6)]


@pytest.mark.parametrize("M,N,K,w_bits", G4_SHAPES)
def test_g4_store_rounds_to_nearest_even_at_ties_edges_and_subnormals(ops, dev, M, N, K, w_bits):
    c = gc.g4(M, N, K, w_bits)
    expect = c.expect_half()
    for variant, out, BM in _launches(ops, dev, c):
        _assert_bits(out, expect, "%s variant %d" % (c.name, variant), BM)


@pytest.mark.parametrize("M,N,K,w_bits", [(130, 580, 72, 8), (130, 580, 72, 4), (256, 288, 128, 8), (300, 292, 100, 8)])
def test_g4_store_at_the_fp32_neighbours_of_65520(ops, dev, M, N, K, w_bits):
    c = gc.g4(M, N, K, w_bits, edges=True)
    expect = c.expect_half()
    for variant, out, BM in _launches(ops, dev, c):
        _assert_bits(out, expect, "%s variant %d" % (c.name, variant), BM)


# rows_per_gate: 0 = VQ_EPI_RESID; aligned with a 256-row tile; straddling tiles (the un-folded gate path)
@pytest.mark.parametrize("M,N,K,w_bits,rpg", [(300, 292, 200, 8, 0), (300, 292, 200, 8, 100), (513, 580, 72, 8, 171),
                                              (513, 580, 72, 4, 256), (512, 576, 256, 8, 0), (512, 576, 256, 8, 256),
                                              (512, 576, 256, 4, 256), (512, 576, 256, 8, 100), (1024, 1152, 1152, 4, 512),
                                              (1024, 1152, 1152, 4, 0), (257, 1156, 1100, 4, 129)])
def test_g4_residual_and_gate_epilogues(ops, dev, M, N, K, w_bits, rpg):
    """half(float(resid) + g float(half(y))) (gemm_common.h), bitwise: zero sums, sums that tie, sums across 65520;
    power-of-two gates, so the folded (gate inside the staged scales) and un-folded forms must agree."""
    c, resid, gate, expected = gc.g4_resid(M, N, K, w_bits, rpg)
    epi = ops.EPI_GATE_RESID if rpg else ops.EPI_RESID
    for variant, out, BM in _launches(ops, dev, c, gate_rows=rpg, epilogue=epi, resid=resid, gate=gate):
        _assert_bits(out, expected, "%s variant %d" % (c.name, variant), BM)


# ------------------------------------------------------------------------------------------------------------ G5
@pytest.mark.parametrize("M,N,K,w_bits", [(300, 292, 200, 8), (257, 1156, 72, 4), (513, 580, 72, 8), (256, 288, 128, 8),
                                          (512, 576, 256, 4), (1024, 1152, 256, 8)])
def test_g5_gelu_epilogue_per_element_and_in_its_tails(ops, dev, M, N, K, w_bits):
    """tanh-GELU in fp64 of the exact y; per element one fp16 ulp of the reference (floor 2^-24) + the relative error of
    the v_exp_f32 / v_rcp_f32 formula (gemm_cases.G5_REL, derived there and checked on the CPU); very negative y gives
    +-0, never NaN."""
    c = gc.g5(M, N, K, w_bits)
    ref = gc.gelu_ref(c.exact)
    bound = gc.g5_bound(ref)
    for variant, out, BM in _launches(ops, dev, c, epilogue=ops.EPI_GELU):
        what = "%s variant %d" % (c.name, variant)
        _assert_bound(out, ref, bound, what, BM)
        tail = out.cpu()[c.exact < -13]
        assert tail.numel() > 0 and bool((tail == 0).all()), what

"""The kernels outside the 28 blocks per output element, on operands whose result is known without a GPU library
(fp_edge_cases.py; the builders, the bounds and the mutants are proven by test_fp_edge_cases_cpu.py).

vq_linear_f16: L1 (address), L2 (exact accumulation, the fp16 store at ties, 65504 / 65519 / 65520, subnormals and zero by
cancellation) and L4 (pitched, poisoned operands; a framed output) are compared BITWISE with the CPU expectation; L3 (all
63488 finite fp16 values through SiLU on either side and GELU on the output side) per element against the bounds derived
in fp_edge_cases.py and gemm_cases.py, with tolerance-free checks of finiteness and sign.  vq_cfg_ddim_step: S1 / S3
bitwise (the unused sigma half of the model outputs is NaN), S2 per element against the stated bound.  vq_adaln_table: A1
bitwise into a framed output.  Poison and sentinels are always inside an allocation the test owns.
"""
import pytest
import torch

import fp_edge_cases as fe

pytestmark = pytest.mark.gpu

SENTINEL = 0x5AA5       # fp16 bit pattern of a finite value (212.6) no case produces by the row
SENTINEL32 = 0x5AA55AA5


def _hex(t, i):
    return int(t.view(torch.int16)[i]) & 0xFFFF


def _assert_bits(out, expect, c, what):
    o, e = out.cpu(), expect
    if torch.equal(o.view(torch.int16), e.view(torch.int16)):
        return
    bad = o.view(torch.int16) != e.view(torch.int16)
    i = tuple(torch.nonzero(bad)[0].tolist())
    raise AssertionError("%s %s: %s; kernel %r (0x%04x), expected %r (0x%04x)" % (
        c.name, what, fe.first_mismatch(bad, c), float(o[i]), _hex(o, i), float(e[i]), _hex(e, i)))


def _assert_bound(out, c, what):
    o = out.cpu().double()
    diff = (o - c.exact).abs()
    bad = ~(diff <= c.bound)                                   # NaN is bad
    ratio = float((diff / c.bound)[~bad].max()) if bool((~bad).any()) else float("nan")
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError("%s %s: %s; kernel %r, reference %r, bound %.3e, worst error / bound %.3f" % (
            c.name, what, fe.first_mismatch(bad, c), float(o[i]), float(c.exact[i]), float(c.bound[i]),
            float((diff / c.bound)[~torch.isnan(diff)].max())))
    return ratio


def _run(ops, dev, c):
    out = ops.linear_f16(c.x.to(dev), c.w.to(dev), None if c.bias is None else c.bias.to(dev), act_in=c.act_in,
                         act_out=c.act_out)
    assert out.shape == (c.M, c.N) and out.dtype == torch.float16
    return out


# ------------------------------------------------------------------------------------------------------------ L1
@pytest.mark.parametrize("M,N,K", fe.LIN_SHAPES)
def test_l1_every_output_names_its_row_column_and_k(ops, dev, M, N, K):
    for phase in range(fe.l1_phases(M, K)):
        c = fe.l1(M, N, K, phase, bias=phase % 2 == 1)
        _assert_bits(_run(ops, dev, c), c.expect_half(), c, "dense")


# ------------------------------------------------------------------------------------------------------------ L2
@pytest.mark.parametrize("M,N,K", fe.LIN_SHAPES)
def test_l2_accumulation_and_bias_are_exact(ops, dev, M, N, K):
    for c in (fe.l2(M, N, K), fe.l2(M, N, K, seed=1, bias=False)):
        _assert_bits(_run(ops, dev, c), c.expect_half(), c, "dense")


@pytest.mark.parametrize("M,N,K", fe.LIN_SHAPES)
def test_l2_store_rounds_to_nearest_even_at_ties_edges_and_subnormals(ops, dev, M, N, K):
    c = fe.l2_landing(M, N, K)
    _assert_bits(_run(ops, dev, c), c.expect_half(), c, "dense")


# ------------------------------------------------------------------------------------------------------------ L3
@pytest.mark.parametrize("act_in,act_out,bias_kind", fe.L3_CASES)
def test_l3_activation_over_every_finite_fp16_value(ops, dev, parity, act_in, act_out, bias_kind):
    """fp64 reference of the activation at its exact fp32 argument; bound = one fp16 ulp of the reference (floor 2^-24) +
    the relative error of the v_exp_f32 / v_rcp_f32 formula (fp_edge_cases.SILU_REL, gemm_cases.G5_REL).  The count of
    outputs that differ from RN(fp64) is recorded, not asserted: the hardware's exp2 and rcp decide it."""
    c = fe.l3(act_in, act_out, bias_kind)
    out = _run(ops, dev, c).cpu()
    bad = fe.l3_sign_violations(out, c)
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError("%s: %s; argument %r gives %r (0x%04x)" % (c.name, fe.first_mismatch(bad, c),
                                                                       float(c.extra["v"][i]), float(out[i]), _hex(out, i)))
    ratio = _assert_bound(out, c, "sweep")
    differ = int((out != c.exact.float().half()).sum())                 # by value: a zero of either sign is 0
    print("%s: worst error / bound %.3f; %d of 63488 outputs differ from RN(fp64)" % (c.name, ratio, differ))
    parity["fp_edge/" + c.name] = {"worst_error_over_bound": ratio, "differ_from_rn_fp64": differ}


# ------------------------------------------------------------------------------------------------------------ L4
def _abi_linear(dev, c, xa, wa, ldo):
    """vq_linear_f16 through the C ABI on arenas: returns (out arena [2 + M + 2, ldo] as int16, its [M, N] fp16 view)."""
    from viditq_amd import _lib
    M, N, K = c.M, c.N, c.K
    oa = torch.full((M + 4, ldo), SENTINEL, dtype=torch.int16, device=dev)
    b = None if c.bias is None else c.bias.to(dev)
    _lib.check(_lib.load().vq_linear_f16(xa.data_ptr(), wa.data_ptr(), None if b is None else b.data_ptr(), oa[2:].data_ptr(),
                                         M, N, K, xa.stride(0), wa.stride(0), ldo, c.act_in, c.act_out,
                                         torch.cuda.current_stream().cuda_stream), "vq_linear_f16")
    torch.cuda.synchronize()
    return oa, oa[2:2 + M, :N].view(torch.float16)


def _frame_untouched(oa, M, N):
    return (bool((oa[:2] == SENTINEL).all()) and bool((oa[2 + M:] == SENTINEL).all())
            and bool((oa[2:2 + M, N:] == SENTINEL).all()))


@pytest.mark.parametrize("dx,dw,do", fe.L4_PITCHES)
@pytest.mark.parametrize("M,N,K", fe.L4_SHAPES)
def test_l4_pitched_poisoned_operands_and_a_framed_output(ops, dev, M, N, K, dx, dw, do):
    """ldx, ldw > K with NaN in every gap column and in rows at and beyond M / N; out rows ldo > N apart between guard
    rows of sentinels: bit-identical to the dense launch and to the CPU expectation, every sentinel untouched."""
    for c in (fe.l1(M, N, K, bias=True), fe.l2(M, N, K), fe.l2_landing(M, N, K)):
        dense = _run(ops, dev, c)
        _assert_bits(dense, c.expect_half(), c, "dense")
        xa, wa = fe.arena(c.x, K + dx, 3).to(dev), fe.arena(c.w, K + dw, 5).to(dev)
        oa, out = _abi_linear(dev, c, xa, wa, N + do)
        what = "pitches ldx = K + %d, ldw = K + %d, ldo = N + %d" % (dx, dw, do)
        assert _frame_untouched(oa, M, N), "%s %s: wrote outside [0, M) x [0, N)" % (c.name, what)
        _assert_bits(out, c.expect_half(), c, what)
        assert torch.equal(out.view(torch.int16), dense.view(torch.int16))
        # dense operands through the C ABI as well: pitches K, K, N inside the same frame
        oa, out = _abi_linear(dev, c, c.x.to(dev), c.w.to(dev), N)
        assert _frame_untouched(oa, M, N), c.name + " dense ABI launch: wrote outside its rows"
        _assert_bits(out, c.expect_half(), c, "dense ABI launch")
        # the host route: a column slice of a wider matrix for x and for w (ops.linear_f16 forwards both row pitches)
        got = ops.linear_f16(xa[:M, :K], wa[:N, :K], None if c.bias is None else c.bias.to(dev))
        _assert_bits(got, c.expect_half(), c, "ops.linear_f16 on sliced views")


# ------------------------------------------------------------------------------------------------------- sampler
def _first_diff(got, want, what):
    bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
    i = tuple(bad[0].tolist())
    return "%s: %d differ, first at (b, c, inner) = %s: expected %r, kernel %r" % (what, bad.shape[0], i, want[i].item(),
                                                                                   got[i].item())


def _step(ops, dev, s):
    """The launch into the middle of a sentinel-framed buffer that starts as NaN where the kernel must write."""
    big = torch.full((s.n + 2, s.C, s.inner), SENTINEL32, dtype=torch.int32, device=dev).view(torch.float32)
    out = big[1:1 + s.n]
    out.fill_(float("nan"))
    x = s.x.to(dev)
    got = ops.cfg_ddim_step(s.cond.to(dev), s.uncond.to(dev), x, *s.params(), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    frame = big.view(torch.int32)
    assert bool((frame[0] == SENTINEL32).all()) and bool((frame[-1] == SENTINEL32).all()), s.name + ": wrote outside x_out"
    assert torch.equal(x.cpu(), s.x), s.name + ": x changed"
    return got.cpu()


def test_s1_sampler_step_is_exact_for_every_parameter_set(ops, dev):
    for p in fe.S1_PARAMS:
        s = fe.s1(2, 4, 129, p)
        got, want = _step(ops, dev, s), s.exact.float()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), _first_diff(got, want, s.name)


def test_s2_sampler_step_at_both_ends_of_the_schedule(ops, dev, parity):
    """fp64 formula; |error| <= 16 2^-24 T (sa + sb / |Bc|) per element (fp_edge_cases.s2: 16 roundings on the longest
    path)."""
    worst = 0.0
    for i, p in enumerate(fe.S2_PARAMS):
        s = fe.s2(2, 4, 257, p, seed=i)
        got = _step(ops, dev, s).double()
        diff = (got - s.exact).abs()
        bad = ~(diff <= s.bound)
        if bool(bad.any()):
            j = tuple(torch.nonzero(bad)[0].tolist())
            raise AssertionError("%s: %d outside the bound, first at (b, c, inner) = %s: kernel %r, reference %r, bound %.3e" % (
                s.name, int(bad.sum()), j, float(got[j]), float(s.exact[j]), float(s.bound[j])))
        worst = max(worst, float((diff / s.bound).max()))
    print("S2 worst error / bound over %d parameter sets: %.3f" % (len(fe.S2_PARAMS), worst))
    parity["fp_edge/s2"] = {"worst_error_over_bound": worst}


@pytest.mark.parametrize("n,C,inner", fe.S3_SHAPES)
def test_s3_sampler_shapes_second_pass_three_and_eight_channels(ops, dev, n, C, inner):
    """1.31 M elements (the grid-stride loop's second pass), one element, C = 3 (every channel guided), C = 8 (five
    pass-through channels).  The scheduler hands the kernel a second buffer as ``out`` and swaps the two after the step
    (t2v/iddpm.py: ``x, buf = out, x``) - never x itself - so that is the launch tested: x must come back unchanged."""
    for p in (fe.S1_PARAMS[3], fe.S1_PARAMS[40]):
        s = fe.s1(n, C, inner, p, "S3")
        got, want = _step(ops, dev, s), s.exact.float()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), _first_diff(got, want, s.name)


# --------------------------------------------------------------------------------------------------------- AdaLN
@pytest.mark.parametrize("B,J,C", fe.A1_SHAPES)
def test_a1_adaln_table_is_one_ieee_add_per_element(ops, dev, B, J, C):
    from viditq_amd import _lib
    table, t0, want = fe.a1(B, J, C)
    n, pad = B * J * C, 1024
    buf = torch.full((n + 2 * pad,), SENTINEL32, dtype=torch.int32, device=dev)
    td, sd = table.to(dev), t0.to(dev)
    _lib.check(_lib.load().vq_adaln_table(td.data_ptr(), sd.data_ptr(), buf[pad:].data_ptr(), B, J, C,
                                          torch.cuda.current_stream().cuda_stream), "vq_adaln_table")
    torch.cuda.synchronize()
    assert bool((buf[:pad] == SENTINEL32).all()) and bool((buf[pad + n:] == SENTINEL32).all()), "wrote outside mod"
    got = buf[pad:pad + n].view(torch.float32).reshape(J, B, C).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), _first_diff(got, want, "adaln %dx%dx%d" % (B, J, C))
    # and the host wrapper
    mod = ops.adaln_table(td, sd).cpu()
    assert torch.equal(mod.view(torch.int32), want.view(torch.int32)), _first_diff(mod, want, "ops.adaln_table")

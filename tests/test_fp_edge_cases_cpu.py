"""What test_fp_edge_exact_gpu.py relies on, proven without a GPU: the exact families of fp_edge_cases.py are exact
(int64 / fp64 proofs), the CPU reference that reads the operands the kernel's way reproduces every expectation, the two
bounds hold for the reference arithmetic alone (fp32 step-by-step evaluation of the kernels' formulas), and every mutant
of the reference - one subtly wrong kernel each - is caught by the family that claims to catch it."""
import pytest
import torch

import fp_edge_cases as fe

MUTANT_SHAPES = [(17, 16, 24), (130, 36, 32), (77, 36, 72), (77, 36, 520), (17, 36, 504)]


def _bits(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------------------ linear
@pytest.mark.parametrize("M,N,K", fe.LIN_SHAPES)
def test_l1_l2_cases_are_exact_and_the_reference_reproduces_them(M, N, K):
    cases = [fe.l1(M, N, K), fe.l1(M, N, K, fe.l1_phases(M, K) - 1, bias=True), fe.l2(M, N, K), fe.l2(M, N, K, bias=False),
             fe.l2_landing(M, N, K)]
    for c in cases:
        total = fe.prove_exact(c)
        assert total <= fe.TWO24
        assert float(c.x.abs().max()) <= 8 and float(c.w.double().abs().max()) <= 8 * 4096
        ref = fe.reference(c)
        assert torch.equal(ref, c.exact), c.name
        assert torch.equal(_bits(fe.reference_half(c)), _bits(c.expect_half())), c.name
    c = cases[0]
    assert int(c.exact.abs().max()) < 2048 and int(c.extra["k"][0]) == K - 1
    assert torch.equal(c.exact, (c.extra["v"][:, None] * fe.l1_weights(N, K)[:, c.extra["k"]].t()).double())


@pytest.mark.parametrize("K", sorted({s[2] for s in fe.LIN_SHAPES}))
def test_l1_phases_meet_every_k_where_the_rows_suffice(K):
    for M, N, K_ in fe.LIN_SHAPES:
        if K_ != K:
            continue
        P = fe.l1_phases(M, K)
        seen = torch.cat([fe.l1_k(M, K, p) for p in range(P)]).unique()
        assert seen.numel() == min(K, P * M)
        assert K - 1 in seen.tolist()
    w = fe.l1_weights(36, K)
    k = torch.arange(K)
    if K % 16 == 0:
        assert bool((w != w[:, k ^ 8]).all())                    # a lane group against its neighbour's weights shows
    assert bool((w[:-1] != w[1:]).all()) and int(w.abs().max()) <= 30


def test_l2_landing_meets_every_value_it_is_there_for():
    census = fe.landing_census([fe.l2_landing(M, N, K) for M, N, K in fe.LIN_SHAPES if M >= 63 and N >= 20])
    print("L2 landing census:", census)
    for name, count in census.items():
        assert count > 0, name


@pytest.mark.parametrize("M,N,K", fe.L4_SHAPES)
def test_l4_reference_through_pitched_arenas_reads_no_poison(M, N, K):
    for dx, dw, _ in fe.L4_PITCHES:
        for c in (fe.l1(M, N, K), fe.l2(M, N, K), fe.l2_landing(M, N, K)):
            xa, wa = fe.arena(c.x, K + dx, 3), fe.arena(c.w, K + dw, 5)
            assert int(torch.isnan(xa).sum()) == xa.numel() - M * K
            assert torch.equal(fe.reference(c, None, xa, wa), c.exact)


# ---------------------------------------------------------------------------------------------------------------- L3
def test_l3_bounds_hold_for_the_fp32_formulas_and_the_sweep_is_complete():
    x = fe.all_finite_halves()
    b = _bits(x.reshape(-1)).long() & 0xFFFF
    assert b.unique().numel() == 63488 and bool(torch.isfinite(x).all())
    assert abs(fe.SILU_REL - (0.6931471805599453 * 2 * 2.0 ** -24 * 126 + 2 * 2.0 ** -23 + 2 * 2.0 ** -24)) < 1e-20
    worst = {}
    for ai, ao, bk in fe.L3_CASES:
        c = fe.l3(ai, ao, bk)
        assert bool(torch.isfinite(c.exact).all())
        got = fe.act_formula_fp32(c.extra["act"], c.extra["v"]).half()
        assert not bool(fe.l3_sign_violations(got, c).any()), c.name
        ratio = float(((got.double() - c.exact).abs() / c.bound).max())
        differ = int((got != c.exact.float().half()).sum())       # by value; recorded, not asserted
        print("%s: fp32 formula at %.3f of the bound; %d of 63488 differ from RN(fp64)" % (c.name, ratio, differ))
        worst[c.extra["act"]] = max(worst.get(c.extra["act"], 0.0), ratio)
        assert ratio <= 1.0, c.name
    print("L3 worst error / bound of the fp32 formulas: SiLU %.3f, GELU %.3f" % (worst[fe.ACT_SILU], worst[fe.ACT_GELU]))
    # the identity weight makes the accumulator x itself: the reference the kernel's way agrees with the closed form
    c = fe.l3(fe.ACT_NONE, fe.ACT_GELU, fe.L3_BIAS_MIXED)
    assert torch.equal(fe.reference(c), c.exact)
    c = fe.l3(fe.ACT_SILU, fe.ACT_NONE)
    assert bool(((fe.reference(c) - c.exact).abs() <= c.bound).all())
    assert int((c.bias if c.bias is not None else torch.zeros(1)).abs().sum()) == 0
    mixed = fe.l3_bias(fe.L3_BIAS_MIXED)
    assert bool((mixed > 0).any()) and bool((mixed < 0).any()) and bool((mixed == 0).any())


# ----------------------------------------------------------------------------------------------------------- mutants
def _linear_family_cases(family):
    if family == "L1":
        return [(fe.l1(M, N, K, p, bias=bool(p)), None, None) for M, N, K in MUTANT_SHAPES for p in (0, 1)]
    if family == "L2":
        return [(c, None, None) for M, N, K in MUTANT_SHAPES for c in (fe.l2(M, N, K), fe.l2_landing(M, N, K))]
    if family == "L3":
        return [(fe.l3(*a), None, None) for a in fe.L3_CASES]
    out = []
    for M, N, K in fe.L4_SHAPES:
        for dx, dw, _ in fe.L4_PITCHES:
            c = fe.l1(M, N, K)
            out.append((c, fe.arena(c.x, K + dx, 3), fe.arena(c.w, K + dw, 5)))
    return out


def _caught(c, mutant, xa, wa):
    got = fe.reference_half(c, mutant, xa, wa)
    if c.bound is None:
        return not torch.equal(_bits(got), _bits(c.expect_half()))
    return bool((~((got.double() - c.exact).abs() <= c.bound)).any())


@pytest.mark.parametrize("mutant", fe.LINEAR_MUTANTS)
def test_every_linear_mutant_fails_the_family_that_claims_it(mutant):
    family = fe.LINEAR_MUTANT_FAMILY[mutant]
    cases = _linear_family_cases(family)
    for c, xa, wa in cases:
        assert not _caught(c, None, xa, wa), c.name            # the unmutated reference passes every case
    hit = [c.name for c, xa, wa in cases if _caught(c, mutant, xa, wa)]
    print("%s: caught by %d of %d %s cases" % (mutant, len(hit), len(cases), family))
    assert hit, (mutant, family)


# ----------------------------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("n,C,inner", [(2, 4, 129)] + fe.S3_SHAPES)
def test_s1_every_intermediate_is_exact(n, C, inner):
    params = fe.S1_PARAMS if n * C * inner < 100000 else fe.S1_PARAMS[::7]
    assert len(fe.S1_PARAMS) == 72
    for p in params:
        s = fe.s1(n, C, inner, p)
        assert fe.s1_prove(s) < 2.0 ** 13
        assert int(torch.isnan(s.cond).sum()) == n * C * inner and bool(torch.isnan(s.cond[:, C:]).all())
        # the fp32 evaluation of the same lines gives the same bits
        assert torch.equal(fe.sampler_reference(s, dtype=torch.float32), s.exact.float())
    assert float(s.cond[:, :C].abs().max()) <= 8 and torch.equal(s.x * 16, (s.x * 16).round())


def test_s2_bound_holds_for_the_fp32_evaluation():
    assert len(fe.S2_PARAMS) == 28 and fe.S2_ROUNDINGS == 16
    worst = 0.0
    for i, p in enumerate(fe.S2_PARAMS):
        s = fe.s2(2, 4, 257, p, seed=i)
        got = fe.sampler_reference(s, dtype=torch.float32)
        ratio = float(((got.double() - s.exact).abs() / s.bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, s.name
    print("S2 worst error / bound of the fp32 evaluation over %d parameter sets: %.3f" % (len(fe.S2_PARAMS), worst))
    ab = [1.0 / (1.0 + p[3] ** 2) for p in fe.S2_PARAMS]
    assert max(ab) > 0.9998 and min(ab) < 4.7e-5


def _sampler_family_cases(family):
    if family == "S3":
        return [fe.s1(n, C, inner, fe.S1_PARAMS[3], "S3") for n, C, inner in fe.S3_SHAPES]
    return [fe.s1(2, 4, 129, p) for p in fe.S1_PARAMS[::5]] + [fe.s1(2, 8, 33, fe.S1_PARAMS[20])]


@pytest.mark.parametrize("mutant", fe.SAMPLER_MUTANTS)
def test_every_sampler_mutant_fails_the_family_that_claims_it(mutant):
    family = fe.SAMPLER_MUTANT_FAMILY[mutant]
    cases = _sampler_family_cases(family)
    hit = []
    for s in cases:
        got = fe.sampler_reference(s, mutant).float()
        want = s.exact.float()
        if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
            hit.append(s.name)
    print("%s: caught by %d of %d %s cases" % (mutant, len(hit), len(cases), family))
    assert hit, (mutant, family)
    assert fe.S3_SHAPES[0][0] * fe.S3_SHAPES[0][1] * fe.S3_SHAPES[0][2] > fe.FIRST_PASS


# ------------------------------------------------------------------------------------------------------------- AdaLN
@pytest.mark.parametrize("B,J,C", fe.A1_SHAPES)
def test_a1_sum_rounds_in_fp32_and_leaves_fp16(B, J, C):
    table, t0, want = fe.a1(B, J, C)
    assert want.shape == (J, B, C) and want.dtype == torch.float32
    exact = table.double()[:, None, :] + t0.double().reshape(B, J, C).permute(1, 0, 2)
    assert int((want.double() != exact).sum()) >= 3            # 65504 +- 2^-24 is not an fp32 number
    assert float(want.abs().max()) == 131008.0
    assert torch.equal(want, exact.float())

"""CPU checks behind test_gemm_exact_gpu.py: the operand families of gemm_cases.py are what their names say - fields
written the way csrc/gemm_i8.hip reads them, exactness claims re-evaluated in fp32 torch in three association orders,
bounds that hold for an fp32 evaluation, chosen fp16 landing values present - and every family changes, beyond its own
tolerance, under the wrong kernels it claims to catch."""
import math

import pytest
import torch

import gemm_cases as gc

BITS = [(8, 8), (8, 6), (8, 4), (6, 8), (6, 6), (6, 4)]


def _g2(M, N, K, ab, wb, **kw):
    return gc.g2(M, N, K, ab, wb, zw_span=gc.g2_zw_span(K, ab, wb), **kw)


def _bits_differ(a, b):
    return a.view(torch.int16) != b.view(torch.int16)


# ------------------------------------------------------------------------------------------------ operand fields
@pytest.mark.parametrize("Kp", [128, 256, 1152])
def test_nibble_packer_round_trips_through_the_decode_of_the_kernel_tests(Kp):
    codes = torch.randint(0, 16, (37, Kp), generator=torch.Generator().manual_seed(Kp)).to(torch.int8)
    wq = gc.pack_nibbles(codes)
    assert wq.dtype == torch.uint8 and wq.shape == (37, Kp // 2)
    assert torch.equal(gc.unpack_nibbles(wq), codes)
    # pack.hip: byte j of a group of 8 k = code[k0 + j] (low nibble), code[k0 + 4 + j] (high nibble)
    for k0, j in ((0, 0), (8, 3), (Kp - 8, 2)):
        byte = wq[:, k0 // 2 + j].int()
        assert torch.equal(byte & 15, codes[:, k0 + j].int()) and torch.equal(byte >> 4, codes[:, k0 + 4 + j].int())


def _family_samples():
    out = [gc.g1(300, 292, 200, 8), gc.g1(130, 580, 1100, 4)]
    out += [_g2(130, 580, 200, ab, wb) for ab, wb in BITS] + [_g2(5, 292, 72, 8, 8, bias=False), _g2(1, 4, 1, 8, 4)]
    out += [gc.g3(34, 52, 4608, 8), gc.g3(34, 52, 16380, 4)]
    out += [gc.g4(300, 292, 200, 8), gc.g4(130, 580, 72, 4, edges=True), gc.g4_resid(300, 292, 200, 8, 100)[0]]
    out += [gc.g5(300, 292, 200, 8), gc.g5(257, 1156, 72, 4)]
    return out


@pytest.mark.parametrize("c", _family_samples(), ids=lambda c: c.name)
def test_fields_are_written_the_way_the_kernels_read_them(c):
    cx, cw = gc.centre(c.a_bits), gc.centre(c.w_bits)
    assert (cx, cw) == (128 if c.a_bits == 8 else 0, 128 if c.w_bits == 8 else 0)
    Kp = (c.K + 127) // 128 * 128
    assert c.xq.dtype == torch.int8 and c.xq.shape == (c.M, Kp) and bool((c.xq[:, c.K:] == 0).all())
    ws = gc.unpack_nibbles(c.wq) if c.w_bits <= 4 else c.wq
    assert c.wq.dtype == (torch.uint8 if c.w_bits <= 4 else torch.int8) and ws.shape == (c.N, Kp)
    assert bool((ws[:, c.K:] == 0).all())
    if c.x_raw is not None:
        assert torch.equal(c.xq[:, :c.K].long(), c.x_raw.long() - cx)
    assert torch.equal(ws[:, :c.K].long(), c.w_raw.long() - cw)
    assert torch.equal(c.zx.long(), c.zx_raw.long() - cx) and torch.equal(c.zw.long(), c.zw_raw.long() - cw)
    assert torch.equal(c.R.long(), c.xq[:, :c.K].long().sum(1) - c.K * c.zx.long())      # R = rowsum - K zx
    assert torch.equal(c.cs.long(), ws[:, :c.K].long().sum(1))                            # cs = sum(code - cw)
    for t, dt in ((c.sx, torch.float32), (c.sw, torch.float32), (c.zx, torch.int32), (c.R, torch.int32),
                  (c.zw, torch.int32), (c.cs, torch.int32)):
        assert t.dtype == dt
    # the expectation follows from the packed operands alone
    assert torch.equal(gc.reference(c).double(), c.exact.double())


# ------------------------------------------------------------------------------------------------------------ G1
@pytest.mark.parametrize("K", [1, 72, 200, 1100, 1152, 4608])
def test_g1_rows_meet_every_k(K):
    kk = gc.g1_k(K, K)                                            # K consecutive rows
    assert int(kk[0]) == K - 1 and sorted(kk.tolist()) == list(range(K))
    if K >= 128:
        hit = set(kk.tolist())
        assert all(k in hit for k in range(127, K, 128))          # the last k before each 128-byte line


@pytest.mark.parametrize("w_bits", [8, 6, 4])
def test_g1_names_its_element(w_bits):
    c = gc.g1(300, 292, 200, w_bits)
    L = 2 ** w_bits
    assert set(c.w_raw.reshape(-1).tolist()) == set(range(L))     # the whole code range
    assert int(c.exact.abs().max()) <= 7 * 128
    # neighbours in m, n differ almost everywhere: a value says where it came from
    e = c.exact
    assert float((e[1:] != e[:-1]).float().mean()) > 0.95 and float((e[:, 1:] != e[:, :-1]).float().mean()) > 0.9


@pytest.mark.parametrize("M,N,K", gc.BENCH_SHAPES)
def test_g1_builds_at_the_benchmark_sizes_without_a_matmul(M, N, K):
    c = gc.g1(M, N, K, 4 if N == 4608 else 8)
    assert c.exact.shape == (M, N) and c.exact.dtype == torch.int16
    rows = torch.tensor([0, 1, 255, 256, M // 2 + 17, M - 1])
    ws = gc.unpack_nibbles(c.wq) if c.w_bits <= 4 else c.wq
    dense = c.xq[rows].double() @ ws.double().t()
    assert torch.equal(dense, c.exact[rows].double())


# ------------------------------------------------------------------------------------------------- G2 / G4 exact
def _exact_cases():
    out = [_g2(M, N, K, ab, wb) for (M, N, K) in [(130, 580, 200), (257, 1156, 1100), (5, 292, 72), (1, 4, 1)] for ab, wb in BITS]
    out += [_g2(256, 288, 128, 8, 8), _g2(512, 576, 256, 8, 4), _g2(300, 4, 200, 8, 8, bias=False)]
    out += [gc.g4(300, 292, 200, 8), gc.g4(300, 292, 1100, 4), gc.g4(130, 580, 72, 8, edges=True), gc.g4(130, 580, 72, 4, edges=True)]
    out += [gc.g4_resid(300, 292, 200, 8, 100)[0], gc.g4_resid(512, 576, 256, 4, 256)[0], gc.g4_resid(513, 580, 72, 8)[0]]
    out += [gc.g5(300, 292, 200, 8), gc.g5(257, 1156, 72, 4)]
    return out


@pytest.mark.parametrize("c", _exact_cases(), ids=lambda c: c.name)
def test_exact_families_are_exact_in_fp32_in_every_association_order(c):
    total = gc.prove_exact(c)
    assert total <= 2 ** 24
    for order in (0, 1, 2):
        y32 = gc.reference(c, order=order, dtype=torch.float32)
        assert y32.dtype == torch.float32
        assert torch.equal(y32.double(), c.exact), order
    # the integer form: one int32, one conversion, mul + add
    t_w, t_x = c.terms()
    tt = (c.acc - t_w - t_x)
    assert int(tt.abs().max()) <= 2 ** 24
    S32 = c.sx[:, None] * c.sw[None, :]
    yi = S32 * tt.float() + (0.0 if c.bias is None else c.bias[None, :])
    assert torch.equal(yi.double(), c.exact)


@pytest.mark.parametrize("ab,wb", BITS)
def test_g2_parameters_move_with_the_index_and_reach_both_ends(ab, wb):
    c = _g2(130, 580, 200, ab, wb)
    assert bool((c.sx[1:] != c.sx[:-1]).all()) and bool((c.sw[1:] != c.sw[:-1]).all())
    assert int(c.x_raw.min()) == 0 and int(c.x_raw.max()) == 2 ** ab - 1
    assert int(c.w_raw.min()) == 0 and int(c.w_raw.max()) == 2 ** wb - 1
    assert {0, 2 ** ab - 1} <= set(c.zx_raw.tolist()) and {0, 2 ** wb - 1} <= set(c.zw_raw.tolist())
    assert len(set(c.zx_raw.tolist())) > 2 ** ab // 4 and len(set(c.zw_raw.tolist())) >= 2 ** wb // 2


# ------------------------------------------------------------------------------------------------------------ G3
@pytest.mark.parametrize("K,w_bits", [(4608, 8), (16380, 8), (4608, 4), (16380, 4)])
def test_g3_reaches_the_extremes_and_an_fp32_evaluation_stays_inside_its_bound(K, w_bits):
    c = gc.g3(130, 292, K, w_bits)
    hi_w = 127 if w_bits == 8 else 15
    lo_w = -128 if w_bits == 8 else 0
    assert int(c.acc.max()) == (K * 128 * 128 if w_bits == 8 else K * 127 * 15)
    assert int(c.acc.min()) == -K * 128 * hi_w
    assert int((c.acc == 0).sum()) > c.acc.numel() // 8 and K % 2 == 0   # +-127 against a constant row cancels
    assert int(c.R.abs().max()) == 255 * K and int(c.R.abs().max()) < 2 ** 23       # all 127 against zero point -128
    assert int(c.cs.abs().max()) == K * max(abs(lo_w), hi_w)
    t_w, t_x = c.terms()
    assert int(t_w.abs().max()) == max(abs(lo_w), hi_w) * 255 * K
    assert int(t_x.abs().max()) == 128 * K * max(abs(lo_w), hi_w)
    if w_bits == 8:
        assert int(c.acc.abs().max()) > 2 ** 24                          # float(acc) itself rounds
    ref, bound = gc.g3_bound(c)
    assert bool(torch.isfinite(ref).all())
    for order in (0, 1, 2):
        y32 = gc.reference(c, order=order, dtype=torch.float32)
        slack = bound - 2.0 ** -10 * ref.abs().clamp(min=2.0 ** -14).double()
        assert bool(((y32.double() - c.exact).abs() <= slack).all())
        assert bool(((y32.half().double() - ref.double()).abs() <= bound).all())
    # cancellation: the terms are many times the result on a good share of the outputs
    terms = (c.acc.abs() + t_w.abs() + t_x.abs()).double()
    tt = (c.acc - t_w - t_x).abs().double()
    assert float((terms > 8 * tt).float().mean()) > 0.1


# ------------------------------------------------------------------------------------------------------------ G4
def _tie_info(e):
    """(is a tie between fp16 neighbours, parity of the lower neighbour) of fp64 values."""
    _, ex = torch.frexp(e)
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), (ex - 11).clamp(min=-24).double())
    h = e.float().half().double()
    tie = ((e - h).abs() == ulp / 2) & torch.isfinite(h)
    lower = torch.floor(e.abs() / ulp)
    return tie, lower.long() % 2


@pytest.mark.parametrize("w_bits", [8, 4])
def test_g4_lands_on_the_chosen_values(w_bits):
    c = gc.g4(300, 292, 200 if w_bits == 8 else 1100, w_bits)
    e, h = c.exact, c.expect_half()
    tie, par = _tie_info(e)
    normal = e.abs() >= 2.0 ** -14
    for sign in (1, -1):
        for p in (0, 1):
            assert int((tie & normal & (par == p) & (torch.sign(e) == sign)).sum()) >= 8, (sign, p)
    assert int((tie & ~normal & (par == 0)).sum()) > 0 and int((tie & ~normal & (par == 1)).sum()) > 0
    for v in (2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -24, -2.0 ** -25):
        assert int((e == v).sum()) > 0, v
    assert bool((h[e == 2.0 ** -25] == 0).all()) and bool((h[e == 3 * 2.0 ** -25] == 2.0 ** -23).all())
    for v, r in ((65504.0, 65504.0), (65512.0, 65504.0), (65520.0, math.inf), (-65504.0, -65504.0), (-65512.0, -65504.0),
                 (-65520.0, -math.inf)):
        assert int((e == v).sum()) > 0 and bool((h[e == v] == r).all()), v
    zero = e == 0
    b = c.bias.double()[None, :].expand_as(e)
    assert int((zero & (b > 0)).sum()) > 0 and int((zero & (b < 0)).sum()) > 0      # cancellation from both signs
    assert bool((h[zero].view(torch.int16) == 0).all())                              # +0
    # the zero-point terms are live: far larger than the result
    t_w, t_x = c.terms()
    assert int(t_x.abs().max()) > 2 ** 19 and int(c.acc.abs().max()) > 2 ** 19


@pytest.mark.parametrize("w_bits", [8, 4])
def test_g4_edges_hold_the_fp32_predecessor_of_65520(w_bits):
    c = gc.g4(130, 580, 72, w_bits, edges=True)
    e, h = c.exact, c.expect_half()
    pred = 65520.0 - 2.0 ** -8
    assert float(torch.tensor(pred).float()) == pred and float(torch.nextafter(torch.tensor(pred), torch.tensor(1e9))) == 65520.0
    for sign in (1.0, -1.0):
        assert int((e == sign * pred).sum()) > 0 and bool((h[e == sign * pred] == sign * 65504.0).all())
        assert int((e == sign * 65520.0).sum()) > 0 and bool(torch.isinf(h[e == sign * 65520.0]).all())


@pytest.mark.parametrize("M,N,K,w_bits,rpg", [(300, 292, 200, 8, 0), (300, 292, 200, 8, 100), (512, 576, 256, 4, 256),
                                              (513, 580, 72, 8, 171)])
def test_g4_residual_cases_hold_zero_sums_ties_and_the_65520_crossing(M, N, K, w_bits, rpg):
    c, resid, gate, expected = gc.g4_resid(M, N, K, w_bits, rpg)
    kind = c.extra["kind"]
    yh = c.expect_half().float()
    z = yh if gate is None else gate[torch.arange(M) // rpg] * yh
    if gate is not None:
        assert gc.is_pow2(gate) and len(set(gate.reshape(-1).tolist())) == 3
    assert bool((expected[kind == 0].view(torch.int16) == 0).all())                  # resid = -g half(y): +0
    s = resid.double() + z.double()
    tie, par = _tie_info(s)
    k1 = (kind == 1) & c.extra["ok_tie"]
    assert int(k1.sum()) > (kind == 1).sum() // 4 and bool(tie[k1].all())
    assert int((k1 & (par == 0)).sum()) > 16 and int((k1 & (par == 1)).sum()) > 16
    k2 = kind == 2
    assert int((k2 & torch.isinf(expected)).sum()) > 16 and int((k2 & (expected.abs() == 65504)).sum()) > 16
    assert bool((s[k2 & torch.isinf(expected)].abs() >= 65520).all())
    assert torch.equal(expected, s.float().half())        # the fp32 sum is exact or cannot move the rounding


# ------------------------------------------------------------------------------------------------------------ G5
@pytest.mark.parametrize("w_bits,N,K", [(8, 292, 200), (4, 1156, 72)])
def test_g5_sweep_covers_the_grid_and_the_formula_error_is_inside_the_derived_term(w_bits, N, K):
    c = gc.g5(300, N, K, w_bits)
    y = c.exact
    vals = set((y[(y.abs() <= 12)] * 64).reshape(-1).tolist())
    assert all(float(t) in vals for t in range(-768, 769)), "every multiple of 2^-6 in [-12, 12]"
    for step in (2.0 ** -10, 2.0 ** -14, 2.0 ** -18, 2.0 ** -24):
        assert int(((y.abs() == step)).sum()) > 0
    assert 5.5e4 < float(y.max()) < 65504 and -65504 < float(y.min()) < -5.5e4
    ref = gc.gelu_ref(y)
    head = y > -3                                                                # (1 + tanh cancels in the library's negative tail)
    assert torch.allclose(ref[head], torch.nn.functional.gelu(y[head], approximate="tanh"), rtol=1e-9, atol=1e-300)
    sub = (ref.abs() < 2.0 ** -14) & (ref.abs() >= 2.0 ** -25)
    assert int((sub & (y < -4)).sum()) > 32 and int((sub & (y.abs() < 1e-3)).sum()) > 32   # subnormal results, both regions
    assert int((y < -13).sum()) > 32
    f32 = gc.gelu_formula_fp32(y)
    assert not bool(torch.isnan(f32).any())
    assert bool((f32[y < -13] == 0).all())
    # same formula in fp32 on the CPU: inside the derived relative term; where |w| passes 126 the exponential leaves the
    # fp32 range and the result, below 2^-126 |y| <= 2^-120, may flush to zero
    assert bool(((f32.double() - ref).abs() <= gc.G5_REL * ref.abs() + 2.0 ** -120).all())
    assert gc.G5_REL < 2.0 ** -11 / 16
    b = gc.g5_bound(ref)
    assert bool((b >= 2.0 ** -24).all()) and bool(((f32.half().double() - ref).abs() <= b).all())


# ------------------------------------------------------------------------------------------------------- mutants
TOKEN = 16      # a mutant must move more elements than this, beyond the family's tolerance


def _moved_bitwise(c, mutant):
    return int(_bits_differ(gc.reference_half(c, mutant), c.expect_half()).sum())


@pytest.mark.parametrize("w_bits", [8, 4])
def test_g1_has_teeth(w_bits):
    c = gc.g1(300, 292, 200, w_bits)
    for mutant in ("kswap", "droplast") + (("nibswap",) if w_bits == 4 else ()):
        assert _moved_bitwise(c, mutant) > TOKEN, mutant


@pytest.mark.parametrize("ab,wb", [(8, 8), (8, 4), (6, 6)])
def test_g2_has_teeth(ab, wb):
    c = _g2(130, 580, 200, ab, wb)
    for mutant in gc.MUTANTS:
        if mutant == "nibswap" and wb > 4:
            continue
        assert _moved_bitwise(c, mutant) > TOKEN, mutant


@pytest.mark.parametrize("w_bits", [8, 4])
def test_g3_has_teeth(w_bits):
    c = gc.g3(130, 292, 4608, w_bits)
    ref, bound = gc.g3_bound(c)
    for mutant in ("row_m1", "col_n1", "droplast", "zpsign"):
        y = gc.reference(c, mutant).float().half().double()
        assert int(((y - ref.double()).abs() > bound).sum()) > TOKEN, mutant


@pytest.mark.parametrize("w_bits", [8, 4])
def test_g4_has_teeth(w_bits):
    c = gc.g4(300, 292, 200 if w_bits == 8 else 1100, w_bits)
    for mutant in ("rtz", "row_m1", "col_n1", "zpsign"):
        assert _moved_bitwise(c, mutant) > TOKEN, mutant
    # the residual add: a round-toward-zero store of the sum moves the ties
    c, resid, gate, expected = gc.g4_resid(300, 292, 200, w_bits, 100)
    z = gate[torch.arange(300) // 100] * c.expect_half().float()
    assert int(_bits_differ(gc.rtz_half(resid.double() + z.double()), expected).sum()) > TOKEN


@pytest.mark.parametrize("w_bits", [8, 4])
def test_g5_has_teeth(w_bits):
    c = gc.g5(300, 292, 200, w_bits)
    ref = gc.gelu_ref(c.exact)
    bound = gc.g5_bound(ref)
    for mutant in ("row_m1", "col_n1", "zpsign"):
        y = gc.gelu_formula_fp32(gc.reference(c, mutant)).half().double()
        assert int(((y - ref).abs() > bound).sum()) > TOKEN, mutant
    # an erf-GELU epilogue is not the tanh form
    y = torch.nn.functional.gelu(c.exact.float()).half().double()
    assert int(((y - ref).abs() > bound).sum()) > TOKEN

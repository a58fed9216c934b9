"""CPU checks behind test_quantizer_edges_gpu.py: the row families of quant_rows.py are what their names say, judged
by oracle/fakequant.py alone (fp32, plus fp64 where a distance is measured), and no bit-exact launch of the GPU file
holds a row the oracle would eps-fill."""
import pytest
import torch

import quant_rows as qr
from oracle import fakequant as fq

# (B, C) of the launches of test_quantizer_edges_gpu.py
SHAPES = [(3, 64), (3, 96), (1, 1152), (1, 768), (1, 1024), (1, 1280), (1, 4608), (2, 1152), (2, 4608)]


def _rows(x):
    B, n, C = x.shape
    return x.permute(1, 0, 2).reshape(n, B * C)


@pytest.mark.parametrize("n_bits", [8, 6, 4])
@pytest.mark.parametrize("B,C", [(3, 64), (1, 1152), (2, 1152), (1, 4608), (1, 96)])
def test_q1_rows_are_exact_ties_on_a_power_of_two_grid(B, C, n_bits):
    qmax = 2 ** n_bits - 1
    x = qr.q1(B, 48, C, n_bits)
    codes, _, delta, zp, eps = fq.dyn_act_quant(x.float(), n_bits)
    assert not eps
    r = _rows(x).double()
    away = torch.zeros(48, dtype=torch.bool)
    for t in range(48):
        lo, hi, k = qr.q1_row_spec(t, n_bits)
        assert float(delta[0, t, 0]) == 2.0 ** -k                                  # exactly, in fp32
        assert float(zp[0, t, 0]) == -lo and int(zp[0, t, 0]) % 2 == (-lo) % 2
        q = r[t] * 2.0 ** k                                                        # exact: a power of two
        tie = (q - torch.floor(q)) == 0.5
        assert int(tie.sum()) == B * C - 2 and int(tie.sum()) >= min(qmax, B * C - 2)
        m = torch.floor(q[tie]).long()
        assert bool((m % 2 == 0).any()) and bool((m % 2 == 1).any())              # both tie parities in every row
        # half-even matters: the oracle's codes are not those of round-half-away-from-zero
        half_away = (torch.sign(q) * torch.floor(q.abs() + 0.5) - lo).clamp(0, qmax)
        away[t] = bool((half_away != _rows(codes)[t].double()).any())
        assert float(r[t].min()) == lo * 2.0 ** -k and float(r[t].max()) == hi * 2.0 ** -k
    assert bool(away.all())
    # zero points of every parity and both ends
    zps = {int(z) for z in zp.reshape(-1).tolist()}
    assert zps == {qmax // 2, qmax // 2 + 1, 0, qmax}


@pytest.mark.parametrize("C", [768, 1024, 1152, 1280, 4608])
@pytest.mark.parametrize("B", [1, 2])
def test_q2_quotients_sweep_both_sides_of_the_bound_and_the_guard(B, C):
    s = qr.q2_smooth(C)
    assert float(s[qr.Q2_S1_LO]) == 1.0 and float(s[qr.Q2_S1_HI]) == 1.0 and bool((s > 1).any()) and bool((s < 1).any())
    bits = s.view(torch.int32) & 0x7FFFFF
    assert bool((bits != 0x7FFFFF).all()) and bool(torch.isfinite(s).all())        # vq_smooth_reciprocal's precondition
    for n_bits in (8, 6):
        x = qr.q1(B, 48, C, n_bits, fixed=True)
        d = qr.row_deltas(x, n_bits, s)
        for t in range(48):
            assert float(d[t]) == 2.0 ** -qr.q1_row_spec(t, n_bits)[2]             # the grid stays 2^-k behind s
        dist = _rows(qr.tie_distance(x, n_bits, s))
        below = ((dist > 1e-6) & (dist < qr.BOUND)).sum(-1)
        mid = ((dist >= qr.BOUND) & (dist < qr.GUARD)).sum(-1)
        past = ((dist >= qr.GUARD) & (dist < 1e-3)).sum(-1)
        if n_bits == 8:
            assert int(below.min()) >= qr.Q2_BAND_MIN and int(mid.min()) >= qr.Q2_BAND_MIN and int(past.min()) >= qr.Q2_BAND_MIN
        else:           # |m + 0.5| <= 63.5: fewer elements reach the outer bands, every band is still met in every row
            assert int(below.min()) >= qr.Q2_BAND_MIN and int(mid.min()) >= 1 and int(past.min()) >= 1
        # both sides of the tie
        q = _rows(x.double() / s.double()) / d.double()[:, None]
        side = (q - torch.floor(q)) - 0.5
        near = dist < qr.GUARD
        assert bool(((side > 0) & near).any(-1).all()) and bool(((side < 0) & near).any(-1).all())


@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("B,C", [(1, 1152), (2, 1152), (3, 64), (1, 4608)])
def test_q3_zero_point_sits_on_a_tie(B, C, n_bits):
    mags = qr.q3_magnitudes(7 if (B, C) == (1, 1152) else 49)
    assert mags.numel() == (4535 if (B, C) == (1, 1152) else 648)
    x = qr.q3(B, C, mags)
    r = _rows(x)
    assert torch.equal(r.max(-1).values, mags) and torch.equal(r.min(-1).values, -mags)
    d = qr.row_deltas(x, n_bits).double()
    t = mags.double() / d
    assert float(((t - torch.floor(t)) - 0.5).abs().max()) < 1e-4
    assert float((torch.floor(t) - (2 ** n_bits - 1) // 2).abs().max()) == 0
    good, flagged = qr.split_eps(x, n_bits)
    assert good.numel() > 0.9 * mags.numel() and flagged.numel() > 0            # the sweep reaches delta < 1e-6


def test_q4_rows_straddle_the_eps_threshold():
    mags = qr.q4_magnitudes(8)
    assert mags.numel() == 143
    for B, C in SHAPES:
        x = qr.q4(B, C, 8)
        r = _rows(x)
        assert torch.equal(r.max(-1).values, mags) and float(r.min()) == 0.0
        good, flagged = qr.split_eps(x, 8)
        assert good.numel() == 63 and flagged.numel() == 80
        for i in flagged.tolist():
            assert fq.dyn_act_quant(x[:, i:i + 1].float(), 8)[4]
        assert not fq.dyn_act_quant(x[:, good].float(), 8)[4]
    # the two sides meet: the largest flagged and the smallest clean magnitude are fp16 neighbours
    d = qr.row_deltas(qr.q4(1, 64, 8), 8)
    assert float(d[d < qr.EPS].max()) < 1e-6 <= float(d[d >= qr.EPS].min())
    assert int(mags.view(torch.int16)[d >= qr.EPS].min()) - int(mags.view(torch.int16)[d < qr.EPS].max()) == 1
    good6, flagged6 = qr.split_eps(qr.q4(1, 64, 6), 6)
    assert good6.numel() > 10 and flagged6.numel() > 10


@pytest.mark.parametrize("B,C", SHAPES)
def test_q5_and_q6_rows_hold_what_they_name(B, C):
    x = qr.q5(B, C)
    assert bool(torch.isfinite(x).all())
    r = _rows(x)
    i = qr.Q5_ROWS.index
    assert float(r[i("both_65504")].max()) == 65504.0 and float(r[i("both_65504")].min()) == -65504.0
    assert float(r[i("both_65504_small_interior")].max()) == 65504.0 and float(r[i("both_65504_small_interior")].min()) == -65504.0
    assert float(r[i("pos_65504")].max()) == 65504.0 and float(r[i("pos_65504")].min()) == 0.0
    assert float(r[i("neg_65504")].min()) == -65504.0 and float(r[i("neg_65504")].max()) <= 0.0
    for name in ("subnormals", "subnormals_neg"):
        assert float(r[i(name)].abs().max()) < 2.0 ** -14 and float(r[i(name)].abs().min()) > 0
    assert float(r[i("normal_and_subnormals")].max()) == 1.0 and float(r[i("normal_and_subnormals")].abs().kthvalue(B * C - 1).values) < 2.0 ** -14
    assert float(r[i("neg_normal_and_subnormals")].min()) == -0.5
    mz = r[i("minus_zeros")]
    assert int(((mz == 0) & torch.signbit(mz)).sum()) >= B * C // 3
    mo = r[i("minus_zeros_and_one")]
    assert int(((mo == 0) & torch.signbit(mo)).sum()) == B * C - 1 and float(mo.max()) == 1.0
    for n_bits in (8, 6):
        _, flagged = qr.split_eps(x, n_bits)
        assert {qr.Q5_ROWS[j] for j in flagged.tolist()} == set(qr.Q5_FLAGGED[n_bits])
    # Q6: the planted extremum is unique and where the spec says
    y = qr.q6(B, C)
    specs = qr.q6_specs(B, C)
    assert y.shape[1] == len(specs) and {p for _, p, _, _ in specs} == {0, 7, C - 1, C // 2, C // 2 - 1, 8, C - 8}
    for t, (which, p, sb, so) in enumerate(specs):
        row = y[:, t].float()
        v = -qr.Q6_VALUE if which == "min" else qr.Q6_VALUE
        assert float(row[sb, p]) == v and int((row == v).sum()) == 1 and int((row == -v).sum()) == 1
        assert float(row.abs().max()) == qr.Q6_VALUE
        assert int((row[so] == -v).sum()) == 1                       # the other extremum is in the sample the spec names
    if B == 2:
        assert any(sb == 1 and so == 0 for _, _, sb, so in specs) and any(sb == so for _, _, sb, so in specs)


@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("B,C", SHAPES)
def test_no_bit_exact_launch_holds_an_eps_filled_row(B, C, n_bits):
    """launch_sets(): the exact launch is clean by the oracle itself (also behind the Q2 smoothing vector and a wide one),
    every family is in it, its length is odd, and every flagged launch is eps-filled because of exactly one row."""
    svecs = [None]
    if C >= 768:
        g = torch.Generator().manual_seed(C)
        svecs += [qr.q2_smooth(C), qr.q4u_vector(torch.exp(torch.randn(C, generator=g) * 0.7).float(), n_bits)]
    for s in svecs:
        exact, flagged, names = qr.launch_sets(B, C, n_bits, s=s, q3_stride=7 if (B, C) == (1, 1152) else 49,
                                               fixed=s is not None and s is svecs[1], ulp=s is not None and s is svecs[-1])
        assert exact.shape[1] % 2 == 1 and len(names) == exact.shape[1]
        assert set(names) - {"Q4u"} == {"Q1", "Q3", "Q4", "Q5", "Q6"}
        assert names.count("Q4u") == (2 if s is not None and s is svecs[-1] else 0)
        assert not fq.dyn_act_quant(qr.smoothed(exact, s), n_bits)[4]
        for n in (131, 257):
            assert not fq.dyn_act_quant(qr.smoothed(qr.thin(exact, n), s), n_bits)[4]
        assert len(flagged) >= (2 if s is svecs[-1] and s is not None else 6)     # (the wide vector lifts most small rows over 1e-6)
        for f in flagged:
            d = qr.row_deltas(f, n_bits, s)
            assert int((d < qr.EPS).sum()) == 1 and fq.dyn_act_quant(qr.smoothed(f, s), n_bits)[4]


@pytest.mark.parametrize("n_bits", [8, 6])
def test_q4u_rows_sit_on_the_eps_threshold_to_the_ulp(n_bits):
    e = torch.tensor(qr.EPS, dtype=torch.float32)
    below, above = torch.nextafter(e, torch.tensor(0.0)), torch.nextafter(e, torch.tensor(1.0))
    for B, C in ((1, 1152), (2, 4608)):
        s = qr.q4u_vector(torch.ones(C), n_bits)
        assert bool(((s.view(torch.int32) & 0x7FFFFF) != 0x7FFFFF).all())
        x = qr.q4u(B, C)
        d = qr.row_deltas(x, n_bits, s)
        assert d.tolist() == [float(below), float(e), float(above)]
        good, flagged = qr.split_eps(x, n_bits, s)
        assert good.tolist() == [1, 2] and flagged.tolist() == [0]
        assert fq.dyn_act_quant(qr.smoothed(x[:, :1], s), n_bits)[4] and not fq.dyn_act_quant(qr.smoothed(x[:, 1:], s), n_bits)[4]


def test_static_rows_reach_both_clamps():
    for n_bits in (8, 6):
        qmax = 2 ** n_bits - 1
        for per_token in (True, False):
            x, delta, zp = qr.static_rows(2, 37, 96, n_bits, per_token)
            assert delta.numel() == (37 if per_token else 1)
            d, z = delta.reshape(1, -1, 1), zp.reshape(1, -1, 1)
            raw = torch.round(x.float() / d) + z
            assert bool((raw < 0).any(-1).any(0).all()) and bool((raw > qmax).any(-1).any(0).all())
            codes, _ = fq.static_act_quant(x.float(), d, z, n_bits)
            assert float(codes.min()) == 0 and float(codes.max()) == qmax
            q = x.double() / d.double()
            assert int(((q - torch.floor(q)) == 0.5).sum()) > 30 * x.shape[1]       # still rows of exact ties


def test_one_hot_queries_pick_one_whole_value_row():
    import attn_regimes as ar
    for T, H, D in ((16, 8, 64), (5, 2, 32), (16, 16, 72), (17, 4, 16), (64, 8, 64)):
        q, k, hot = qr.one_hot_qk(6, T, H, D, D ** -0.5, seed=T + D)
        for s in range(6):
            assert sorted(hot[s].tolist()) == list(range(T))                      # every V row is some query's output
        gp = ar.gaps(q, k, hot[:, :, None].expand(6, T, H).contiguous(), D ** -0.5, [T] * 6)
        assert float((gp >= ar.R1_GAP).all(-1).double().mean()) >= 0.9


# ----------------------------------------------------------------------------- LayerNorm + modulate in front of the quantizer
def _ln_codes(x, shift, scale, n_bits, d_mean=None, d_rstd=None):
    """The oracle's LayerNorm + modulate + quantizer written out (fp32), with the row mean / rstd optionally moved by one
    fp32 ulp (d_mean, d_rstd: None, True = up, False = down)."""
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = ((xf - mean) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + 1e-6)
    if d_mean is not None:
        mean = qr.ulp_step(mean, d_mean)
    if d_rstd is not None:
        rstd = qr.ulp_step(rstd, d_rstd)
    xm = ((xf - mean) * rstd) * (1 + scale[:, None, :]) + shift[:, None, :]
    return fq.dyn_act_quant(xm, n_bits)


def ln_family_ok(name, B, C):
    """Does the oracle alone stay inside the LN route's bound (<= 1 code step on < 0.5 % of the elements) on this family
    when its LayerNorm statistics move by one fp32 ulp?"""
    x, shift, scale = qr.ln_inputs(name, B, C)
    base = _ln_codes(x, shift, scale, 8)
    assert not base[4]
    for dm in (None, True, False):
        for dr in (None, True, False):
            c = _ln_codes(x, shift, scale, 8, dm, dr)[0]
            diff = (c - base[0]).abs()
            if float(diff.max()) > 1 or float((diff > 0).float().mean()) >= 5e-3:
                return False
    return True


@pytest.mark.parametrize("B,C", [(1, 64), (1, 1152), (2, 1152)])
def test_ln_route_families_are_stable_under_one_ulp_of_the_statistics(B, C):
    """The families test_quantizer_edges_gpu.py runs through vq_ln_modulate_rowquant (qr.LN_FAMILIES) stay inside the 0.5 %
    bound in the oracle itself; a family that does not is not in that list (none had to be dropped)."""
    for name in qr.LN_FAMILIES:
        assert ln_family_ok(name, B, C), name

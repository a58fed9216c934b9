"""ln_cases.py on the CPU: (1) every member of the model set - every fp32 evaluation of LayerNorm + modulate a correct
kernel may be - passes check_launch / check_static against the fp64 reference, inside the caps, on every family, width and
code width: a correct kernel cannot fail test_ln_modulate_exact_gpu.py; (2) Python mutants of the model - the ways such a
kernel goes wrong - are each rejected on a named family.  The measured E values and shares are printed (pytest -s) and
kept in profiles/ln_exact/README.md."""
import pytest
import torch

import ln_cases as lc
import quant_rows as qr
from oracle import fakequant as fq

WIDTHS = (64, 768, 1152, 1408, 4608)
ROWS = 9


def _cases():
    for C in WIDTHS:
        for B in ((1, 2) if C in (768, 1152) else (1,)):
            for fam in lc.FAMILIES:
                for eps in ((1e-6, 1e-5) if fam == "L3" else (1e-6,)):
                    yield pytest.param(fam, B, C, eps, id="%s-B%d-C%d-eps%g" % (fam, B, C, eps))


@pytest.mark.parametrize("fam,B,C,eps", list(_cases()))
def test_every_model_passes_the_checker_inside_the_caps(fam, B, C, eps):
    x, shift, scale = lc.family(fam, B, ROWS, C)
    s = lc.smooth_vectors(C, 1)[0]
    base = lc.Reference(x, shift, scale, eps, 8, [None, s], names=[fam] * ROWS)
    for n_bits in (8, 6, 4):
        ref = base.rebits(n_bits)
        f = ref.figures()
        print("%s B%d C%d eps %g b%d: E_u %.2e xm share %.4f / %.4f | plain E_t %.2e E_z %.2e E_d %.1e share %.4f | "
              "smoothed E_t %.2e E_z %.2e E_d %.1e share %.4f" % (
                  fam, B, C, eps, n_bits, f["E_u"], f["xm_share"], f["xm_share_ill"],
                  f["out0"]["E_t"], f["out0"]["E_z"], f["out0"]["E_delta_rel"], f["out0"]["code_share"],
                  f["out1"]["E_t"], f["out1"]["E_z"], f["out1"]["E_delta_rel"], f["out1"]["code_share"]))
        assert ref.finite_and_small(), f
        ds, zs = lc.static_grids(ref, per_token=n_bits != 6, n_out=2)
        for name, u in zip(ref.model_names, ref.model_u):
            for j, sj in enumerate(ref.smooth):
                lc.check_launch(ref, j, lc.launch_of(u, sj, n_bits, C), "%s out%d b%d" % (name, j, n_bits))
            for j, got in enumerate(lc.static_launch_of(u, ref.smooth, ds, zs, n_bits, C)):
                lc.check_static(ref, j, got, ds[j], zs[j], "%s static out%d b%d" % (name, j, n_bits))
                got["xm"] = None
                lc.check_static(ref, j, got, ds[j], zs[j], "%s static out%d b%d" % (name, j, n_bits))


def _gpu_shapes():
    import test_ln_modulate_exact_gpu as g               # (imports no GPU code: its cases are plain data)
    return sorted({(c[1], c[2]) for c in g.LNQ + g.SHARED + g.STATIC}), g.ROWS_EPS


@pytest.mark.parametrize("B,C", _gpu_shapes()[0])
def test_the_mixed_launches_of_the_gpu_test_stay_inside_the_caps(B, C):
    """The launches test_ln_modulate_exact_gpu.py makes (ln_cases.mixed at every shape and row count of its case lists, with
    their eps): the oracle member passes with status 0 (no eps fill), and the shares are inside the caps at every code
    width, plain and behind each smoothing vector."""
    for n, eps in _gpu_shapes()[1]:
        x, shift, scale, names = lc.mixed(B, n, C)
        sv = lc.smooth_vectors(C, 3)
        base = lc.Reference(x, shift, scale, eps, 8, [None] + sv, names=names)
        for n_bits in (8, 6, 4):
            ref = base.rebits(n_bits)
            assert ref.finite_and_small(), ref.figures()
            cap = lc._cap(x.numel())
            assert ref.xm_share() <= cap and ref.xm_share(True) <= lc.XM_ILL_CAP
            for j, sj in enumerate(ref.smooth):
                assert ref.code_share(j) <= cap
                got = lc.launch_of(ref.model_u[0], sj, n_bits, C)
                assert got["status"] == 0
                lc.check_launch(ref, j, got, "oracle mixed n%d out%d b%d" % (n, j, n_bits))


# ----------------------------------------------------------------------------- mutants
def _ln32(x, shift, scale, eps, unbiased=False, one_pass=False, shared_mod=False):
    xf = x.float()
    C = xf.shape[-1]
    mu = xf.mean(-1, keepdim=True)
    if one_pass:
        var = (xf * xf).mean(-1, keepdim=True) - mu * mu
    else:
        var = ((xf - mu) ** 2).sum(-1, keepdim=True) / (C - 1 if unbiased else C)
    y = (xf - mu) * (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32)))
    if shared_mod:
        shift, scale = shift[:1].expand_as(shift), scale[:1].expand_as(scale)
    return y * (1.0 + scale[:, None, :]) + shift[:, None, :]


def _toward_zero(u):
    h = u.half()
    over = h.float().abs() > u.abs()
    return torch.where(over, torch.nextafter(h, torch.zeros_like(h)), h)


def _m_short_R(got, ref):
    got["R"] = got["R"] - got["xq"][:, :8].int().sum(-1)                  # lane 0's first chunk never summed


def _m_channel(got, ref):
    got["xq"][:, 5] += 1                                                   # (int8: L1 rows hold no code at 127 in channel 5)
    got["R"] = (got["xq"].int().sum(-1) - ref.C * got["zx"]).int()


def _m_last_zx(got, ref):
    got["zx"][-1] += 1
    got["R"] = (got["xq"].int().sum(-1) - ref.C * got["zx"]).int()       # R follows: only the zero point is wrong


# name: (family the mutant is rejected on, B, C, eps passed, u of the mutant or None, edit of the outputs or None, xm edit)
MUTANTS = {
    "eps_dropped": ("L3", 1, 1152, 1e-6, lambda x, sh, sc, e: _ln32(x, sh, sc, 0.0), None),
    "eps_hard_coded_1e-5": ("L3", 1, 1152, 1e-6, lambda x, sh, sc, e: _ln32(x, sh, sc, 1e-5), None),
    "eps_hard_coded_1e-6": ("L3", 1, 1152, 1e-5, lambda x, sh, sc, e: _ln32(x, sh, sc, 1e-6), None),
    "variance_over_C_minus_1": ("L1", 1, 64, 1e-6, lambda x, sh, sc, e: _ln32(x, sh, sc, e, unbiased=True), None),
    "one_pass_variance": ("L2", 1, 1152, 1e-6, lambda x, sh, sc, e: _ln32(x, sh, sc, e, one_pass=True), None),
    "sample_0_modulation_for_every_row": ("L1", 2, 1152, 1e-6, lambda x, sh, sc, e: _ln32(x, sh, sc, e, shared_mod=True), None),
    "xm_rounded_toward_zero": ("L1", 1, 1152, 1e-6, None, "xm"),
    "R_short_of_one_chunk": ("L1", 1, 1152, 1e-6, None, _m_short_R),
    "one_channel_off_by_one": ("L1", 1, 1152, 1e-6, None, _m_channel),
    "last_row_zx_off_by_one": ("L1", 2, 1152, 1e-6, None, _m_last_zx),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutants_are_rejected(name):
    fam, B, C, eps, wrong_u, edit = MUTANTS[name]
    x, shift, scale = lc.family(fam, B, ROWS, C)
    ref = lc.Reference(x, shift, scale, eps, 8, [None], names=[fam] * ROWS)
    good = _ln32(x, shift, scale, eps)
    lc.check_launch(ref, 0, lc.launch_of(good, None, 8, C), "unmutated")          # the same code, unmutated, passes
    got = lc.launch_of(good if wrong_u is None else wrong_u(x, shift, scale, eps), None, 8, C)
    if edit == "xm":
        got["xm"] = _toward_zero(good)
    elif edit is not None:
        edit(got, ref)
    with pytest.raises(AssertionError) as e:
        lc.check_launch(ref, 0, got, name)
    print(name, "rejected on", fam, ":", str(e.value)[:160])
    if name == "last_row_zx_off_by_one":
        assert " zx:" in str(e.value)
    if name == "R_short_of_one_chunk":
        assert " R:" in str(e.value)
    if name == "xm_rounded_toward_zero":
        assert " xm:" in str(e.value)


def test_the_models_grid_is_the_oracles():
    """_grid() is token_params before the rounding of the zero point; static_grids() are integer-valued zero points."""
    x, shift, scale, names = lc.mixed(2, 9, 768)
    ref = lc.Reference(x, shift, scale, 1e-6, 8, [None], names=names)
    u = ref.model_u[0]
    d, z = lc._grid(u, 8)
    delta, zp, fill = fq.token_params(u, 8)
    assert not fill and torch.equal(d, delta.reshape(-1)) and torch.equal(torch.round(z), zp.reshape(-1))
    for per_token in (True, False):
        ds, zs = lc.static_grids(ref, per_token, 3)
        assert all(t.numel() == (9 if per_token else 1) for t in ds + zs)
        assert all(torch.equal(t, torch.round(t)) for t in zs)
    assert names[:7] == list(lc.FAMILIES) and set(qr.LN_FAMILIES) <= set(lc.FAMILIES)

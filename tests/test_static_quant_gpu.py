"""vq_rowquant_static: the one-pass quantizers of static (calibrated) grids, against the CPU oracle
(oracle/fakequant.py: static_act_quant) bit for bit - codes, zeroed pad columns, sx, zx and R - through every lane map
of csrc/rowquant_static.hip:

  C = 1152   a half-wave per row (plain, added rows; LayerNorm at B = 2), a wave per row (LayerNorm at B = 1, 3)
  C = 4608   a row over two partner waves (plain), a wave per row (added rows, LayerNorm)
  C = 200, 64, and 1152 with Kp = 1408: a wave per row with 1 or 3 chunks, pad columns beyond the row

Rows are quant_rows.static_rows: exact ties on 2^-k grids, both clamps, values 300 steps outside and +-65504 - the
inputs the product form of round(x / delta) must survive on a grid the row did not define.  Then the routes that use
the entry point: vq_rowquant's static dispatch, and the fused block of the tiny static STDiT / PixArt plans with the
route switch on and off (equal outputs, and the launches a block makes)."""
import pytest
import torch

import quant_rows as qr
from test_quantizer_edges_gpu import _check_exact, _first_diff

pytestmark = pytest.mark.gpu


def _grids(delta, zp, n_out):
    """A distinct grid per output from the rows' own: the step doubled / halved, the zero point moved (still an integer),
    so each output clamps other values."""
    return [delta, delta * 2.0, delta * 0.5][:n_out], [zp, zp + 1.0, zp - 3.0][:n_out]


def _smooth(C, mix, n_out):
    """-> (smoothing vector or None per output, fast_div).  none | rcp: every output smoothed, reciprocal form |
    div: output 0 smoothed, IEEE division (no reciprocal passed)."""
    if mix == "none":
        return [None] * n_out, True
    g = torch.Generator().manual_seed(C + n_out)
    vec = [(0.5 + 1.5 * torch.rand(C, generator=g)).float() for _ in range(n_out)]
    if mix == "rcp":
        return vec, True
    return [vec[0]] + [None] * (n_out - 1), False


CASES = [(C, None, n, B) for C in (1152, 4608, 200, 64) for n in (131, 257) for B in (1, 2)] + [(1152, 1408, 131, 1)]


@pytest.mark.parametrize("n_bits", [8, 6, 4])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add_rows"])
@pytest.mark.parametrize("C,Kp,n_tok,B", CASES)
def test_plain_and_added_rows_on_static_grids(ops, dev, C, Kp, n_tok, B, add, n_bits):
    T = 4
    add_div = -(-n_tok // T)
    for per_token in (True, False):
        x, delta, zp = qr.static_rows(B, n_tok, C, n_bits, per_token)
        xin = x
        addr = None
        if add:                                   # the oracle is fed the fp16 inputs added in fp32
            g = torch.Generator().manual_seed(7 * C + n_tok)
            addr = (torch.randn(T, C, generator=g) * 2.0 ** -3).half()
            xin = x.float() + addr.float()[torch.arange(n_tok) // add_div][None]
        xd, ad = x.to(dev), None if addr is None else addr.to(dev)
        for n_out in (1, 2, 3):
            ds, zs = _grids(delta, zp, n_out)
            for mix in ("none", "rcp", "div"):
                vec, fast = _smooth(C, mix, n_out)
                dvec = [None if v is None else v.to(dev) for v in vec]
                if mix == "rcp":
                    assert all(ops.smooth_rcp(v) is not None for v in dvec)
                outs = ops.rowquant_static(xd, [d.to(dev) for d in ds], [z.to(dev) for z in zs], n_bits=n_bits,
                                           smooth=dvec, add_rows=ad, add_div=add_div, fast_div=fast, Kp=Kp)
                assert len(outs) == n_out
                for j, qa in enumerate(outs):
                    assert qa.xq.shape == (B * n_tok, Kp or ops.pad128(C))
                    dd = ds[j] if per_token else ds[j].expand(n_tok)
                    zz = zs[j] if per_token else zs[j].expand(n_tok)
                    what = "C%d Kp%s n%d B%d b%d pt%d add%d %s out%d/%d" % (C, Kp, n_tok, B, n_bits, per_token, add, mix,
                                                                           j, n_out)
                    _check_exact(qa, None, xin, n_bits, vec[j], what, delta=dd, zp=zz)


def _ln_rows(B, n_tok, C, seed):
    g = torch.Generator().manual_seed(seed)
    row_scale = 0.1 * 300.0 ** torch.rand(B, n_tok, 1, generator=g)          # 0.1 .. 30
    offset = torch.randn(B, n_tok, 1, generator=g) * row_scale
    x = (torch.randn(B, n_tok, C, generator=g) * row_scale + offset).half()
    shift = (torch.randn(B, C, generator=g) * 0.3).float()
    scale = (torch.randn(B, C, generator=g) * 0.3).float()
    return x, shift, scale


# B = 1 / B = 2 at a block width are the launches a static plan makes today (a wave / a half-wave per row); C = 64 and
# B = 3 take the generic kernel's order, C = 4608 the 9-chunk form
@pytest.mark.parametrize("C,B", [(1152, 1), (1152, 2), (64, 1), (64, 2), (1152, 3), (4608, 1)])
def test_layernorm_arm_quantizes_the_activation_stored_today(ops, dev, C, B):
    n_tok, n_bits = 131, 8
    qmax = 2 ** n_bits - 1
    x, shift, scale = _ln_rows(B, n_tok, C, seed=C + B)
    xd, shd, scd = x.to(dev), shift.to(dev), scale.to(dev)
    _, xm_ref = ops.ln_modulate_rowquant(xd, shd, scd, 1e-6, smooth=[None], n_bits=8, want_xm=True)
    xm = xm_ref.cpu()
    lo, hi = float(xm.float().min()), float(xm.float().max())
    ds = [torch.tensor([f * (hi - lo) / qmax], dtype=torch.float32) for f in (0.8, 1.0, 1.3)]
    zs = [torch.round(-lo / d) for d in ds]
    vec, _ = _smooth(C, "rcp", 3)
    for smooth in ([None] * 3, [None, vec[1], vec[2]]):
        dvec = [None if v is None else v.to(dev) for v in smooth]
        outs, got_xm = ops.rowquant_static(xd, [d.to(dev) for d in ds], [z.to(dev) for z in zs], n_bits=n_bits, smooth=dvec,
                                           shift=shd, scale=scd, eps=1e-6, want_xm=True)
        assert torch.equal(got_xm.view(torch.int16), xm_ref.view(torch.int16)), _first_diff(
            got_xm.cpu().float(), xm.float(), "C%d B%d xm" % (C, B))
        for j, qa in enumerate(outs):
            _check_exact(qa, None, xm, n_bits, smooth[j], "LN C%d B%d out%d" % (C, B, j), delta=ds[j].expand(n_tok),
                         zp=zs[j].expand(n_tok))
    # both clamps act on the outputs whose grid is narrower than the activation's range
    codes = outs[0].xq[:, :C].int() + 128
    assert bool((codes == 0).any()) and bool((codes == qmax).any())


@pytest.mark.parametrize("C", [1152, 4608])
@pytest.mark.parametrize("per_token", [True, False])
def test_rowquant_with_a_static_grid_runs_the_one_pass_kernel(ops, dev, C, per_token):
    n_tok = 131
    x, delta, zp = qr.static_rows(1, n_tok, C, 8, per_token)
    qa = ops.rowquant(x.to(dev), n_bits=8, delta=delta.to(dev), zp=zp.to(dev))
    dd, zz = (delta, zp) if per_token else (delta.expand(n_tok), zp.expand(n_tok))
    _check_exact(qa, None, x, 8, None, "rowquant static C%d" % C, delta=dd, zp=zz)
    one = ops.rowquant_static(x.to(dev), [delta.to(dev)], [zp.to(dev)], n_bits=8)[0]
    for f in ("xq", "sx", "zx", "R"):
        assert torch.equal(getattr(qa, f), getattr(one, f)), f


# ----------------------------------------------------------------------------- the block's route
def _tiny_static_stdit(dev):
    from helpers import load_npz, quant_params_of
    from test_parity_gpu import _cfgs, _load_qp, _stdit
    g = load_npz("tiny_stdit_static.npz")
    wq, aq = _cfgs(8, dynamic=False, per_group=False, mixed_precision=[4, 6, 8])
    qnn = _stdit(g, dev, wq, aq, cfg_split=False)
    _load_qp(qnn, quant_params_of(g, "qp_tw"))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    x, y, mask = g["x"].to(dev), g["y"].half().to(dev), g["mask"].to(dev)
    return qnn, (torch.cat([x, x]), torch.tensor([721, 721], device=dev), y), dict(mask=mask)


def _tiny_naive_pixart(dev):
    from helpers import load_npz, quant_params_of
    from test_parity_gpu import _cfgs, _load_qp, _pixart
    g = load_npz("tiny_pixart_alpha.npz")
    wq, aq = _cfgs(8, dynamic=False, per_group=False, T=1, S=64)
    qn = _pixart("PixArt", g, dev, wq, aq)
    _load_qp(qn, quant_params_of(g, "qp_naive"))
    assert all(b.fused_ok() for b in qn.model.blocks)
    return qn, (g["x"].to(dev), g["t"].to(dev), g["y"].half().to(dev)), dict(mask=g["mask"].to(dev))


@pytest.mark.parametrize("build", [_tiny_static_stdit, _tiny_naive_pixart], ids=["stdit_static_tw", "pixart_alpha_naive"])
def test_the_one_pass_route_equals_the_layerwise_quantizers_on_a_model(ops, dev, monkeypatch, build):
    from viditq_amd.t2v import stdit
    qnn, args, kw = build(dev)
    calls = []
    real = ops.rowquant_static
    monkeypatch.setattr(ops, "rowquant_static", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert stdit._STATIC_FUSED is True
    new = qnn(*args, **kw)
    assert calls, "the static plan did not take the one-pass quantizers"
    n = len(calls)
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    old = qnn(*args, **kw)
    assert len(calls) == n
    assert torch.isfinite(new).all()
    assert torch.equal(new, old), "%d of %d values differ" % (int((new != old).sum()), new.numel())


@pytest.mark.parametrize("fused,want", [(True, dict(rowquant_static=3, rowquant=5, ln_modulate_rowquant=0)),
                                        (False, dict(rowquant_static=0, rowquant=12, ln_modulate_rowquant=2))],
                         ids=["one_pass", "layerwise"])
def test_quantizer_launches_of_one_fused_block(ops, dev, monkeypatch, fused, want):
    """Per STDiTBlock.forward_fused of the static tensor-wise plan (the prompt's K / V are handed in, as the model does when
    it batches them): three one-pass launches (LN + q|k|v, temporal q|k|v with the position embedding, LN + fc1) and the
    five single quantizers of proj, proj, q_linear, proj and fc2 - against 12 generic passes behind 2 LayerNorm launches."""
    from viditq_amd.t2v import stdit
    qnn, args, kw = _tiny_static_stdit(dev)
    monkeypatch.setattr(stdit, "_STATIC_FUSED", fused)
    count = dict.fromkeys(want, 0)
    for name in want:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            count[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    per_block = []
    inner = stdit.STDiTBlock.forward_fused

    def forward_fused(self, x2, y2, t0, y_lens, tpe, B, kv_ready=None, mod=None):
        if kv_ready is None:
            kv_ready = self.prompt_kv(y2)
        before = dict(count)
        out = inner(self, x2, y2, t0, y_lens, tpe, B, kv_ready=kv_ready, mod=mod)
        per_block.append({k: count[k] - before[k] for k in count})
        return out
    monkeypatch.setattr(stdit.STDiTBlock, "forward_fused", forward_fused)
    qnn(*args, **kw)
    assert len(per_block) == len(qnn.model.blocks) == 2
    for got in per_block:
        assert got == want

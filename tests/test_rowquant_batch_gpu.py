"""vq_rowquant_batch on the GPU: the one-pass per-token quantizers of a batched forward (3 <= B <= 16 rows of a token share one
grid).  Plain / smoothed arm against the CPU oracle bit for bit (quant_rows.py), GELU arm under gelu_cases.check, LayerNorm
arm under ln_cases.check_launch, every arm against the launches it replaces, guard rows, and one STDiT block behind
stdit._BATCH_QUANT against the oracle block."""
import functools

import pytest
import torch

import gelu_cases as gc
import ln_cases as lc
import quant_rows as qr
from test_quantizer_edges_gpu import _check_exact
from test_rowquant_batch_cpu import LN_SHAPES, ln_reference

pytestmark = pytest.mark.gpu
FIELDS = ("xq", "sx", "zx", "R")
launch_sets = functools.lru_cache(maxsize=None)(lambda B, C, n_bits, smoothed: qr.launch_sets(
    B, C, n_bits, s=qr.q2_smooth(C) if smoothed else None, q3_stride=49, fixed=True))


def _vectors(C, kind):
    """The smoothing vectors of one launch and whether each has a reciprocal form (an all-ones significand has none)."""
    wide = [torch.exp(torch.randn(C, generator=torch.Generator().manual_seed(3 + j)) * 0.7).float() for j in range(2)]
    if kind == "none":
        return [None], [False]
    if kind == "exact_div":
        s = qr.q2_smooth(C).clone()
        s[5] = 1.0 - 2.0 ** -24
        return [s], [False]
    return ([qr.q2_smooth(C)], [True]) if kind == "rcp" else ([qr.q2_smooth(C)] + wide, [True] * 3)


def _got(qa, st, xm=None):
    return dict({f: getattr(qa, f).cpu() for f in FIELDS}, status=int(st.item()), xm=None if xm is None else xm.cpu())


@pytest.mark.parametrize("kind", ["none", "rcp", "exact_div", "three"])
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("B,C", [(3, 96), (3, 1152), (5, 1408), (8, 1152), (9, 768), (16, 1152), (4, 4608), (16, 4608)])
def test_plain_and_smoothed_arm_against_the_oracle(ops, dev, B, C, n_bits, kind):
    """Exact ties, near ties, symmetric rows, the eps threshold, fp16 extremes and planted extrema: codes, step, zero point
    and R bit for bit with status 0 on 131, 65 and 3 rows (3 leaves dead token groups), status 1 on the flagged launches."""
    vec, has_rcp = _vectors(C, kind)
    dvec = [None if v is None else v.to(dev) for v in vec]
    assert [v is not None and ops.smooth_rcp(v) is not None for v in dvec] == has_rcp
    exact, flagged, _ = launch_sets(B, C, n_bits, kind != "none")
    for v in vec:                                            # rows the oracle eps-fills behind one of the vectors are left out
        exact = exact[:, qr.split_eps(exact, n_bits, v)[0]]
    for n in (131, 65, 3):
        x, st = qr.thin(exact, n), ops.new_status(dev)
        for qa, v in zip(ops.rowquant_batch(x.to(dev), n_bits, dvec, status=st), vec):
            _check_exact(qa, st, x, n_bits, v, "B%d C%d b%d %s n%d" % (B, C, n_bits, kind, n))
    for x in flagged[:2] if kind != "exact_div" else []:     # (flagged behind no vector / the Q2 vector, which comes first)
        st = ops.new_status(dev)
        ops.rowquant_batch(x.to(dev), n_bits, dvec, status=st)
        assert int(st.item()) == 1


@pytest.mark.parametrize("s", [None, 0.75])
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("B", [3, 16])
@pytest.mark.parametrize("C", [4608, 1152])
def test_gelu_arm_over_every_fp16_input(ops, dev, C, B, n_bits, s):
    """gelu_cases' pair rows tiled to B samples (x[b] = pair[b % 2]) keep every token's grid: sample b's outputs are held to
    the pair's expectation of sample b % 2: samples 0 and 1 through gelu_cases.check, every later one equal to them."""
    pair = gc.rows(n_bits, 2, C)
    n = pair.shape[1]
    st = ops.new_status(dev)
    qa = ops.gelu_rowquant_batch(pair.to(dev)[torch.arange(B, device=dev) % 2].contiguous(), n_bits,
                                 None if s is None else torch.full((C,), s, device=dev), status=st)
    got = {f: getattr(qa, f).view(B, n, -1) for f in FIELDS}
    for f in FIELDS:
        assert torch.equal(got[f], got[f][:2].repeat((B + 1) // 2, 1, 1)[:B]), f
    first = dict({f: got[f][:2].reshape(2 * n, -1).squeeze(-1).cpu() for f in FIELDS}, status=int(st.item()))
    gc.check(gc.expected(pair, n_bits, s), first, "gelu B%d C%d b%d s%s" % (B, C, n_bits, s))


@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("n_bits", [8, 4])
@pytest.mark.parametrize("B,C", LN_SHAPES)
def test_ln_arm_under_the_margin_exact_rule(ops, dev, B, C, n_bits, n_out):
    for n, eps in ((9, 1e-6), (1, 1e-6)) + (((9, 1e-5),) if (B, C) == (8, 1152) else ()):
        x, shift, scale, smooth, ref8 = ln_reference(B, n, C, eps)
        ref = ref8.rebits(n_bits, smooth[:n_out])
        st = ops.new_status(dev)
        outs, xm = ops.ln_modulate_rowquant_batch(x.to(dev), shift.to(dev), scale.to(dev), eps, [None if v is None else v.to(dev)
                                                  for v in smooth[:n_out]], n_bits, status=st, want_xm=True)
        for j, qa in enumerate(outs):
            lc.check_launch(ref, j, _got(qa, st, xm if j == 0 else None), "ln B%d C%d n%d b%d out%d eps%g" % (B, C, n, n_bits, j, eps))


@pytest.mark.parametrize("B", [4, 8])
def test_equals_the_launches_it_replaces(ops, dev, B):
    """Gaussian rows: every field of ops.rowquant(B) per output, plain and smoothed, C = 1152 and 4608."""
    for C in (1152, 4608):
        x = (torch.randn(B, 37, C, generator=torch.Generator().manual_seed(B + C)) * 1.5).half().to(dev)
        sv = [None] + [v.to(dev) for v in _vectors(C, "three")[0][1:]]
        for qa, s in zip(ops.rowquant_batch(x, 6, sv), sv):
            ref = ops.rowquant(x, n_bits=6, s=s)
            assert all(torch.equal(getattr(qa, f), getattr(ref, f)) for f in FIELDS), (C, s is None)


@pytest.mark.parametrize("B", [4, 8])
def test_gelu_arm_grid_equals_the_epilogue_route(ops, dev, B):
    """The GELU arm's grid fields against fc1's GELU-epilogue activation followed by ops.rowquant, on Gaussian rows, without
    and with a constant smoothing value.  The two routes are not one function: the epilogue applies GELU to the fp32
    accumulator and rounds once, the one-pass quantizers (this arm, vq_gelu_rowquant at B <= 2, the reference) to the fp16
    fc1 output.  A token's GRID is the same all the same where its extremes do not feel that order, which these rows ensure
    and the test asserts first: a maximum of 6 or more (there 2^w < 2^-24, the sigmoid rounds to 1 and GELU is the identity in
    both routes) and, among a token's B * 4608 values, inputs next to GELU's flat minimum -0.169971, which lies 4.9e-5 from
    the fp16 value -0.16992 and 1.2e-5 from the rounding boundary below it - every value within 1.1e-4 of the minimum rounds to
    -0.16992 in either route.  A constant smoothing value keeps both extremes where they are.  Behind a PER-CHANNEL vector
    the extreme of g / s may sit on any g, and there the routes do differ: that figure is printed, not asserted (measured:
    the step of 2 of 37 tokens at B = 4 and 3 of 37 at B = 8, one fp16 ulp of the extreme apart)."""
    W = (torch.randn(4608, 1152, generator=torch.Generator().manual_seed(1)) * 0.05).half().to(dev)
    pw = ops.pack_weight(W, *ops.weight_minmax(W, 8), 8)
    x = (torch.randn(B, 37, 1152, generator=torch.Generator().manual_seed(B)) * 1.5).half().to(dev)
    h, hg = [ops.gemm_i8(ops.rowquant(x.view(1, -1, 1152)), pw, epilogue=e).view(B, 37, -1) for e in (ops.EPI_NONE, ops.EPI_GELU)]
    tok = h.float().permute(1, 0, 2).reshape(37, -1)
    assert float(tok.max(-1).values.min()) >= 6.0 and int(((tok + 0.7518).abs() < 0.01).sum(-1).min()) >= 8
    for s in (None, torch.full((4608,), 0.75, device=dev)):
        qa, ref = ops.gelu_rowquant_batch(h, 8, s), ops.rowquant(hg, n_bits=8, s=s)
        assert torch.equal(qa.sx, ref.sx) and torch.equal(qa.zx, ref.zx), s is None
    s2 = _vectors(4608, "three")[0][1].to(dev)
    qa, ref = ops.gelu_rowquant_batch(h, 8, s2), ops.rowquant(hg, n_bits=8, s=s2)
    print("B %d, per-channel vector: %d of %d rows differ in sx, %d in zx" % (
        B, int((qa.sx != ref.sx).sum()), qa.sx.numel(), int((qa.zx != ref.zx).sum())))


@pytest.mark.parametrize("arm", ["plain", "gelu", "ln"])
@pytest.mark.parametrize("B", [3, 16])
def test_writes_only_its_rows(ops, dev, B, arm):
    """Sentinel rows around every output and xm, n_tok = 7 (no multiple of the 5 token groups of B = 3): only rows [0, B n_tok)
    change, and they are the wrapper's."""
    import ctypes
    from viditq_amd import _lib
    n_tok, C, pad, n_out = 7, 1152, 4, 1 if arm == "gelu" else 3
    rows = B * n_tok
    x = (torch.randn(B, n_tok, C, generator=torch.Generator().manual_seed(B)) * 1.5).half().to(dev)
    sv = [v.to(dev) for v in _vectors(C, "three")[0][:n_out]]
    mod = [(torch.randn(B, C, generator=torch.Generator().manual_seed(7 + k)) * 0.3).to(dev) for k in range(2)] if arm == "ln" else [None, None]
    fill = {"xq": ((rows + 2 * pad, C), torch.int8, 0x5A), "sx": ((rows + 2 * pad,), torch.float32, -7.0),
            "zx": ((rows + 2 * pad,), torch.int32, -77), "R": ((rows + 2 * pad,), torch.int32, -777)}
    bufs = [{f: torch.full(sh, val, dtype=dt, device=dev) for f, (sh, dt, val) in fill.items()} for _ in range(n_out)]
    xm = torch.full((rows + 2 * pad, C), 3.0, dtype=torch.float16, device=dev) if arm == "ln" else None
    arr = lambda vals: ctypes.cast((ctypes.c_void_p * 3)(*(list(vals) + [None] * (3 - n_out))), ctypes.c_void_p)  # noqa: E731
    keep = [arr(s.data_ptr() for s in sv), arr(ops.smooth_rcp(s).data_ptr() for s in sv)] + [arr(b[f][pad:].data_ptr() for b in bufs) for f in FIELDS]
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    assert _lib.load().vq_rowquant_batch(p(x), p(mod[0]), p(mod[1]), 1e-6, int(arm == "gelu"), n_out, *keep, None if xm is None else
                                         xm[pad:].data_ptr(), B, n_tok, C, C, 8, None, torch.cuda.current_stream().cuda_stream) == 0
    if arm == "ln":
        ref, ref_xm = ops.ln_modulate_rowquant_batch(x, mod[0], mod[1], 1e-6, sv, 8, want_xm=True)
        assert bool((xm[:pad] == 3.0).all()) and bool((xm[pad + rows:] == 3.0).all()) and torch.equal(xm[pad:pad + rows], ref_xm.view(rows, C))
    else:
        ref = [ops.gelu_rowquant_batch(x, 8, sv[0])] if arm == "gelu" else ops.rowquant_batch(x, 8, sv)
    for b, r in zip(bufs, ref):
        for f, (_, _, val) in fill.items():
            assert bool((b[f][:pad] == val).all()) and bool((b[f][pad + rows:] == val).all()), f
            assert torch.equal(b[f][pad:pad + rows], getattr(r, f)), f


def test_one_block_behind_the_switch(ops, dev, monkeypatch):
    """A depth-1 STDiT block (C = 1152, 16 heads, d_t = 2, d_s = 8, a smoothing vector on every Linear, dynamic 8-bit grids).
    B = 4: off, today's calls; on, the eight batched launches in their place; both within the per-block 1e-3 rel-L2 of the
    oracle block.  B = 16: the off route raises (LayerNorm quantizer, B > 8), the on route holds the same bound."""
    from viditq_amd import synth
    from viditq_amd.config import loads_yaml
    from viditq_amd.t2v import stdit
    from oracle import stdit_ref as sr
    T, S, H, C, L = 2, 8, 16, 1152, 12
    names = ["rowquant", "ln_modulate_rowquant", "gelu_rowquant", "rowquant_batch", "ln_modulate_rowquant_batch", "gelu_rowquant_batch"]
    count = dict.fromkeys(names, 0)
    for name in names:
        def counted(*a, _real=getattr(ops, name), _name=name, **k):
            count[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    cfg = loads_yaml(synth.W4A8_TIMESTEP_AWARE.replace("cfg_split: True", "cfg_split: False").replace("quantizer: {n_bits: 4,", "quantizer: {n_bits: 8,"))
    m = synth.build_stdit(dev, depth=1, input_size=(T, 4, 8), model_max_length=L, caption_channels=64, seed=5)
    qnn = synth.quantize_model(m, cfg)
    blk = qnn.model.blocks[0]
    g = torch.Generator().manual_seed(6)
    seen, inner = [], stdit.STDiTBlock.forward_fused
    monkeypatch.setattr(stdit.STDiTBlock, "forward_fused", lambda self, x2, y2, t0, off, tpe, B, kv_ready=None, mod=None: (
        seen.append((x2.clone(), y2.clone(), t0.clone())), inner(self, x2, y2, t0, off, tpe, B, kv_ready=kv_ready, mod=mod))[1])
    with torch.no_grad():                                    # one joint forward sets the step and hands over a block's inputs
        qnn(torch.randn(4, 4, T, 4, 8, generator=g).to(dev), torch.full((4,), 721, device=dev),
            (torch.randn(4, 1, L, 64, generator=g) * 0.3).half().to(dev), mask=torch.ones(4, L, dtype=torch.int64, device=dev), timestep_id=721)
    monkeypatch.setattr(stdit.STDiTBlock, "forward_fused", inner)
    x4, y4, t4 = seen[0]
    act_scale = {"blocks.0." + n: l.act_quantizer.act_scale.detach().cpu().float() for n, l in blk.named_modules()
                 if getattr(getattr(l, "act_quantizer", None), "act_scale", None) is not None}
    sd = {k: v.detach().cpu().float() for k, v in m.state_dict().items() if "weight_quantizer" not in k and "act_quantizer" not in k}

    def run(B, on):
        monkeypatch.setattr(stdit, "_BATCH_QUANT", on)
        rep = B // 4
        xin = torch.cat([(x4.float() * (1.0 + 0.25 * r)).half() for r in range(rep)])
        y2, t0, off = y4.repeat(rep, 1), t4.repeat(rep, 1), stdit.seq_offsets([L] * B, dev)
        with torch.no_grad():
            kv = blk.prompt_kv(y2)
            before = dict(count)
            o = blk.forward_fused(xin.clone(), y2, t0, off, None, B, kv_ready=kv)
        spec = sr.QSpec(w_bits=8, a_bits=8, act_scale=act_scale, alpha=[0.11, 0.11], timerange=[[0, 500], [501, 1000]])
        ref = sr.stdit_block(sd, 0, xin.cpu().float().view(B, T * S, C), y2.cpu().float().view(1, -1, C), t0.cpu().float(), [L] * B,
                             None, T, S, H, spec, 721)
        rel = float((o.cpu().double().view(B, T * S, C) - ref.double()).norm() / ref.double().norm())
        print("B %d, switch %s: rel-L2 to the oracle block %.3e" % (B, on, rel))
        return rel, {k: count[k] - before[k] for k in names}
    rel, calls = run(4, False)
    assert rel < 1e-3 and calls == dict(rowquant=8, ln_modulate_rowquant=2, gelu_rowquant=0, rowquant_batch=0,
                                        ln_modulate_rowquant_batch=0, gelu_rowquant_batch=0), (rel, calls)
    rel, calls = run(4, True)
    assert rel < 1e-3 and calls == dict(rowquant=0, ln_modulate_rowquant=0, gelu_rowquant=0, rowquant_batch=5,
                                        ln_modulate_rowquant_batch=2, gelu_rowquant_batch=1), (rel, calls)
    with pytest.raises(ops.VQError):
        run(16, False)
    assert run(16, True)[0] < 1e-3
    assert int(qnn.check_status()) == 0

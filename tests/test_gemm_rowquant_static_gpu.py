"""vq_gemm_i8_rowquant_static: mlp.fc1's int8 GEMM with GELU(tanh) and fc2's static tensor-wise quantizer in its epilogue -
the quantizing arm of the 256 x 288 and 128 x 288 tiles, general and interior form.  Codes, sx, zx and R against the two
launches they replace (vq_gemm_i8 with the GELU epilogue, then vq_rowquant's static case) bit for bit, on grids whose exact
ties and clamps are counted on the host from the two-launch fp16 output; chosen rows against the CPU oracle
(oracle/fakequant.py: static_act_quant); nothing written outside the rows of the launch, R independent of what it held;
every form bit-equal to the others; the block routes behind their switch; and a graph replayed twice.

Grid C, unsmoothed: GELU(tanh) is never below -0.17, so rint(h / 2^-5) + 16 >= 11 and the LOWER end of the 6-bit range
cannot be reached by any implementation; there the upper end must be reached and the lowest code must be 11 or less, and
both ends must be reached wherever a smoothing vector divides the input (entries below 0.34 bring -0.17 / s under -0.5)."""
import functools

import pytest
import torch

import quant_rows as qr
import test_gemm_rowquant_static_cpu as sc
from oracle import fakequant as fq
from test_quantizer_edges_gpu import _first_diff

pytestmark = pytest.mark.gpu

CASES = [(shape, v) for shape, variants in sc.SHAPES for v in variants]
CASE_IDS = ["%dx%dx%d-v%d" % (s + (v,)) for s, v in CASES]
GRIDS = {"A": (2.0 ** -6, 64.0, 8), "B": (2.0 ** -6, -8.0, 8), "C": (2.0 ** -5, 16.0, 6)}


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, dev):
    """Random int8 operands of out[M, N] = x[M, K] w[N, K]^T whose pre-activation has a standard deviation of about 2
    (codes uniform in +-100 around small zero points; sx[m] sw[n] = 2 / (58^2 sqrt(K)) up to +-20 %), computed once."""
    from viditq_amd import ops
    g = torch.Generator().manual_seed(1000 * M + N + K)
    Kp = ops.pad128(K)
    xs = torch.zeros(M, Kp, dtype=torch.int8)
    xs[:, :K] = torch.randint(-100, 101, (M, K), generator=g, dtype=torch.int8)
    ws = torch.zeros(N, Kp, dtype=torch.int8)
    ws[:, :K] = torch.randint(-100, 101, (N, K), generator=g, dtype=torch.int8)
    zx = torch.randint(-6, 7, (M,), generator=g, dtype=torch.int32)
    zw = torch.randint(-6, 7, (N,), generator=g, dtype=torch.int32)
    a = (2.0 / (58.0 * 58.0 * K ** 0.5)) ** 0.5
    sx = (a * (0.8 + 0.4 * torch.rand(M, generator=g))).float()
    sw = (a * (0.8 + 0.4 * torch.rand(N, generator=g))).float()
    R = (xs.int().sum(1) - K * zx).int()
    cs = ws.int().sum(1).int()
    bias = (torch.randn(N, generator=g) * 0.3).float()
    qa = ops.QAct(xs.to(dev), sx.to(dev), zx.to(dev), R.to(dev), K, 8)
    pw = ops.PackedWeight(ws.to(dev), sw.to(dev), zw.to(dev), cs.to(dev), N, K, Kp, 8)
    return qa, pw, bias.to(dev)


@functools.lru_cache(maxsize=None)
def _gelu_fp16(M, N, K, variant, dev):
    """What the fused launch never writes: vq_gemm_i8's fp16 output with the GELU epilogue (computed once, not modified)."""
    from viditq_amd import ops
    qa, pw, bias = _operands(M, N, K, dev)
    h = ops.gemm_i8(qa, pw, bias=bias, epilogue=ops.EPI_GELU, variant=variant)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(h).all())
    assert 1.5 < float(_pre_std(qa, pw, bias)) < 2.5
    return h


def _pre_std(qa, pw, bias):
    K = qa.K
    x = (qa.xq[:, :K].float() - qa.zx[:, None].float()) * qa.sx[:, None]
    w = (pw.wq[:, :K].float() - pw.zw[:, None].float()) * pw.sw[:, None]
    return (x @ w.t() + bias).std()


@functools.lru_cache(maxsize=None)
def _smooth(N, dev):
    """A log-normal smoothing vector with a valid reciprocal form (entries from about 0.15 to 6)."""
    from viditq_amd import ops
    s = torch.exp(torch.randn(N, generator=torch.Generator().manual_seed(7)) * 0.6).float().to(dev)
    assert ops.smooth_rcp(s) is not None
    return s


def _grid(name, dev):
    d, z, nb = GRIDS[name]
    return torch.tensor([d], dtype=torch.float32, device=dev), torch.tensor([z], dtype=torch.float32, device=dev), nb


@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fused_gemm_quantizer_equals_two_launches(ops, dev, case, grid, smooth):
    (M, N, K), variant = case
    qa, pw, bias = _operands(M, N, K, dev)
    h = _gelu_fp16(M, N, K, variant, dev)
    delta, zp, n_bits = _grid(grid, dev)
    s = _smooth(N, dev) if smooth else None
    Kp_out, qmax, cx = ops.pad128(N), 2 ** n_bits - 1, 128 if n_bits == 8 else 0
    got = ops.gemm_i8_rowquant_static(qa, pw, bias, delta, zp, n_bits, s=s, variant=variant)
    assert got is not None and got.n_bits == n_bits and got.K == N and got.xq.shape == (M, Kp_out)
    ref = ops.rowquant(h.view(1, M, N), n_bits=n_bits, delta=delta, zp=zp, s=s)
    for f in ("xq", "sx", "zx", "R"):
        x, y = getattr(got, f), getattr(ref, f)
        assert x.shape == y.shape and x.dtype == y.dtype
        assert torch.equal(x, y), _first_diff(x.cpu().int() if f != "sx" else x.cpu(), y.cpu().int() if f != "sx" else y.cpu(), f)
    assert bool((got.xq[:, N:] == 0).all()), "pad columns"
    assert bool((got.sx == delta).all()) and bool((got.zx == int(zp) - cx).all())
    raw = ref.xq[:, :N].int() + cx
    assert torch.equal(got.R, (raw.sum(1) - N * int(zp)).int())
    if M * N < 10 ** 5:
        return
    # not vacuous: counted on the host from the two-launch fp16 output h (q0: its levels) and from the quantizer's own input
    # (q: the levels of h, or of the IEEE quotients h / s)
    q0 = h.cpu().double() / float(delta)
    q = qr.smoothed(h.cpu()[None], None if s is None else s.cpu())[0].double() / float(delta)
    lev0, lev = torch.round(q0) + float(zp), torch.round(q) + float(zp)
    name = CASE_IDS[CASES.index(case)]
    if grid == "A":
        tie = ((q0 - torch.floor(q0)) == 0.5) & (lev0 >= 0) & (lev0 <= qmax)
        parity = torch.floor(q0[tie]).long() % 2
        print("grid A %s: ties %.3f %%, above the grid %.3f %%" % (name, 100 * float(tie.double().mean()),
                                                                  100 * float((lev0 > qmax).double().mean())))
        assert float(tie.double().mean()) >= 0.005
        assert bool((parity == 0).any()) and bool((parity == 1).any())
        assert bool((lev0 > qmax).any()) and bool((lev > qmax).any()) and int(raw.max()) == qmax, "the upper clamp must act"
    elif grid == "B":
        print("grid B %s: below the grid %.3f %%" % (name, 100 * float((lev0 < 0).double().mean())))
        assert bool((lev0 < 0).any()) and bool((lev < 0).any()) and int(raw.min()) == 0, "the lower clamp must act"
    else:
        print("grid C %s: codes %d .. %d" % (name, int(raw.min()), int(raw.max())))
        assert int(raw.max()) == qmax, "the upper end of the 6-bit range"
        assert int(raw.min()) == 0 if smooth else int(raw.min()) <= 11, "the lower end (module docstring)"


@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_chosen_rows_against_the_oracle(ops, dev, grid, smooth):
    """Rows of the fused output at (300, 1160, 200) - first and last of the launch, both sides of the 128- and 256-row tile
    edges - carry the codes of oracle.fakequant.static_act_quant of the (smoothed) two-launch fp16 row."""
    M, N, K = 300, 1160, 200
    qa, pw, bias = _operands(M, N, K, dev)
    h = _gelu_fp16(M, N, K, -1, dev).cpu()
    delta, zp, n_bits = _grid(grid, dev)
    s = _smooth(N, dev) if smooth else None
    got = ops.gemm_i8_rowquant_static(qa, pw, bias, delta, zp, n_bits, s=s)
    rows = torch.tensor([0, 1, 15, 16, 127, 128, 255, 256, 299])
    codes, _ = fq.static_act_quant(qr.smoothed(h[rows][None], None if s is None else s.cpu()), delta.cpu(), zp.cpu(), n_bits)
    cx = 128 if n_bits == 8 else 0
    mine = got.xq.cpu()[rows, :N].int() + cx
    assert torch.equal(mine, codes[0].int()), _first_diff(mine, codes[0].int(), "fused codes")
    assert torch.equal(got.R.cpu()[rows], (codes[0].int().sum(-1) - N * int(zp)).int())


def test_writes_only_its_rows_and_R_does_not_depend_on_what_it_held(ops, dev):
    """Rows past M exist in the last row tile and columns past N in the last column tile, but not in memory: with poison
    rows before and after every output nothing outside the launch's rows changes - and R, which the waves ADD into, does
    not depend on what it held (poisoned, then holding the first call's result)."""
    from viditq_amd import _lib
    M, N, K = 300, 1160, 200
    qa, pw, bias = _operands(M, N, K, dev)
    h = _gelu_fp16(M, N, K, -1, dev)
    delta, zp, n_bits = _grid("A", dev)
    Kp_out, pad = ops.pad128(N), 16
    assert Kp_out == 1280 and qa.Kp == 256
    bufs = {"xq": torch.full((M + 2 * pad, Kp_out), 0x5A, dtype=torch.int8, device=dev),
            "sx": torch.full((M + 2 * pad,), -7.0, dtype=torch.float32, device=dev),
            "zx": torch.full((M + 2 * pad,), -77, dtype=torch.int32, device=dev),
            "R": torch.full((M + 2 * pad,), -777, dtype=torch.int32, device=dev)}
    before = {n: t.clone() for n, t in bufs.items()}
    p = {n: t[pad:].data_ptr() for n, t in bufs.items()}
    first = None
    for _ in range(2):
        _lib.check(_lib.load().vq_gemm_i8_rowquant_static(
            qa.xq.data_ptr(), qa.sx.data_ptr(), qa.zx.data_ptr(), qa.R.data_ptr(), pw.wq.data_ptr(), pw.sw.data_ptr(),
            pw.zw.data_ptr(), pw.cs.data_ptr(), bias.data_ptr(), None, None, delta.data_ptr(), zp.data_ptr(), p["xq"],
            p["sx"], p["zx"], p["R"], M, N, K, qa.Kp, Kp_out, 8, n_bits, -1, torch.cuda.current_stream().cuda_stream),
            "vq_gemm_i8_rowquant_static")
        torch.cuda.synchronize()
        if first is None:
            first = bufs["R"].clone()
    assert torch.equal(bufs["R"], first), "R depends on what it held before the call"
    for n, t in bufs.items():
        assert torch.equal(t[:pad], before[n][:pad]) and torch.equal(t[pad + M:], before[n][pad + M:]), n
    ref = ops.rowquant(h.view(1, M, N), n_bits=n_bits, delta=delta, zp=zp)
    for n in bufs:
        assert torch.equal(bufs[n][pad:pad + M], getattr(ref, n)), n
    assert bool((bufs["xq"][pad:pad + M, N:] == 0).all())


@pytest.mark.parametrize("shape,variants", [((256, 1152, 128), (-1, 11, 16, 19)), ((128, 1152, 128), (-1, 11, 16)),
                                            ((300, 1160, 200), (-1, 11, 16)), ((64, 256, 64), (-1, 11, 16))],
                         ids=["256x1152x128", "128x1152x128", "300x1160x200", "64x256x64"])
def test_forms_agree(ops, dev, shape, variants):
    """The 256- and 128-row tiles, general and interior form, are bit-equal wherever each is legal ((256, 1152, 128)
    reaches all four: 11 and 19 the 256-row tile, 16 and the library's own choice the 128-row one)."""
    M, N, K = shape
    qa, pw, bias = _operands(M, N, K, dev)
    delta, zp, n_bits = _grid("C", dev)
    s = _smooth(N, dev)
    outs = [ops.gemm_i8_rowquant_static(qa, pw, bias, delta, zp, n_bits, s=s, variant=v) for v in variants]
    for v, o in zip(variants[1:], outs[1:]):
        for f in ("xq", "sx", "zx", "R"):
            assert torch.equal(getattr(o, f), getattr(outs[0], f)), (v, f)
    if 19 not in variants:
        with pytest.raises(ops.VQError):
            ops.gemm_i8_rowquant_static(qa, pw, bias, delta, zp, n_bits, s=s, variant=19)


# ----------------------------------------------------------------------------- the blocks' route
NAMES = ["rowquant_static", "rowquant", "gemm_i8", "gemm_i8_rowquant_static"]


def _count_block_calls(ops, monkeypatch, block_cls):
    """Per forward_fused call of ``block_cls``: the number of calls of every ops function in NAMES (the prompt's K / V
    computed beforehand where the block takes them)."""
    count = dict.fromkeys(NAMES, 0)
    for name in NAMES:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            count[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    per_block = []
    inner = block_cls.forward_fused

    def forward_fused(self, *a, **k):
        if hasattr(self, "prompt_kv") and k.get("kv_ready") is None:
            k["kv_ready"] = self.prompt_kv(a[1])
        before = dict(count)
        out = inner(self, *a, **k)
        per_block.append({n: count[n] - before[n] for n in count})
        return out
    monkeypatch.setattr(block_cls, "forward_fused", forward_fused)
    return per_block


def _switches_off(monkeypatch, stdit):
    for sw in ("_STATIC_GEMM_QUANT", "_STATIC_FWD_ATTN_QUANT", "_STATIC_ATTN_QUANT"):
        monkeypatch.setattr(stdit, sw, False)


def test_block_route_of_the_static_stdit_plan(ops, dev, monkeypatch):
    from helpers import load_npz, rel_l2
    from test_static_quant_gpu import _tiny_static_stdit
    from viditq_amd.t2v import stdit
    qnn, args, kw = _tiny_static_stdit(dev)
    g = load_npz("tiny_stdit_static.npz")
    _switches_off(monkeypatch, stdit)
    parent = qnn(*args, **kw)
    per_block = _count_block_calls(ops, monkeypatch, stdit.STDiTBlock)
    # switch off: today's launches and outputs
    off = qnn(*args, **kw)
    assert torch.equal(off, parent)
    n_gemm = per_block[0]["gemm_i8"]
    assert per_block == [dict(rowquant_static=3, rowquant=5, gemm_i8=n_gemm, gemm_i8_rowquant_static=0)] * 2
    del per_block[:]
    # the new switch on alone: same output, fc2's quantizer pass and fc1's plain launch gone
    monkeypatch.setattr(stdit, "_STATIC_GEMM_QUANT", True)
    on = qnn(*args, **kw)
    assert per_block == [dict(rowquant_static=3, rowquant=4, gemm_i8=n_gemm - 1, gemm_i8_rowquant_static=1)] * 2
    assert torch.equal(on, parent), "%d of %d values differ" % (int((on != parent).sum()), on.numel())
    del per_block[:]
    # all three static switches on
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", True)
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", True)
    every = qnn(*args, **kw)
    assert per_block == [dict(rowquant_static=3, rowquant=1, gemm_i8=n_gemm - 1, gemm_i8_rowquant_static=1)] * 2
    assert torch.isfinite(every).all()
    # the bound test_static_attn_quant_gpu.test_block_route_of_the_static_plan applies to this golden
    ref32, ref16 = g["tw_joint_t721"], g["tw_joint_t721_ref_fp16"]
    assert rel_l2(every.cpu(), ref32) < 1.25 * rel_l2(ref16, ref32) + 1e-4
    # without the one-pass static route the switch does nothing: the layerwise route, as before
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    del per_block[:]
    layerwise = qnn(*args, **kw)
    assert torch.equal(layerwise, parent)
    assert all(b["gemm_i8_rowquant_static"] == 0 and b["gemm_i8"] == n_gemm for b in per_block)


def test_block_route_of_the_naive_pixart_plan(ops, dev, monkeypatch):
    from test_static_quant_gpu import _tiny_naive_pixart
    from viditq_amd.t2i import pixart
    from viditq_amd.t2v import stdit
    qn, args, kw = _tiny_naive_pixart(dev)
    _switches_off(monkeypatch, stdit)
    parent = qn(*args, **kw)
    per_block = _count_block_calls(ops, monkeypatch, pixart.PixArtMSBlock)
    off = qn(*args, **kw)
    assert torch.equal(off, parent)
    n_blocks = len(qn.model.blocks)
    n_gemm = per_block[0]["gemm_i8"]
    assert per_block == [dict(rowquant_static=2, rowquant=5, gemm_i8=n_gemm, gemm_i8_rowquant_static=0)] * n_blocks
    del per_block[:]
    monkeypatch.setattr(stdit, "_STATIC_GEMM_QUANT", True)
    on = qn(*args, **kw)
    assert per_block == [dict(rowquant_static=2, rowquant=4, gemm_i8=n_gemm - 1, gemm_i8_rowquant_static=1)] * n_blocks
    assert torch.equal(on, parent), "%d of %d values differ" % (int((on != parent).sum()), on.numel())
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    del per_block[:]
    layerwise = qn(*args, **kw)
    assert torch.equal(layerwise, parent)
    assert all(b["gemm_i8_rowquant_static"] == 0 and b["gemm_i8"] == n_gemm for b in per_block)


def test_switched_on_forward_replays_from_a_graph(ops, dev, monkeypatch):
    """The grid is read on the device and R is zeroed by a kernel node on the stream: nothing synchronises, so the
    switched-on forward is capturable, and its replays return the eager result bit for bit - the second one too, which an
    R that is not zeroed in every replay would not."""
    from test_static_quant_gpu import _tiny_static_stdit
    from viditq_amd.t2v import stdit
    _switches_off(monkeypatch, stdit)
    monkeypatch.setattr(stdit, "_STATIC_GEMM_QUANT", True)
    qnn, args, kw = _tiny_static_stdit(dev)
    kw = dict(kw, timestep_id=int(args[1][0]))             # (known on the host: no t[0].item() under capture)
    calls = []
    real = ops.gemm_i8_rowquant_static
    monkeypatch.setattr(ops, "gemm_i8_rowquant_static", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    from viditq_amd.graph import ForwardGraph
    with torch.no_grad():
        eager = qnn(*args, **kw).clone()
    assert calls, "the switched-on forward did not take the fused route"
    fg = ForwardGraph(qnn, *args, kw)
    out = fg.run(*args)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    out2 = fg.run(*args).clone()
    torch.cuda.synchronize()
    assert torch.equal(out2, eager)

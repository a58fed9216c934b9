"""vq_attn_fwd_rowquant_static: spatial / cross attention with proj's static tensor-wise quantizer fused in - the
static-grid forms of attn_fwd_kernel, attn_fwd32d_kernel, attn_fwd64d_kernel and attn_cross32_kernel (2..5 tile images).
The fp16 output against vq_attn_fwd's bit for bit; codes, sx, zx and R against vq_rowquant's static case on that output
and against the CPU oracle (oracle/fakequant.py: static_act_quant) on exact ties, both clamps and fp16's largest value;
nothing written outside the rows of the launch, R independent of what it held; and the block routes behind their switch."""
import functools

import pytest
import torch

import attn_regimes as ar
import quant_rows as qr
import test_static_fwd_attn_quant_cpu as sc
from oracle import fakequant as fq
from test_quantizer_edges_gpu import _first_diff

pytestmark = pytest.mark.gpu

IDS = ar.kernel_ids()
N = len(sc.SHAPES)


def _lib():
    from viditq_amd import _lib as L
    return L.load()


def _launch_inputs(i, q, k, v, dev):
    """Device buffers and launch arguments of SHAPES[i] for q, k, v [n, L, H, D] (attn_regimes.fwd_layout: K | V share rows,
    packed by offsets or one dense block per sequence)."""
    case = sc.shape_case(i)
    a = ar.fwd_layout(case)
    n, lens, Cc = a["n_seq"], case["shape"]["lens"], a["H"] * a["D"]
    qd = q.reshape(n * a["Lq"], Cc).to(dev)
    if a["offs"] is not None:
        kvd = torch.cat([torch.cat([k[s, :L].reshape(L, Cc), v[s, :L].reshape(L, Cc)], 1) for s, L in enumerate(lens)]).to(dev)
        off = torch.tensor(a["offs"], dtype=torch.int32, device=dev)
    else:
        kvd = torch.cat([k.reshape(n * lens[0], Cc), v.reshape(n * lens[0], Cc)], 1).to(dev)
        off = None
    route = _lib().vq_attn_fwd_route(qd.data_ptr(), kvd.data_ptr(), kvd[:, Cc:].data_ptr(), qd.data_ptr(), n, a["Lq"], a["Lk"],
                                     a["H"], a["D"], a["q_seq"], a["q_tok"], a["kv_seq"], a["kv_tok"], a["o_seq"], a["o_tok"],
                                     None if off is None else off.data_ptr(), case["scale"], None)
    assert route == IDS[case["kernel"]], (case["id"], route)       # the kernel under test is the one the shape names
    return a, qd, kvd, off


def _plain(ops, a, qd, kvd, off):
    Cc = a["H"] * a["D"]
    o = torch.full((a["n_seq"] * a["Lq"], Cc), float("nan"), dtype=torch.float16, device=qd.device)
    ops.attn_fwd(qd, kvd, kvd[:, Cc:], o, a["n_seq"], a["Lq"], a["Lk"], a["H"], a["D"], a["q_seq"], a["q_tok"], a["kv_seq"],
                 a["kv_tok"], a["o_seq"], a["o_tok"], kv_off=off)
    return o


def _fused(ops, a, qd, kvd, off, delta, zp, n_bits, s=None, o=None):
    Cc = a["H"] * a["D"]
    return ops.attn_fwd_rowquant_static(qd, kvd, kvd[:, Cc:], a["n_seq"], a["Lq"], a["Lk"], a["H"], a["D"], a["q_seq"],
                                        a["q_tok"], a["kv_seq"], a["kv_tok"], delta, zp, n_bits=n_bits, kv_off=off, o=o,
                                        o_seq_stride=a["o_seq"], o_tok_stride=a["o_tok"], s=s)


@functools.lru_cache(maxsize=None)
def _gaussian(i, dev):
    """Gaussian q / k / v of SHAPES[i] (one V row zeroed) on the device and vq_attn_fwd's output of them, computed once."""
    import viditq_amd  # noqa: F401
    from viditq_amd import ops
    kern, D, n, Lq, lens, H, kv_off = sc.SHAPES[i]
    g = torch.Generator().manual_seed(500 + i)
    q = torch.randn(n, Lq, H, D, generator=g).half()
    k = torch.randn(n, max(lens), H, D, generator=g).half()
    v = torch.randn(n, max(lens), H, D, generator=g).half()
    v[0, min(lens) // 2] = 0                              # one value row zeroed
    a, qd, kvd, off = _launch_inputs(i, q, k, v, dev)
    return a, qd, kvd, off, _plain(ops, a, qd, kvd, off)


@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "smooth"])
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("i", range(N), ids=sc.SHAPE_IDS)
def test_static_fused_fwd_attention_equals_two_kernels(ops, dev, i, n_bits, smooth):
    a, qd, kvd, off, o_ref = _gaussian(i, dev)
    Cc, rows = a["H"] * a["D"], a["n_seq"] * a["Lq"]
    assert bool(torch.isfinite(o_ref).all())
    sm = torch.exp(torch.randn(Cc, generator=torch.Generator().manual_seed(3)) * 0.6).float().to(dev) if smooth else None
    # the grid from the 2nd and 98th percentile of what the quantizer sees: both clamps act
    xin = o_ref.float() if sm is None else o_ref.float() / sm
    lo, hi = [float(x) for x in torch.quantile(xin.flatten()[:: max(1, xin.numel() // 200000)], torch.tensor([0.02, 0.98], device=dev))]
    qmax = 2 ** n_bits - 1
    delta = torch.tensor([(hi - lo) / qmax], dtype=torch.float32, device=dev)
    zp = torch.round(-lo / delta)
    o = torch.full_like(o_ref, float("nan"))
    got = _fused(ops, a, qd, kvd, off, delta, zp, n_bits, s=sm, o=o)
    assert got is not None and got.n_bits == n_bits and got.K == Cc and got.xq.shape == (rows, ops.pad128(Cc))
    assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16)), _first_diff(o.cpu().float(), o_ref.cpu().float(), "o")
    ref = ops.rowquant(o_ref.view(1, rows, Cc), n_bits=n_bits, delta=delta, zp=zp, s=sm, fast_div=False)
    for f in ("xq", "sx", "zx", "R"):
        x, y = getattr(got, f), getattr(ref, f)
        assert x.shape == y.shape and torch.equal(x, y), _first_diff(x.cpu().int(), y.cpu().int(), f)
    cx = 128 if n_bits == 8 else 0
    raw = got.xq[:, :Cc].int() + cx
    assert int(raw.min()) == 0 and int(raw.max()) == qmax, "both clamps must act"
    assert bool((got.xq[:, Cc:] == 0).all())
    got2 = _fused(ops, a, qd, kvd, off, delta, zp, n_bits, s=sm)          # o = None
    for f in ("xq", "sx", "zx", "R"):
        assert torch.equal(getattr(got2, f), getattr(got, f)), f


@pytest.mark.parametrize("smooth", [False, True], ids=["plain", "q2_smooth"])
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("i", range(N), ids=sc.SHAPE_IDS)
def test_static_fused_fwd_attention_edge_rows_against_the_oracle(ops, dev, i, n_bits, smooth):
    """One-hot attention whose V rows are quant_rows.static_rows (ties of both parities, values beyond both grid ends,
    +-65504): a selected output row IS the hot V row of every head, so codes, sx, zx and R must be the oracle's static
    quantizer of it."""
    kern, D, n, Lq, lens, H, kv_off = sc.SHAPES[i]
    Cc, rows = H * D, n * Lq
    s = qr.q2_smooth(Cc) if smooth else None
    q, k, _, hot = sc.one_hot(i)
    v, delta, zp = sc.static_v(i, n_bits)
    a, qd, kvd, off = _launch_inputs(i, q, k, v, dev)
    o = torch.full((rows, Cc), float("nan"), dtype=torch.float16, device=dev)
    qa = _fused(ops, a, qd, kvd, off, delta.to(dev), zp.to(dev), n_bits, s=None if s is None else s.to(dev), o=o)
    assert qa is not None
    torch.cuda.synchronize()
    sel = sc.one_hot_selected(i).reshape(rows)
    assert float(sel.double().mean()) >= 0.9
    idx = sel.nonzero()[:, 0]
    want = sc.hot_rows(v, hot).reshape(rows, Cc)[idx]
    assert torch.equal(o.cpu()[idx], want), "the output is not the hot V row"
    codes, _ = fq.static_act_quant(qr.smoothed(want[None], s), delta, zp, n_bits)
    cx = 128 if n_bits == 8 else 0
    got = qa.xq.cpu()[idx, :Cc].int() + cx
    assert torch.equal(got, codes[0].int()), _first_diff(got, codes[0].int(), "fused static codes")
    assert int(got.min()) == 0 and int(got.max()) == 2 ** n_bits - 1
    assert bool((qa.xq[:, Cc:] == 0).all())
    assert torch.equal(qa.sx.cpu(), delta.expand(rows))
    zx = int(zp) - cx
    assert torch.equal(qa.zx.cpu(), torch.full((rows,), zx, dtype=torch.int32))
    assert torch.equal(qa.R.cpu()[idx], ((codes[0].int() - cx).sum(-1) - Cc * zx).int())


# one attn_fwd_kernel shape (offsets, Lq % 128 != 0), one attn_fwd32d_kernel shape with a ragged last query tile, one
# attn_cross32_kernel shape with offsets
@pytest.mark.parametrize("i", [0, 3, 9], ids=[sc.SHAPE_IDS[j] for j in (0, 3, 9)])
def test_static_fused_fwd_attention_writes_only_its_rows(ops, dev, i):
    """Queries past Lq exist in the kernels (clamped to row Lq - 1) but not in memory: with poison rows before and after
    every output and poison in the gap columns of a strided o, nothing outside the launch's rows changes - and R, which the
    heads ADD into, does not depend on what it held (poisoned, then holding the first call's result)."""
    from viditq_amd import _lib
    a, qd, kvd, off, o_ref = _gaussian(i, dev)
    Cc, rows, pad = a["H"] * a["D"], a["n_seq"] * a["Lq"], 16
    Kp, ldo = ops.pad128(Cc), Cc + 8
    delta = torch.tensor([0.01], device=dev)
    zp = torch.tensor([100.0], device=dev)
    bufs = {"xq": torch.full((rows + 2 * pad, Kp), 0x5A, dtype=torch.int8, device=dev),
            "sx": torch.full((rows + 2 * pad,), -7.0, dtype=torch.float32, device=dev),
            "zx": torch.full((rows + 2 * pad,), -77, dtype=torch.int32, device=dev),
            "R": torch.full((rows + 2 * pad,), -777, dtype=torch.int32, device=dev),
            "o": torch.full((rows + 2 * pad, ldo), 1234.0, dtype=torch.float16, device=dev)}
    before = {n: t.clone() for n, t in bufs.items()}
    p = {n: t[pad:].data_ptr() for n, t in bufs.items()}
    first = None
    for _ in range(2):
        _lib.check(_lib.load().vq_attn_fwd_rowquant_static(
            qd.data_ptr(), kvd.data_ptr(), kvd[:, Cc:].data_ptr(), None, None, delta.data_ptr(), zp.data_ptr(), p["xq"],
            p["sx"], p["zx"], p["R"], p["o"], a["n_seq"], a["Lq"], a["Lk"], a["H"], a["D"], a["q_seq"], a["q_tok"],
            a["kv_seq"], a["kv_tok"], a["Lq"] * ldo, ldo, None if off is None else off.data_ptr(), Kp, 8, a["D"] ** -0.5,
            torch.cuda.current_stream().cuda_stream), "vq_attn_fwd_rowquant_static")
        torch.cuda.synchronize()
        if first is None:
            first = bufs["R"].clone()
    assert torch.equal(bufs["R"], first), "R depends on what it held before the call"
    for n, t in bufs.items():
        assert torch.equal(t[:pad], before[n][:pad]) and torch.equal(t[pad + rows:], before[n][pad + rows:]), n
    assert bool((bufs["o"][:, Cc:] == 1234.0).all()), "gap columns of o"
    assert torch.equal(bufs["o"][pad:pad + rows, :Cc], o_ref)
    assert bool((bufs["sx"][pad:pad + rows] == 0.01).all()) and bool((bufs["zx"][pad:pad + rows] == -28).all())
    ref = ops.rowquant(o_ref.view(1, rows, Cc), delta=delta, zp=zp)
    assert torch.equal(bufs["xq"][pad:pad + rows], ref.xq) and torch.equal(bufs["R"][pad:pad + rows], ref.R)


# ----------------------------------------------------------------------------- the blocks' route
NAMES = ["rowquant_static", "rowquant", "attn_fwd", "attn_fwd_rowquant_static", "attn_temporal_rowquant_static"]


def _count_block_calls(ops, monkeypatch, block_cls, attn_args):
    """Per forward_fused call of ``block_cls``: the number of calls of every ops function in NAMES (the prompt's K / V
    computed beforehand where the block takes them).  ``attn_args`` collects the arguments of every ops.attn_fwd call."""
    count = dict.fromkeys(NAMES, 0)
    for name in NAMES:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            count[_name] += 1
            if _name == "attn_fwd":
                attn_args.append((a, k))
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


def _assert_supported_routes(ops, attn_args):
    """Every ops.attn_fwd launch of the switched-off forward takes a route that has a static-grid form."""
    lib = _lib()
    assert attn_args
    for a, k in attn_args:
        q, kk, v, o, n_seq, Lq, Lk, H, D, qs, qt, ks, kt, os_, ot = a[:15]
        off = k.get("kv_off")
        route = lib.vq_attn_fwd_route(q.data_ptr(), kk.data_ptr(), v.data_ptr(), o.data_ptr(), n_seq, Lq, Lk, H, D, qs, qt, ks,
                                      kt, os_, ot, None if off is None else off.data_ptr(), 1.0, None)
        assert route == IDS["VQ_ATTN_K_FWD"], route                # hidden 64, 4 heads: the general kernel
        assert ops.pad128(H * D) == 128 > H * D == 64              # pad columns exist


def test_block_route_of_the_static_stdit_plan(ops, dev, monkeypatch):
    from helpers import load_npz, rel_l2
    from test_static_quant_gpu import _tiny_static_stdit
    from viditq_amd.t2v import stdit
    qnn, args, kw = _tiny_static_stdit(dev)
    g = load_npz("tiny_stdit_static.npz")
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", False)
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", False)
    parent = qnn(*args, **kw)
    attn_args = []
    per_block = _count_block_calls(ops, monkeypatch, stdit.STDiTBlock, attn_args)
    # switch off: today's launches and outputs
    off = qnn(*args, **kw)
    assert torch.equal(off, parent)
    assert per_block == [dict(rowquant_static=3, rowquant=5, attn_fwd=2, attn_fwd_rowquant_static=0,
                              attn_temporal_rowquant_static=0)] * 2
    _assert_supported_routes(ops, attn_args)
    del per_block[:]
    # the new switch on alone: same output, two quantizer passes and both attn_fwd launches gone
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", True)
    on = qnn(*args, **kw)
    assert per_block == [dict(rowquant_static=3, rowquant=3, attn_fwd=0, attn_fwd_rowquant_static=2,
                              attn_temporal_rowquant_static=0)] * 2
    assert torch.equal(on, parent), "%d of %d values differ" % (int((on != parent).sum()), on.numel())
    del per_block[:]
    # both static switches on
    monkeypatch.setattr(stdit, "_STATIC_ATTN_QUANT", True)
    both = qnn(*args, **kw)
    assert per_block == [dict(rowquant_static=3, rowquant=2, attn_fwd=0, attn_fwd_rowquant_static=2,
                              attn_temporal_rowquant_static=1)] * 2
    assert torch.isfinite(both).all()
    # the bound test_static_attn_quant_gpu.test_block_route_of_the_static_plan applies to this golden
    ref32, ref16 = g["tw_joint_t721"], g["tw_joint_t721_ref_fp16"]
    assert rel_l2(both.cpu(), ref32) < 1.25 * rel_l2(ref16, ref32) + 1e-4
    # without the one-pass static route the switches do nothing: the layerwise route, as before
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    del per_block[:]
    layerwise = qnn(*args, **kw)
    assert torch.equal(layerwise, parent)
    assert all(b["attn_fwd_rowquant_static"] == 0 and b["attn_fwd"] == 2 for b in per_block)


def test_block_route_of_the_naive_pixart_plan(ops, dev, monkeypatch):
    from test_static_quant_gpu import _tiny_naive_pixart
    from viditq_amd.t2i import pixart
    from viditq_amd.t2v import stdit
    qn, args, kw = _tiny_naive_pixart(dev)
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", False)
    parent = qn(*args, **kw)
    attn_args = []
    per_block = _count_block_calls(ops, monkeypatch, pixart.PixArtMSBlock, attn_args)
    off = qn(*args, **kw)
    assert torch.equal(off, parent)
    n_blocks = len(qn.model.blocks)
    # LN + qkv and LN + fc1 in one pass each; proj, q_linear, kv_linear (the prompt), proj and fc2 one quantizer each
    assert per_block == [dict(rowquant_static=2, rowquant=5, attn_fwd=2, attn_fwd_rowquant_static=0,
                              attn_temporal_rowquant_static=0)] * n_blocks
    _assert_supported_routes(ops, attn_args)
    del per_block[:]
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", True)
    on = qn(*args, **kw)
    assert per_block == [dict(rowquant_static=2, rowquant=3, attn_fwd=0, attn_fwd_rowquant_static=2,
                              attn_temporal_rowquant_static=0)] * n_blocks
    assert torch.equal(on, parent), "%d of %d values differ" % (int((on != parent).sum()), on.numel())
    monkeypatch.setattr(stdit, "_STATIC_FUSED", False)
    del per_block[:]
    layerwise = qn(*args, **kw)
    assert torch.equal(layerwise, parent)
    assert all(b["attn_fwd_rowquant_static"] == 0 and b["attn_fwd"] == 2 for b in per_block)


def test_switched_on_forward_replays_from_a_graph(ops, dev, monkeypatch):
    """The grid is read on the device and R is zeroed by a memset node on the stream: nothing synchronises, so the
    switched-on forward is capturable and its replay (memset, kernel, atomics) returns the eager result bit for bit."""
    from test_static_quant_gpu import _tiny_static_stdit
    from viditq_amd.t2v import stdit
    monkeypatch.setattr(stdit, "_STATIC_FWD_ATTN_QUANT", True)
    qnn, args, kw = _tiny_static_stdit(dev)
    kw = dict(kw, timestep_id=int(args[1][0]))             # (known on the host: no t[0].item() under capture)
    calls = []
    real = ops.attn_fwd_rowquant_static
    monkeypatch.setattr(ops, "attn_fwd_rowquant_static", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
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

"""vq_rowquant_smooth_multi_shared: the smoothed q | k | v quantizers of a joint cond | uncond forward (x [2, n_tok, C], a
token's grid shared by its rows of both samples) from ONE pass over the rows - smooth_rowquant_multi_kernel<.., PAIR>,
plain and behind LayerNorm + modulate.  The plain arm against the CPU oracle bit for bit on the edge rows of quant_rows.py,
both arms against the launches they replace (every field, bit for bit), the LayerNorm arm against the oracle at the bounds
of test_ln_modulate_rowquant_edges and - figure only - against today's generic three-output call, nothing written outside
the rows of a launch, the block's routes behind VQ_SMOOTH_JOINT in child processes, and graph replay."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import quant_rows as qr
from oracle import fakequant as fq
from test_quantizer_edges_gpu import _check_exact, _first_diff
from test_smooth_joint_cpu import WIDTHS, edge_rows, vectors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("xq", "sx", "zx", "R")
N_TOK = (1, 7, 8, 9, 131)       # a lone token, a partial workgroup, one full workgroup (8 waves = 8 tokens), one plus a token


def _same(got, ref, what):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        assert a.shape == b.shape and torch.equal(a, b), _first_diff(a.cpu().float(), b.cpu().float(), "%s %s" % (what, f))


def _smooth(C, dev, n=3):
    return [torch.exp(torch.randn(C, generator=torch.Generator().manual_seed(40 + j)) * 0.6).float().to(dev) for j in range(n)]


def _gauss(n_tok, C, seed):
    return (torch.randn(2, n_tok, C, generator=torch.Generator().manual_seed(seed)) * 1.5).half()


_edge_rows = functools.lru_cache(maxsize=None)(edge_rows)


# ----------------------------------------------------------------------------- 1. plain arm against the oracle, exactly
@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("C", [1152, 768, 1024, 1280])
def test_plain_arm_edges_against_the_oracle(ops, dev, C, G, n_bits):
    """Exact ties, near ties from both sides, symmetric rows, the eps threshold, fp16 extremes and planted extrema
    (quant_rows.py, B = 2) behind the Q2 vector, its mirror and a wide one: codes, delta, zero point, R and the status word
    bit for bit.  C = 1152: every exact row, and 131, 65 and 3 of them; the other widths: 131 rows."""
    vec = vectors(C)[:G]
    dvec = [v.to(dev) for v in vec]
    for v in dvec:
        assert ops.smooth_rcp(v) is not None
    exact, flagged, _ = _edge_rows(C, n_bits)
    sets = [exact, qr.thin(exact, 131), qr.thin(exact, 65), qr.thin(exact, 3)] if C == 1152 else [qr.thin(exact, 131)]
    for x in sets:
        st = ops.new_status(dev)
        outs = ops.rowquant_multi_shared(x.to(dev), dvec, n_bits=n_bits, status=st)
        assert outs is not None and len(outs) == G
        for j, (qa, v) in enumerate(zip(outs, vec)):
            _check_exact(qa, st, x, n_bits, v, "shared%d C%d out%d b%d n%d" % (G, C, j, n_bits, x.shape[1]))
    for i, x in enumerate(flagged if C == 1152 else flagged[:3]):
        st = ops.new_status(dev)
        assert ops.rowquant_multi_shared(x.to(dev), dvec, n_bits=n_bits, status=st) is not None
        assert int(st.item()) == 1, "C%d b%d flagged launch %d: status %d" % (C, n_bits, i, int(st.item()))


# ----------------------------------------------------------------------------- 2. plain arm against the launches it replaces
@pytest.mark.parametrize("n_bits", [8, 6, 4, 2])
@pytest.mark.parametrize("C", WIDTHS)
def test_plain_arm_equals_one_launch_per_output(ops, dev, C, n_bits):
    """Output j is ops.rowquant(x, n_bits, s=s_j) at B = 2 (smooth_rowquant_half_kernel<.., PAIR>), every field.  Q6 plants the
    unique extremum of a token in a chosen sample: a missing merge across the half-waves fails there."""
    sv = _smooth(C, dev)
    xs = [("gauss%d" % n, _gauss(n, C, 7 * n + C)) for n in N_TOK] + [("q6", qr.q6(2, C))]
    for name, x in xs:
        xd = x.to(dev)
        for G in ((1, 2, 3) if x.shape[1] == 9 else (3,)):
            st = ops.new_status(dev)
            outs = ops.rowquant_multi_shared(xd, sv[:G], n_bits=n_bits, status=st)
            assert outs is not None and len(outs) == G
            for j, qa in enumerate(outs):
                assert qa.xq.shape == (2 * x.shape[1], ops.pad128(C)) and qa.K == C and qa.n_bits == n_bits
                _same(qa, ops.rowquant(xd, n_bits=n_bits, s=sv[j]), "%s C%d b%d G%d out%d" % (name, C, n_bits, G, j))
            assert int(st.item()) == 0


# ----------------------------------------------------------------------------- 3. LayerNorm arm against the launches it replaces
def _mod(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, C, generator=g) * 0.3).float().to(dev) for _ in range(2)]    # the two samples differ


@pytest.mark.parametrize("n_bits", [8, 6])
@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("C", WIDTHS)
def test_ln_arm_equals_one_launch_per_output(ops, dev, C, G, n_bits):
    """Output j is ops.ln_modulate_rowquant(x, shift, scale, smooth=[s_j], n_bits) at B = 2 (smooth_rowquant_half_kernel<.., LN,
    .., PAIR>), every field.  shift / scale differ between the samples: sample 0's vectors in the upper half fail."""
    sv = _smooth(C, dev, G)
    shift, scale = _mod(C, dev, C + G)
    assert not torch.equal(shift[0], shift[1]) and not torch.equal(scale[0], scale[1])
    for n in N_TOK:
        xd = _gauss(n, C, 11 * n + C).to(dev)
        st = ops.new_status(dev)
        outs = ops.rowquant_multi_shared(xd, sv, n_bits=n_bits, status=st, shift=shift, scale=scale)
        assert outs is not None and len(outs) == G
        for j, qa in enumerate(outs):
            ref = ops.ln_modulate_rowquant(xd, shift, scale, 1e-6, smooth=[sv[j]], n_bits=n_bits)[0]
            _same(qa, ref, "ln n%d C%d b%d G%d out%d" % (n, C, n_bits, G, j))
        assert int(st.item()) == 0


@pytest.mark.parametrize("name", qr.LN_FAMILIES)
def test_ln_arm_edges_against_the_oracle(ops, dev, name):
    """Q3 / Q5 / Q6 behind LayerNorm + modulate and three vectors, against the oracle at the bounds of
    test_ln_modulate_rowquant_edges: at most one code step on under 0.5 % of the elements, dequantized rel-L2 under 2e-3,
    delta to 1e-5 (test_quant_rows_cpu.py shows the oracle itself stays inside them on these rows)."""
    B, C = 2, 1152
    x, shift, scale = qr.ln_inputs(name, B, C)
    n_tok = x.shape[1]
    smooth = [(torch.rand(C, generator=torch.Generator().manual_seed(50 + j)) + 0.5).float() for j in range(3)]
    xm = fq.t2i_modulate(fq.layernorm_noaffine(x.float()), shift[:, None, :], scale[:, None, :])
    st = ops.new_status(dev)
    outs = ops.rowquant_multi_shared(x.to(dev), [s.to(dev) for s in smooth], status=st, shift=shift.to(dev), scale=scale.to(dev))
    assert outs is not None
    for j, (s, qa) in enumerate(zip(smooth, outs)):
        codes, dq, delta, zp, eps = fq.dyn_act_quant(xm / s, 8)
        assert not eps
        got = qa.xq[:, :C].cpu().int().reshape(B, n_tok, C) + 128
        diff = (got - codes.int()).abs()
        print("%s out%d: max code step %d, share %.3g" % (name, j, int(diff.max()), float((diff > 0).float().mean())))
        assert int(diff.max()) <= 1
        assert float((diff > 0).float().mean()) < 5e-3
        got_dq = (got.float() - (qa.zx.cpu().reshape(B, n_tok, 1) + 128)) * qa.sx.cpu().reshape(B, n_tok, 1)
        rel = float((got_dq.double() - dq.double()).norm() / dq.double().norm())
        assert rel < 2e-3, rel
        assert torch.allclose(qa.sx.cpu().reshape(B, n_tok)[0], delta.reshape(-1), rtol=1e-5)
        assert torch.equal(qa.sx[:n_tok], qa.sx[n_tok:]) and torch.equal(qa.zx[:n_tok], qa.zx[n_tok:])   # one grid per token
    assert int(st.item()) == 0


# ----------------------------------------------------------------------------- 4. LayerNorm arm against today's generic call
def test_ln_arm_against_the_generic_three_output_call(ops, dev):
    """Today's route of the block's (q, k, v) at B = 2 is the generic ln_modulate_rowquant_kernel<3>, which sums a row in
    the wave order; the pair kernel sums it in the half-wave order.  Nothing is asserted beyond test 3 and the oracle
    bounds above: the count of codes that differ is printed for the record."""
    C, n = 1152, 2048
    sv = _smooth(C, dev)
    shift, scale = _mod(C, dev, 5)
    xd = _gauss(n, C, 99).to(dev)
    new = ops.rowquant_multi_shared(xd, sv, shift=shift, scale=scale)
    old = ops.ln_modulate_rowquant(xd, shift, scale, 1e-6, smooth=sv)
    assert new is not None and len(old) == 3
    for j in range(3):
        d = (new[j].xq.int() - old[j].xq.int()).abs()
        print("generic vs pair, output %d: %d of %d codes differ (max step %d), %d of %d grids" % (
            j, int((d > 0).sum()), d.numel(), int(d.max()), int((new[j].sx != old[j].sx).sum()), new[j].sx.numel()))


# ----------------------------------------------------------------------------- 5. guard rows
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("n_tok,C", [(1, 1152), (9, 768), (13, 1280)])
def test_writes_only_its_rows(ops, dev, n_tok, C, ln):
    """Pattern rows before and after every output: nothing outside rows [0, 2 n_tok) - Kp bytes each - changes, and a
    refused call leaves the pattern everywhere."""
    import ctypes
    from viditq_amd import _lib
    rows, pad = 2 * n_tok, 8
    sv = _smooth(C, dev)
    rcp = [ops.smooth_rcp(s) for s in sv]
    shift, scale = _mod(C, dev, 3) if ln else (None, None)
    xd = _gauss(n_tok, C, 21).to(dev)

    def fresh():
        return [{"xq": torch.full((rows + 2 * pad, C), 0x5A, dtype=torch.int8, device=dev),
                 "sx": torch.full((rows + 2 * pad,), -7.0, dtype=torch.float32, device=dev),
                 "zx": torch.full((rows + 2 * pad,), -77, dtype=torch.int32, device=dev),
                 "R": torch.full((rows + 2 * pad,), -777, dtype=torch.int32, device=dev)} for _ in range(3)]

    def call(bufs, B, x):
        arr = lambda vals: ctypes.cast((ctypes.c_void_p * 3)(*vals), ctypes.c_void_p)  # noqa: E731
        keep = [arr([s.data_ptr() for s in sv]), arr([r.data_ptr() for r in rcp])] + [
            arr([b[f][pad:].data_ptr() for b in bufs]) for f in FIELDS]
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return _lib.load().vq_rowquant_smooth_multi_shared(p(x), p(shift), p(scale), 1e-6, 3, *keep, B, n_tok, x.shape[-1],
                                                           x.shape[-1], 6, None, torch.cuda.current_stream().cuda_stream)
    bufs = fresh()
    assert call(bufs, 2, xd) == 0
    torch.cuda.synchronize()
    want = fresh()[0]
    ref = ops.rowquant_multi_shared(xd, sv, n_bits=6, shift=shift, scale=scale)
    for j, b in enumerate(bufs):
        for f in FIELDS:
            assert torch.equal(b[f][:pad], want[f][:pad]) and torch.equal(b[f][pad + rows:], want[f][pad + rows:]), (j, f)
            assert torch.equal(b[f][pad:pad + rows], getattr(ref[j], f)), (j, f)
    # refused: three samples (the entry point), an uncovered width (the wrapper): nothing is written
    bufs = fresh()
    assert call(bufs, 3, xd) == -4
    assert ops.rowquant_multi_shared(torch.zeros(2, n_tok, 896, dtype=torch.float16, device=dev),
                                     [torch.ones(896, device=dev)]) is None
    assert ops.rowquant_multi_shared(xd[:1], sv) is None
    torch.cuda.synchronize()
    for b in bufs:
        for f in FIELDS:
            assert torch.equal(b[f], want[f]), f


# ----------------------------------------------------------------------------- 6. the block's routes
_BLOCK_CHILD = r"""
import json, sys
import torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import viditq_amd
from viditq_amd import ops, synth
from viditq_amd.config import loads_yaml
from viditq_amd.t2v import stdit
from oracle import stdit_ref as sr
dev = torch.device("cuda:0")
NAMES = ["rowquant", "rowquant_multi_shared", "ln_modulate_rowquant", "rowquant_multi"]
count = dict.fromkeys(NAMES, 0)
for name in NAMES:
    def counted(*a, _real=getattr(ops, name), _name=name, **k):
        count[_name] += 1
        return _real(*a, **k)
    setattr(ops, name, counted)
out = {"switch": stdit._SMOOTH_JOINT}
T, S, H, C = 2, 8, 16, 1152
with torch.no_grad():
    for bits in (8, 6):
        text = synth.W4A8_TIMESTEP_AWARE.replace("cfg_split: True", "cfg_split: False")
        text = text.replace("quantizer: {n_bits: 4,", "quantizer: {n_bits: %%d," %% bits).replace("            n_bits: 8\n", "            n_bits: %%d\n" %% bits)
        cfg = loads_yaml(text)
        assert cfg.quant.weight.quantizer.n_bits == bits and cfg.quant.activation.quantizer.n_bits == bits
        m = synth.build_stdit(dev, depth=1, input_size=(T, 4, 8), model_max_length=12, caption_channels=64, seed=5)
        qnn = synth.quantize_model(m, cfg)
        blk = qnn.model.blocks[0]
        assert blk.d_t == T and blk.d_s == S and blk.fused_ok()
        g = torch.Generator().manual_seed(6)
        x = torch.randn(1, 4, T, 4, 8, generator=g).to(dev)
        y = (torch.randn(2, 1, 12, 64, generator=g) * 0.3).half().to(dev)
        mask = torch.zeros(2, 12, dtype=torch.int64)
        mask[0, :9] = 1
        mask[1, :12] = 1
        t = torch.tensor([721, 721], device=dev)
        seen = []
        inner = stdit.STDiTBlock.forward_fused
        def spy(self, x2, y2, t0, y_lens, tpe, B, kv_ready=None, mod=None):
            seen.append((x2.clone(), y2.clone(), t0.clone(), y_lens.clone(), B))
            return inner(self, x2, y2, t0, y_lens, tpe, B, kv_ready=kv_ready, mod=mod)
        stdit.STDiTBlock.forward_fused = spy
        qnn(torch.cat([x, x]), t, y, mask=mask.to(dev), timestep_id=721)        # sets the step, the status word, the block's inputs
        stdit.STDiTBlock.forward_fused = inner
        x2, y2, t0, off, B = seen[0]
        assert B == 2 and x2.shape == (2 * T * S, C)
        svs = [l.smooth_vector(*l._range_and_alpha()) for l in blk.hot_layers()]
        assert all(s is not None for s in svs)                                   # a smoothing vector on every Linear
        kv = blk.prompt_kv(y2)
        outs = []
        for rep in range(2):                                                     # the route without tpe: every block but the first
            xin = (x2.float() * (1.0 + 0.25 * rep)).half()
            before = dict(count)
            o = blk.forward_fused(xin.clone(), y2, t0, off, None, B, kv_ready=kv).clone()
            calls = {k: count[k] - before[k] for k in count}
            act_scale = {"blocks.0." + n: l.act_quantizer.act_scale.detach().cpu().float() for n, l in blk.named_modules()
                         if getattr(getattr(l, "act_quantizer", None), "act_scale", None) is not None}
            assert len(act_scale) == 13
            spec = sr.QSpec(w_bits=bits, a_bits=bits, act_scale=act_scale, alpha=[0.11, 0.11], timerange=[[0, 500], [501, 1000]])
            sd = {k: v.detach().cpu().float() for k, v in m.state_dict().items() if "weight_quantizer" not in k and "act_quantizer" not in k}
            lens = (off[1:] - off[:-1]).cpu().tolist()
            ref = sr.stdit_block(sd, 0, xin.cpu().float().view(2, T * S, C), y2.cpu().float().view(1, -1, C), t0.cpu().float(),
                                 lens, None, T, S, H, spec, 721)
            rel = float((o.cpu().float().view(2, T * S, C).double() - ref.double()).norm() / ref.double().norm())
            outs.append({"calls": calls, "rel": rel, "finite": bool(torch.isfinite(o).all())})
        out["b%%d" %% bits] = outs
        out["status%%d" %% bits] = int(qnn.check_status())
print("RESULT " + json.dumps(out))
"""


def _block_child(switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VQ_")}     # every route switch at its default
    if switch:
        env["VQ_SMOOTH_JOINT"] = "1"
    code = _BLOCK_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_block_routes_behind_the_switch(dev):
    """One STDiT block (C = 1152, 16 heads, d_t = 2, d_s = 8) of a joint forward with a smoothing vector on every Linear and
    dynamic 8-bit - and once 6-bit - grids, in a process without and one with VQ_SMOOTH_JOINT=1 (read once per process).
    Off: today's calls.  On: two ops.rowquant_multi_shared calls per forward, three fewer ops.rowquant calls and the (q, k,
    v) ops.ln_modulate_rowquant call gone.  Each of the two forwards within the per-block 1e-3 rel-L2 of the oracle block
    (README.md)."""
    off, on = _block_child(False), _block_child(True)
    assert off["switch"] is False and on["switch"] is True
    for bits in (8, 6):
        a, b = off["b%d" % bits], on["b%d" % bits]
        assert len(a) == len(b) == 2
        for fa, fb in zip(a, b):
            print("block, %d bits: rel-L2 to the oracle block %.3e (switch off), %.3e (switch on); calls %s -> %s" % (
                bits, fa["rel"], fb["rel"], fa["calls"], fb["calls"]))
        for fa, fb in zip(a, b):
            n = fa["calls"]["rowquant"]
            # the parent's calls: a1.proj, temporal q | k | v, a2.proj, cross_attn.q_linear, cross_attn.proj; LN for (q, k, v) and fc1
            assert fa["calls"] == dict(rowquant=7, rowquant_multi_shared=0, ln_modulate_rowquant=2, rowquant_multi=0)
            assert fb["calls"] == dict(rowquant=n - 3, rowquant_multi_shared=2, ln_modulate_rowquant=1, rowquant_multi=0)
            assert fa["finite"] and fb["finite"]
            assert fa["rel"] < 1e-3 and fb["rel"] < 1e-3, (bits, fa["rel"], fb["rel"])
        assert off["status%d" % bits] == 0 and on["status%d" % bits] == 0


# ----------------------------------------------------------------------------- 7. graph replay
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
def test_replays_from_a_graph(ops, dev, ln):
    """Nothing synchronises: a call is capturable (its vectors' reciprocals known from the eager pass), and each replay on
    changed inputs is the eager result."""
    C, n = 1152, 37
    sv = _smooth(C, dev)
    shift, scale = _mod(C, dev, 8) if ln else (None, None)
    xbuf = _gauss(n, C, 1).to(dev)
    run = lambda: ops.rowquant_multi_shared(xbuf, sv, n_bits=6, shift=shift, scale=scale)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert run() is not None                                       # warm-up: reciprocals, allocator
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    assert outs is not None
    for seed in (2, 3):
        xbuf.copy_(_gauss(n, C, seed).to(dev))
        if ln:
            shift.mul_(1.25)
        graph.replay()
        torch.cuda.synchronize()
        got = [{f: getattr(o, f).clone() for f in FIELDS} for o in outs]
        eager = run()
        for j in range(3):
            for f in FIELDS:
                assert torch.equal(got[j][f], getattr(eager[j], f)), (seed, j, f)

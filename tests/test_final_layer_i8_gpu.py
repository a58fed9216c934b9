"""ops.final_layer_i8 (vq_final_layer_i8, csrc/final_layer_i8.hip): an exactly computable family; float64 beside the three
launches it replaces; the grid shared over the batch; guard rows, canaries and the status word; a graph; the model route
behind VQ_FINAL_QUANT_FUSED.

Observed e_new / e_pair (max-abs errors against float64, one MI355X run): 1.000 in all 14 cases, every one bit-identical to
the three launches; e_pair itself 4.7e-4 .. 4.9e-3.  The tiny PixArt's route: 2.414e-4 both ways (W8A8), 1.055e-3 (W4A8).
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from helpers import load_npz, quant_params_of, trace_ops
from test_final_layer_gpu import bound

pytestmark = pytest.mark.gpu
CN = [(96, 16), (1152, 32), (1536, 64)]        # (C, N_out): a masked tail step with Kp = 128; the flagship; the widest
BR = [(1, 1), (1, 17), (2, 9), (4, 5), (2, 520)]  # (B, rows per sample): lone row, ragged tiles of 16 / 8 / 4 tokens, 65 tiles


def exact_case(C, N, B, R, w_bits, n_bits):
    """scale = -1 makes xm = shift whatever the LayerNorm gives; shift = integer codes x 2^-1 with 0 and qmax in every
    sample: delta = 2^-1, zp = 0, the codes are those integers; weight = integers x 2 around per-channel zero points at
    mid-range, so that the int8 images are small and every term of ring_dequant's fp32 form (sx sw acc, U P, V Q: the
    entry point dequantises as the GEMM does) is an integer below 2^24 - at most 1536 x 128 x 6 - hence exact."""
    g = torch.Generator().manual_seed(7 * C + 100 * R + B + w_bits + n_bits)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    qmax = 2 ** n_bits - 1
    codes = ri(0, 3, B, C)
    codes[:, 0], codes[:, 1] = 0, qmax
    wi, zw = ri(-2, 2, N, C), ((128 if w_bits == 8 else 2) + torch.arange(N) % 3).float()
    return dict(x=(torch.randn(B, R, C, generator=g) * 2 + 1).half(), shift=codes * 0.5, scale=-torch.ones(B, C),
                w=(wi * 2).half(), wd=torch.full((N,), 2.0), wz=zw, b=ri(-8, 8, N))


def run(ops, dev, d, w_bits, n_bits=8, s=None, status=None):
    g = {k: v.to(dev) for k, v in d.items()}
    s = None if s is None else s.to(dev)
    pw = ops.pack_weight(g["w"], g["wd"], g["wz"], w_bits, s=s)
    return ops.final_layer_i8(g["x"], g["shift"], g["scale"], 1e-6, pw, g["b"], s, n_bits, status), pw, g


EXACT = [(c, n, b, r, w, 8) for c, n in CN for b, r in BR for w in (8, 4)] + [(1152, 32, 2, 9, 8, 6)]


@pytest.mark.parametrize("C,N,B,R,w_bits,n_bits", EXACT)
def test_exact_family(ops, dev, C, N, B, R, w_bits, n_bits):
    d = exact_case(C, N, B, R, w_bits, n_bits)
    want = d["shift"].double() @ d["w"].double().T + d["b"].double()                    # [B, N], the same for every row
    assert torch.equal(want, want.round()) and float(want.abs().max()) < 2048
    out = run(ops, dev, d, w_bits, n_bits)[0].cpu()
    assert torch.equal(out.double(), want[:, None, :].expand(B, R, N))


def make(C, N, B, R, w_bits, smooth):
    g = torch.Generator().manual_seed(1000 * C + 10 * R + B)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = dict(x=(r(B, R, C) * 1.5 + 0.3).half(), shift=r(B, C) * 0.3, scale=r(B, C) * 0.3, w=(r(N, C) / C ** 0.5).half(),
             b=r(N) * 0.1)
    s = (r(C).abs() * 0.5 + 0.5) if smooth else None
    v = d["w"].float() * (1.0 if s is None else s)                                      # the packer's fp32 arithmetic
    lo, hi = v.min(1)[0].clamp(max=0), v.max(1)[0].clamp(min=0)
    d["wd"] = (hi - lo) / (2 ** w_bits - 1)
    d["wz"] = torch.round(-lo / d["wd"])
    wdeq = (torch.clamp(torch.round(v / d["wd"][:, None]) + d["wz"][:, None], 0, 2 ** w_bits - 1) - d["wz"][:, None]).double() \
        * d["wd"][:, None].double()
    return d, s, wdeq


def reference(x, shift, scale, s, wdeq, bias, n_bits=8, eps=1e-6):
    """float64 from the fp16 inputs: LayerNorm, modulate, round to fp16, / s, the grid shared over the batch, codes, Linear."""
    from oracle.fakequant import quant_codes, token_params
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    y = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    xm = (y * (1 + scale.double()[:, None]) + shift.double()[:, None]).half().double()
    q = (xm if s is None else xm / s.double()).float()
    delta, zp, _ = token_params(q, n_bits)
    deq = (quant_codes(q, delta, zp, n_bits).double() - zp.double()) * delta.double()
    return deq @ wdeq.T + bias.double()


GRID = [(c, n, b, r) for c, n in CN for b, r in BR if (c, r) != (1536, 520)]


@pytest.mark.parametrize("i", range(len(GRID)))
def test_against_float64_beside_the_three_launches(ops, dev, i):
    (C, N, B, R), smooth = GRID[i], bool(i % 2)
    w_bits = 4 if smooth else 8
    d, s, wdeq = make(C, N, B, R, w_bits, smooth)
    ref = reference(d["x"], d["shift"], d["scale"], s, wdeq, d["b"])
    new, pw, g = run(ops, dev, d, w_bits, s=s)
    xm = ops.ln_modulate_rowquant(g["x"], g["shift"], g["scale"], 1e-6, want_xm=True)[1]
    pair = ops.gemm_i8(ops.rowquant(xm, n_bits=8, s=None if s is None else s.to(dev)), pw, g["b"]).reshape(B, R, N)
    pair, new = pair.cpu().double(), new.cpu().double()
    assert new.shape == ref.shape and bool(torch.isfinite(new).all())
    e_pair, e_new = float((pair - ref).abs().max()), float((new - ref).abs().max())
    print("final_layer_i8 C %d N %d B %d R %d W%d smooth %d: e_pair %.3e e_new %.3e ratio %.3f bit-equal %s"
          % (C, N, B, R, w_bits, smooth, e_pair, e_new, e_new / max(e_pair, 1e-30), torch.equal(pair, new)))
    assert e_new <= bound(e_pair, ref), (e_new, e_pair)


@pytest.mark.parametrize("C,N,R", [(96, 16, 9), (1152, 32, 17)])
def test_shared_grid_and_own_sample_vectors(ops, dev, C, N, R):
    d = make(C, N, 2, R, 8, False)[0]
    d["shift"][1] = float("nan")                            # sample 1 is NaN; sample 0 meets it only through the shared grid
    assert bool(torch.isfinite(run(ops, dev, d, 8)[0][0]).all())
    for k in ("x", "shift", "scale"):
        d[k][1] = d[k][0]
    one = dict(d, x=d["x"][:1], shift=d["shift"][:1], scale=d["scale"][:1])
    two = run(ops, dev, d, 8)[0]
    assert torch.equal(two[0], two[1]) and torch.equal(two[:1], run(ops, dev, one, 8)[0])


@pytest.mark.parametrize("C,N,B,R", [(96, 16, 1, 17), (1152, 32, 2, 9)])
def test_guard_rows_canaries_and_status(ops, dev, C, N, B, R):
    from viditq_amd import _lib
    d = make(C, N, B, R, 8, False)[0]
    want, pw, g = run(ops, dev, d, 8)
    M, p = B * R, lambda t: t.data_ptr()  # noqa: E731
    xbuf = torch.full((M + 16, C), float("nan"), dtype=torch.float16, device=dev)
    xbuf[:M] = g["x"].reshape(M, C)
    status = ops.new_status(dev)

    def raw(x, shift, scale):
        out = torch.full((M + 16, N), 7.0, dtype=torch.float16, device=dev)
        rc = _lib.load().vq_final_layer_i8(p(x), p(shift), p(scale), 1e-6, None, None, p(pw.wq), p(pw.sw), p(pw.zw), p(pw.cs),
                                           p(g["b"]), p(out), p(status), M, R, C, pw.Kp, N, C, 8, 8,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and bool((out[M:] == 7.0).all())
        return out[:M]
    assert torch.equal(raw(xbuf, g["shift"], g["scale"]), want.reshape(M, N)) and int(status.item()) == 0
    xbuf[:M] = torch.arange(M, device=dev, dtype=torch.float16)[:, None]               # every row constant: xm = 0, delta = 0
    raw(xbuf, torch.zeros_like(g["shift"]), -torch.ones_like(g["scale"]))
    assert int(status.item()) == 1


def test_graph_replays_equal_the_eager_call(ops, dev):
    d, s, _ = make(1152, 32, 2, 17, 4, True)
    g = {k: v.to(dev) for k, v in d.items()}
    s = s.to(dev)
    pw = ops.pack_weight(g["w"], g["wd"], g["wz"], 4, s=s)
    call = lambda: ops.final_layer_i8(g["x"], g["shift"], g["scale"], 1e-6, pw, g["b"], s)  # noqa: E731
    eager = call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def route_child(name, w_bits):
    """(started with VQ_FINAL_QUANT_FUSED=1) the tiny PixArt's patch-major forward, switch as found and cleared, each traced"""
    from test_parity_gpu import _cfgs, _load_qp, _pixart
    from viditq_amd import ops
    from viditq_amd.t2v import stdit
    dev = torch.device("cuda:0")
    g = load_npz(name)
    wq, aq = _cfgs(w_bits, T=1, S=64, **(dict(smooth=dict(alpha=0.3), mixed_precision=[4, 6, 8]) if w_bits == 4 else {}))
    qnn = _pixart("PixArtMS", g, dev, wq, aq)
    if w_bits == 4:
        qnn.set_smooth_quant(smooth_quant=False, smooth_quant_running_stat=False)
    _load_qp(qnn, quant_params_of(g, "qp_after_ptq" if w_bits == 4 else "qp"))
    x, y, mask = g["x"].to(dev), g["y"].half().to(dev), g["mask"].to(dev)
    t = g["t"].to(dev) if "t" in g else torch.tensor([820, 820], device=dev)
    seen, fwd, fused = {}, stdit.T2IFinalLayer.forward, ops.final_layer_i8

    def spy(self, x, t):
        seen.update(x=x.cpu(), t=t.cpu(), table=self.scale_shift_table.cpu(), layer=self.linear)
        return fwd(self, x, t)
    stdit.T2IFinalLayer.forward = spy
    res = {"switch": stdit._FINAL_QUANT_FUSED}
    with torch.no_grad():
        for key, on in (("on", stdit._FINAL_QUANT_FUSED), ("off", False)):
            stdit._FINAL_QUANT_FUSED, n = on, []
            ops.final_layer_i8 = lambda *a, **k: (n.append(1), fused(*a, **k))[1]
            with trace_ops() as calls:
                out = qnn(x, t, y, mask=mask, patch_major=True).cpu().double()
            names = [c[0] for c in calls]
            last = len(names) - 1 - names[::-1].index("adaln_table")                   # final_layer's modulation table
            res[key] = {"fused": len(n), "tail": [c for c in names[last:] if c in ("ln_modulate_rowquant", "rowquant", "gemm_i8")],
                        "out": out.tolist()}
    layer = seen["layer"]
    wqz = layer.weight_quantizer
    W, dl, zp = layer.weight.detach().cpu().float(), wqz.delta.cpu().float().reshape(-1, 1), wqz.zero_point.cpu().float().reshape(-1, 1)
    wdeq = ((torch.clamp(torch.round(W / dl) + zp, 0, 2 ** wqz.n_bits - 1) - zp) * dl).double()
    tt = seen["t"].half().float()                                     # adaln_table: fp32 sums of the fp16 table and t
    res["ref"] = reference(seen["x"], seen["table"][0].float() + tt, seen["table"][1].float() + tt, None, wdeq,
                           layer.bias.detach().cpu()).tolist()
    print("ROUTE " + json.dumps(res))


@pytest.mark.parametrize("name,w_bits", [("tiny_pixart_w8a8.npz", 8), ("tiny_pixart_w4a8.npz", 4)])
def test_model_route_behind_the_switch(name, w_bits):
    """Switch set (a child process: it is read at import): one fused call, none of the three launches behind the last
    block; cleared: the three."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VQ_FINAL_QUANT_FUSED="1", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    p = subprocess.run([sys.executable, "-c", "import test_final_layer_i8_gpu as t; t.route_child(%r, %d)" % (name, w_bits)],
                       env=env, cwd=here, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROUTE ")][-1][6:])
    assert res["switch"] is True and res["on"]["fused"] == 1 and res["on"]["tail"] == []
    assert res["off"]["fused"] == 0 and res["off"]["tail"] == ["ln_modulate_rowquant", "rowquant", "gemm_i8"]
    ref, on, off = [torch.tensor(res[k] if k == "ref" else res[k]["out"], dtype=torch.float64) for k in ("ref", "on", "off")]
    e_pair, e_new = float((off - ref).abs().max()), float((on - ref).abs().max())
    print("route %s: e_pair %.3e e_new %.3e" % (name, e_pair, e_new))
    assert e_new <= bound(e_pair, ref), (e_new, e_pair)

"""ops.final_layer_f16 (vq_final_layer_f16, csrc/final_layer.hip) against float64 beside the two launches it replaces; each row
on its own sample's vectors; guard rows and canaries; the model route behind VQ_FINAL_FUSED; a graph.

Observed e_new / e_pair (max-abs errors against float64, one MI355X run): 1.000 in 19 of the 20 cases - bit-identical to the
pair in the 8 smallest, equal in error but not in every bit in the rest - and 1.001 at C 1536, N_out 64, B 2, 33 rows per
sample (9.772e-4 against 9.760e-4); e_pair itself 4.9e-4 .. 1.9e-3.  The tiny STDiT's route: 1.378e-4 both ways.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from helpers import load_npz, trace_ops

pytestmark = pytest.mark.gpu
CN = [(32, 16), (96, 32), (1152, 32), (1536, 64)]     # (C, N_out); the last: the widest, its weight read from global memory
BR = [(1, 1), (1, 17), (2, 15), (2, 33), (2, 1024)]     # (B, rows per sample): lone row, ragged tile, straddled tiles, 128 tiles


def make(C, N, B, R, seed=0):
    g = torch.Generator().manual_seed(1000 * C + 10 * R + B + seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=(r(B, R, C) * 1.5 + 0.3).half(), shift=r(B, C) * 0.3, scale=r(B, C) * 0.3, w=(r(N, C) / C ** 0.5).half(),
                b=(r(N) * 0.1).half())


def reference(d, eps=1e-6):
    """float64 from the fp16 inputs: LayerNorm, modulate, round to fp16, Linear."""
    x = d["x"].double()
    mu = x.mean(-1, keepdim=True)
    y = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    xm = (y * (1 + d["scale"].double()[:, None]) + d["shift"].double()[:, None]).half().double()
    return xm @ d["w"].double().T + d["b"].double()


def bound(e_pair, ref):                 # 1.5 x the two launches' own error + one fp16 ulp of the largest |reference| value
    top = float(ref.abs().max())
    return 1.5 * e_pair + 2.0 ** (max(torch.frexp(torch.tensor(top))[1].item() - 1, -14) - 10)


def both(ops, dev, d):
    g = {k: v.to(dev) for k, v in d.items()}
    xm = ops.ln_modulate_rowquant(g["x"], g["shift"], g["scale"], 1e-6, want_xm=True)[1]
    return ops.linear_f16(xm, g["w"], g["b"]), ops.final_layer_f16(g["x"], g["shift"], g["scale"], 1e-6, g["w"], g["b"])


@pytest.mark.parametrize("B,R", BR)
@pytest.mark.parametrize("C,N", CN)
def test_against_float64_beside_the_two_launches(ops, dev, C, N, B, R):
    d = make(C, N, B, R)
    ref = reference(d)
    pair, new = [o.cpu().double() for o in both(ops, dev, d)]
    assert new.shape == ref.shape and bool(torch.isfinite(new).all())
    e_pair, e_new = float((pair - ref).abs().max()), float((new - ref).abs().max())
    print("final_layer C %d N %d B %d R %d: e_pair %.3e e_new %.3e ratio %.3f bit-equal %s"
          % (C, N, B, R, e_pair, e_new, e_new / max(e_pair, 1e-30), torch.equal(pair, new)))
    assert e_new <= bound(e_pair, ref), (e_new, e_pair)


@pytest.mark.parametrize("C,N,R", [(96, 32, 15), (1152, 32, 33)])
def test_a_row_reads_its_own_samples_vectors(ops, dev, C, N, R):
    d = make(C, N, 2, R)
    clean = both(ops, dev, d)[1]
    d["shift"][1] = float("nan")
    out = both(ops, dev, d)[1]
    assert torch.equal(out[0], clean[0]) and bool(torch.isfinite(out[0]).all()) and bool(torch.isnan(out[1]).all())


@pytest.mark.parametrize("C,N,M,R", [(96, 32, 17, 17), (1152, 32, 66, 33)])
def test_guard_rows_and_canaries(ops, dev, C, N, M, R):
    from viditq_amd import _lib       # NaN rows behind row M of x change nothing; the rows behind out keep their canary
    d = make(C, N, M // R, R)
    g = {k: v.to(dev) for k, v in d.items()}
    xbuf = torch.full((M + 16, C), float("nan"), dtype=torch.float16, device=dev)
    xbuf[:M] = g["x"].reshape(M, C)
    out = torch.full((M + 16, N), 7.0, dtype=torch.float16, device=dev)
    rc = _lib.load().vq_final_layer_f16(xbuf.data_ptr(), g["shift"].data_ptr(), g["scale"].data_ptr(), 1e-6, g["w"].data_ptr(),
                                        g["b"].data_ptr(), out.data_ptr(), M, R, C, N, C, C,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and torch.equal(out[:M], both(ops, dev, d)[1].reshape(M, N)) and bool((out[M:] == 7.0).all())


def test_graph_replays_equal_the_eager_call(ops, dev):
    g = {k: v.to(dev) for k, v in make(1152, 32, 2, 33).items()}
    call = lambda: ops.final_layer_f16(g["x"], g["shift"], g["scale"], 1e-6, g["w"], g["b"])  # noqa: E731
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


def route_child():
    """(started with VQ_FINAL_FUSED=1) the tiny STDiT's patch-major forward, switch as found and cleared, each traced"""
    from test_model_gpu import _build
    from viditq_amd import ops
    from viditq_amd.t2v import stdit
    dev = torch.device("cuda:0")
    g = load_npz("tiny_stdit_w8a8.npz")
    qnn = _build(g, dev, 8)
    args = (g["x"].to(dev), torch.tensor([500.0], device=dev), g["y"].half().to(dev)[:1])
    seen, fwd, fused = {}, stdit.T2IFinalLayer.forward, ops.final_layer_f16

    def spy(self, x, t):
        seen.update(x=x.cpu(), t=t.cpu(), table=self.scale_shift_table.cpu(), w=self.linear.org_weight.cpu(),
                    b=self.linear.org_bias.cpu())
        return fwd(self, x, t)
    stdit.T2IFinalLayer.forward = spy
    res = {"switch": stdit._FINAL_FUSED}
    with torch.no_grad():
        for key, on in (("on", stdit._FINAL_FUSED), ("off", False)):
            stdit._FINAL_FUSED, n = on, []
            ops.final_layer_f16 = lambda *a, **k: (n.append(1), fused(*a, **k))[1]
            with trace_ops() as calls:
                out = qnn(*args, mask=g["mask"].to(dev), patch_major=True).cpu().double()
            tail = [c for c in calls if (c[0] == "ln_modulate_rowquant" and c[1]["want_xm"]) or
                    (c[0] == "linear_f16" and c[1]["w"][1] == list(seen["w"].shape))]
            res[key] = {"fused": len(n), "pair": [c[0] for c in tail], "out": out.tolist()}
    tt = seen["t"].half().float()                                     # adaln_table: fp32 sums of the fp16 table and t
    res["ref"] = reference(dict(x=seen["x"], shift=seen["table"][0].float() + tt, scale=seen["table"][1].float() + tt,
                                w=seen["w"], b=seen["b"])).tolist()
    print("ROUTE " + json.dumps(res))


def test_model_route_behind_the_switch():
    """Switch set (a child process: it is read at import): one fused call, neither launch of the pair; cleared: the pair."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VQ_FINAL_FUSED="1", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    p = subprocess.run([sys.executable, "-c", "import test_final_layer_gpu as t; t.route_child()"], env=env, cwd=here,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROUTE ")][-1][6:])
    assert res["switch"] is True and res["on"]["fused"] == 1 and res["on"]["pair"] == []
    assert res["off"]["fused"] == 0 and res["off"]["pair"] == ["ln_modulate_rowquant", "linear_f16"]
    ref, on, off = [torch.tensor(res[k] if k == "ref" else res[k]["out"], dtype=torch.float64) for k in ("ref", "on", "off")]
    e_pair, e_new = float((off - ref).abs().max()), float((on - ref).abs().max())
    assert e_new <= bound(e_pair, ref), (e_new, e_pair)

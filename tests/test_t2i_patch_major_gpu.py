"""The three PixArt sampler steps on final_layer's patch-major output (vq_cfg_{dpmpp,ddpm,sa}_step_patch2d) on the GPU:
bit for bit the dense entry points on unpatchify(eps), no worse than them against fp64, blind to what they must not read,
nothing written outside the outputs; and the fused loops and step graphs of the tiny PixArt under VQ_T2I_PATCH_MAJOR=1."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddpm_step_cases as pc
import dpm_step_cases as dc
import sa_step_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, CO, GUARD, MARK = 4, 8, 64, 777.0
# (n, H, W, p, eps offset in elements): one token row; non-square; an address only on its own element (the one-element form);
# several workgroups and strips; p = 1
GEOS = [(1, 4, 4, 2, 0), (2, 4, 12, 2, 0), (1, 6, 6, 2, 1), (2, 64, 64, 2, 0), (1, 4, 4, 1, 0)]


def unpatchify(e, H, W, p):
    e = e.reshape(e.shape[0], H // p, W // p, p, p, -1)
    return torch.einsum("nhwpqc->nchpwq", e).reshape(e.shape[0], -1, H, W).contiguous()     # (p = 1: reshape is a view)


@functools.lru_cache(maxsize=None)
def _rows(kind):
    """[(table, k, guided)]: one row per solver order (dpmpp: 1, 2, 3 and 'taylor'; sa: every row of a 6-step table, whose
    corrector / predictor orders run through 0 - 2); ddpm: clip off / on, the last row, guided and unguided."""
    def table(k, row):
        t = np.zeros((k + 1, 16), dtype=np.float32)
        t[k] = row
        return torch.from_numpy(t)
    if kind == "dpmpp":
        first = {}
        for _, k, row, _ in dc.d2_rows():
            first.setdefault((row[dc.ORDER], row[dc.TAYLOR]), (table(k, row), k, None))
        return list(first.values())
    if kind == "ddpm":
        r = pc.p2_rows()
        return [(table(0, r[0][2]), 0, 3), (table(0, r[5][2]), 0, 3), (table(0, r[3][2]), 0, 0)]
    return [(table(k, row), k, None) for _, k, row in sc.p2_rows(6)]


def _guarded(t):
    """A copy of ``t`` between two guard regions: (the view, its buffer)."""
    buf = torch.full((t.numel() + 2 * GUARD,), MARK, dtype=t.dtype, device=t.device)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
    return buf[GUARD:GUARD + t.numel()].view(t.shape), buf


def _launch(ops, kind, patch, eps, inp, rows, k, guided, counter):
    """One step on guarded copies of the operands: {name: (output, its buffer)}."""
    t = {name: _guarded(v) for name, v in inp.items()}
    xm = _guarded(torch.zeros((2 * inp["x"].shape[0],) + tuple(inp["x"].shape[1:]), dtype=torch.float16, device=eps.device))
    kw = dict(step=torch.tensor([k], dtype=torch.int32, device=eps.device), row=0) if counter else dict(row=k)
    kw.update(x_out=t["x"][0], x_model=xm[0])
    sfx = "_patch2d" if patch else ""
    if kind == "dpmpp":
        getattr(ops, "cfg_dpmpp_step" + sfx)(eps, t["x"][0], t["hist"][0], rows, **kw)
    elif kind == "ddpm":
        t["x0"] = _guarded(torch.zeros_like(inp["x"]))
        getattr(ops, "cfg_ddpm_step" + sfx)(eps, t["x"][0], t["noise"][0], rows, x0_out=t["x0"][0], guided=guided, **kw)
    else:
        getattr(ops, "cfg_sa_step" + sfx)(eps, t["x"][0], t["xp"][0], t["hist"][0], t["noise"][0], rows, xp_out=t["xp"][0],
                                          **kw)
    return dict(t, xm=xm)


def _fp64(kind, row, dense, inp, k, guided):
    """x_out of the header's formulas in float64 (the case files' expression trees, nothing rounded)."""
    f = lambda v: v.double().cpu().numpy()   # noqa: E731
    n = inp["x"].shape[0]
    x = f(inp["x"]).reshape(n, C, -1)
    e = f(dense).reshape(2 * n, dense.shape[1], -1)
    ident = lambda v: v   # noqa: E731
    row = row.astype(np.float64)
    if kind == "dpmpp":
        h = f(inp["hist"])
        return dc._tree(row, e[:n], e[n:], x, h[(k - 1) % 3].reshape(x.shape), h[(k - 2) % 3].reshape(x.shape), ident, ident,
                        "reciprocal")[0]
    if kind == "ddpm":
        P = pc._tree(row, e[:n, :C], e[n:, :C], e[:n, C:], x, guided, ident, ident)
        return P["mean"] + row[pc.NONZERO] * np.exp(P["h"]) * f(inp["noise"]).reshape(x.shape)
    h, z = f(inp["hist"]), f(inp["noise"])
    return sc._tree(row, e[:n], e[n:], x, f(inp["xp"]).reshape(x.shape), h[(k - 1) % 2].reshape(x.shape),
                    z[k % 2].reshape(x.shape), z[(k + 1) % 2].reshape(x.shape), ident, ident)[0]


@pytest.mark.parametrize("pad", [0, 24], ids=["dense", "padded"])
@pytest.mark.parametrize("half", [True, False], ids=["fp16eps", "fp32eps"])
@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "n%d_%dx%d_p%d_off%d" % g)
@pytest.mark.parametrize("kind", ["dpmpp", "ddpm", "sa"])
def test_patch2d_step_is_the_dense_step_on_the_unpatchified_output(ops, dev, kind, geo, half, pad):
    n, H, W, p, off = geo
    tok, cols, total = (H // p) * (W // p), p * p * CO, n * C * H * W
    g = lambda shape, seed, s=1.0: torch.from_numpy(dc.gauss(shape, seed, s)).to(dev)   # noqa: E731
    clean = g((2 * n, tok, cols), 1).view(2 * n, tok, p * p, CO)
    clean[..., C:] *= 0.4                                    # the variance channels of IDDPM: (v + 1) / 2 around 1 / 2
    clean = clean.view(2 * n, tok, cols).to(torch.float16 if half else torch.float32)
    # what no kernel may read: the pitch padding, what lies in front of eps, and the learned-sigma channels - of both halves
    # for dpmpp / sa, of the uncond half (the second) for ddpm
    ld = tok * cols + pad
    store = torch.full((off + 2 * n * ld,), float("nan"), dtype=clean.dtype, device=dev)
    eps = store[off:].view(2 * n, ld)[:, :tok * cols].view(2 * n, tok, p * p, CO)
    eps.copy_(clean.view(2 * n, tok, p * p, CO))
    eps[n if kind == "ddpm" else 0:, :, :, C:] = float("nan")
    eps = eps.view(2 * n, tok, cols)
    assert getattr(ops, "cfg_%s_step_patch2d_ok" % kind)(eps, torch.empty(n, C, H, W, device=dev))
    dense = unpatchify(clean, H, W, p)
    dense = dense if kind == "ddpm" else dense[:, :C]
    inp = dict(x=g((n, C, H, W), 2))
    if kind == "dpmpp":
        inp["hist"] = g((3, total), 3)
    elif kind == "ddpm":
        inp["noise"] = g((n, C, H, W), 4)
    else:
        inp.update(xp=g((n, C, H, W), 5), hist=g((2, total), 3), noise=g((2, total), 4))
    cases = _rows(kind)
    for j, (rows, k, guided) in enumerate(cases):
        rows = rows.to(dev)
        want = _launch(ops, kind, False, dense, inp, rows, k, guided, False)
        got = _launch(ops, kind, True, eps, inp, rows, k, guided, counter=j == len(cases) - 1)
        for name in want:
            a, b = got[name][1], want[name][1]
            # 1. every output bit for bit, 3. with NaN wherever the kernel must not read, 4. guards untouched (both
            # buffers carry the same guards, so one comparison of the whole buffers says all three)
            assert torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                               b.view(torch.int16 if b.dtype == torch.float16 else torch.int32)), (name, k)
            assert bool((a[:GUARD] == MARK).all()) and bool((a[-GUARD:] == MARK).all()), (name, k)
            assert bool(torch.isfinite(a).all()), (name, k)
        if not half:                                         # 2. against fp64: no worse than the dense kernel
            ref = _fp64(kind, rows[k].cpu().numpy(), dense, inp, k, guided).reshape(n, C, H, W)
            err = [float(np.abs(v["x"][0].double().cpu().numpy() - ref).max()) for v in (got, want)]
            print(kind, geo, k, "max |x_out - fp64|: patch2d %.3e dense %.3e" % tuple(err))
            assert err[0] <= err[1]


CHILD = r"""
import json, sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import ddpm_step_cases as pc
from test_dpm_step_gpu import _tiny_pixart
import viditq_amd
from viditq_amd import ops
from viditq_amd.t2i import fused_loop
from viditq_amd.t2i.dpm_solver import DPMS_sigma
from viditq_amd.t2i.sa_solver import SASolver
kind, dev = %r, "cuda"
calls = {}
def count(name):
    orig = getattr(ops, name)
    def f(*a, **k):
        calls[name] = calls.get(name, 0) + 1
        return orig(*a, **k)
    setattr(ops, name, f)
for name in ("cfg_%%s_step" %% kind, "cfg_%%s_step_patch2d" %% kind):
    count(name)
g, qnn = _tiny_pixart(dev)
z = g["dpm_z"].to(dev)
cond, null, mask = g["y"][:1].half().to(dev), g["dpm_null_y"].half().to(dev), g["mask"][:1].to(dev)
def run(graph):
    seen = []
    if kind == "dpmpp":
        s = DPMS_sigma(qnn.forward_with_dpmsolver, condition=cond, uncondition=null, cfg_scale=4.5,
                       model_kwargs=dict(data_info=None, mask=mask))
        s.model_input_dtype = torch.float16
        cb = lambda i, v: seen.append(v.clone())
        out = s.step_graph(z, steps=5, order=2).run(z, step_callback=cb) if graph else \
            s.sample(z, steps=5, order=2, fused=True, step_callback=cb)
    elif kind == "ddpm":
        s = pc.make_sampler("10")
        z2 = z.float().repeat(2, 1, 1, 1)
        kw = dict(y=torch.cat([cond, null]), cfg_scale=4.5, data_info=None, mask=mask)
        noise = torch.randn((10,) + tuple(z2.shape), generator=torch.Generator().manual_seed(5)).to(dev)
        cb = lambda i, v, x0: seen.extend([v.clone(), x0.clone()])
        out = s.p_sample_graph(qnn.forward_with_cfg, z2, False, kw).run(z2, noise_steps=noise, step_callback=cb) if graph \
            else s.p_sample_loop(qnn.forward_with_cfg, tuple(z2.shape), z2, clip_denoised=False, model_kwargs=kw,
                                 noise_steps=noise, fused=True, step_callback=cb)
    else:
        s = SASolver(qnn.forward_with_dpmsolver, cond, null, 4.5, dict(data_info=None, mask=mask))
        tau = lambda t: 1 if 0.2 <= t <= 0.8 else 0
        noise = torch.randn((9,) + tuple(z.shape), generator=torch.Generator().manual_seed(5)).to(dev)
        if graph:
            out = s.step_graph(z, tau, 8).run(z, noise_steps=noise)
        else:
            out, seen = s.sample("few_steps", z, tau, 8, predictor_order=2, corrector_order=2, return_intermediate=True,
                                 noise_steps=noise, fused=True)
    return [out] + list(seen)
assert fused_loop._T2I_PATCH_MAJOR
on, on_graph = run(False), run(True)
n_on = dict(calls)
fused_loop._T2I_PATCH_MAJOR = False
calls.clear()
off, off_graph = run(False), run(True)
same = lambda a, b: len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
print("PATCH2D", json.dumps([n_on, calls, len(on), same(on, off), same(on_graph, off_graph), same(on_graph[:1], on[:1])]))
"""


@pytest.mark.parametrize("kind,steps", [("dpmpp", 5), ("ddpm", 10), ("sa", 8)])
def test_tiny_pixart_loop_and_graph_under_the_switch(dev, kind, steps):
    """VQ_T2I_PATCH_MAJOR=1 at import: the fused loop of the tiny PixArt and its step graph run forward(patch_major=True) and
    the patch2d step only (the graph's launches: its warm-up passes and the capture), and every step's sample equals, bit
    for bit, the one of the same loop and graph with the switch off, which launch the dense step only."""
    env = dict(os.environ, VQ_T2I_PATCH_MAJOR="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), kind)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PATCH2D")][-1]
    n_on, n_off, n_seen, loop_same, graph_same, graph_is_loop = json.loads(line[len("PATCH2D"):])
    dense, patch = "cfg_%s_step" % kind, "cfg_%s_step_patch2d" % kind
    assert set(n_on) == {patch} and n_on[patch] > steps and set(n_off) == {dense} and n_off[dense] == n_on[patch]
    assert n_seen > 1 and loop_same and graph_same and graph_is_loop, line

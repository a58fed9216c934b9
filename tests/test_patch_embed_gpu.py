"""ops.patch_embed_f16 (csrc/patch_embed.hip): bit for bit the launches it replaces (patchify copy, cast, ops.linear_f16, torch's
fp16 "+ pos") and those against float64; the index map alone; isolation and guard rows; a graph; the routes behind the switch."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from helpers import load_npz, state_dict_of, trace_ops

pytestmark = pytest.mark.gpu
# (B, Cin, latent dims, patch, C, pos_rows); the grid is 2 workgroups per CU: only the last two (1125, 604 tiles) walk the loop
CASES = {
    "one_token": (1, 4, (2, 2), (2, 2), 16, 1),                  # waves without a channel group
    "straddle": (2, 4, (6, 10), (2, 2), 96, 15),                 # 15 tokens per sample, uneven channel split
    "frames": (2, 4, (3, 4, 6), (1, 2, 2), 96, 6),               # n % pos_rows across frames
    "k32_2d": (1, 8, (4, 6), (2, 2), 32, 6),
    "k32_3d": (1, 4, (4, 4, 6), (2, 2, 2), 48, 6),               # and a last group of 16 channels
    "k8": (1, 2, (4, 4), (2, 2), 32, 4),
    "pw_odd": (1, 4, (4, 6), (2, 1), 32, 12),                    # K = 8; the gather without paired loads
    "c1152": (1, 4, (6, 22), (2, 2), 1152, 33),
    "c1536": (1, 4, (6, 22), (2, 2), 1536, 33),
    "rows2048": (2, 4, (64, 64), (2, 2), 1152, 1024),
    "walk_2d": (2, 4, (180, 200), (2, 2), 96, 9000),
    "walk_3d": (1, 4, (20, 42, 46), (1, 2, 2), 48, 483),
}


def make(dev, name, f32=True, bias=True, pos=True):
    B, Cin, dims, patch, C, P = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    K = Cin * int(torch.tensor(patch).prod())
    x, w, b, pe = [torch.randn(*sh, generator=g) for sh in ((B, Cin) + dims, (C, K), (C,), (P, C))]
    return dict(x=(x if f32 else x.half()).to(dev), w=(w / K ** 0.5).half().to(dev), b=(b * 0.1).half().to(dev) if bias else None,
                pos=pe.half().to(dev) if pos else None, patch=patch)


def fused(ops, d):
    return ops.patch_embed_f16(d["x"], d["w"], d["b"], d["pos"], d["patch"])


def three(v):
    return (1,) * (3 - len(v)) + tuple(v)


def patchify(x, patch):
    """[B, N, K]: tokens row-major over the patch grid, k in the flatten order of the Conv weight."""
    x5 = x if x.dim() == 5 else x[:, :, None]
    pt, ph, pw = three(patch)
    B, Cin, D, H, W = x5.shape
    xp = x5.reshape(B, Cin, D // pt, pt, H // ph, ph, W // pw, pw).permute(0, 2, 4, 6, 1, 3, 5, 7)
    return xp.reshape(B, -1, Cin * pt * ph * pw)


def add_pos(a, pos):
    return a if pos is None else (a.reshape(a.shape[0], -1, pos.shape[0], a.shape[2]) + pos).reshape(a.shape)


def pair(ops, d):
    """Today's route: the patchified fp16 copy through ops.linear_f16, then torch's fp16 add of pos[n % P]."""
    return add_pos(ops.linear_f16(patchify(d["x"], d["patch"]).half().contiguous(), d["w"], d["b"]), d["pos"])


def float64(d):
    a = patchify(d["x"], d["patch"]).half().double() @ d["w"].double().T
    return add_pos(a if d["b"] is None else a + d["b"].double(), None if d["pos"] is None else d["pos"].double())


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("name,bias,pos", [(n, True, True) for n in CASES] + [("straddle", False, False), ("c1152", False, False)])
def test_bit_equal_to_the_launches_it_replaces_and_those_against_float64(ops, dev, name, bias, pos, f32):
    d = make(dev, name, f32, bias, pos)
    new, old, ref = fused(ops, d), pair(ops, d), float64(d)
    rel = float((old.double() - ref).norm() / ref.norm())
    print("patch_embed %s f32 %s: pair rel-L2 to float64 %.3e" % (name, f32, rel))
    assert new.dtype == torch.float16 and torch.equal(new, old) and rel <= 1e-3      # the project's per-layer bound (README.md)


@pytest.mark.parametrize("B,Cin,dims,patch", [(2, 4, (8, 16), (2, 2)), (1, 4, (2, 8, 8), (1, 2, 2)), (1, 2, (4, 8, 16), (2, 2, 2)), (2, 4, (8, 16), (2, 1))])
def test_index_map_with_a_one_hot_weight(ops, dev, B, Cin, dims, patch):
    x = torch.randperm(B * Cin * int(torch.tensor(dims).prod()), generator=torch.Generator().manual_seed(3)) + 1.0
    x = x.reshape(B, Cin, *dims)                                  # distinct integers <= 2048: exact in fp16
    (pt, ph, pw), (D, H, W) = three(patch), three(dims)
    K, Hp, Wp = Cin * pt * ph * pw, H // ph, W // pw
    out = ops.patch_embed_f16(x.to(dev), torch.eye(32, K, dtype=torch.float16, device=dev), patch=patch).cpu()      # w[k, k] = 1
    n, k = torch.arange((D // pt) * Hp * Wp)[:, None], torch.arange(K)[None, :]
    t, i, j = n // (Hp * Wp), n // Wp % Hp, n % Wp
    ci, dt, dh, dw = k // (pt * ph * pw), k // (ph * pw) % pt, k // pw % ph, k % pw
    want = x.reshape(B, Cin, D, H, W)[:, ci, t * pt + dt, i * ph + dh, j * pw + dw]
    assert torch.equal(out[:, :, :K].float(), want) and bool((out[:, :, K:] == 0).all())


@pytest.mark.parametrize("name", ["straddle", "frames", "c1152"])
def test_samples_unused_pos_rows_and_the_rows_behind_out_are_isolated(ops, dev, name):
    from viditq_amd import _lib       # NaN rows behind row pos_rows of pos change nothing; the rows behind out keep their canary
    d = make(dev, name)
    B, Cin, dims, patch, C, P = CASES[name]
    want = fused(ops, d)
    M = want.numel() // C
    pos = torch.cat([d["pos"], torch.full((4, C), float("nan"), dtype=torch.float16, device=dev)])
    out = torch.full((M + 16, C), 7.0, dtype=torch.float16, device=dev)
    (pt, ph, pw), (D, H, W) = three(patch), three(dims)
    rc = _lib.load().vq_patch_embed_f16(d["x"].data_ptr(), 1, d["w"].data_ptr(), d["b"].data_ptr(), pos.data_ptr(), out.data_ptr(),
                                        B, Cin, D, H, W, pt, ph, pw, C, P, d["w"].stride(0),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and torch.equal(out[:M], want.reshape(M, C)) and bool((out[M:] == 7.0).all())
    if B == 2:                        # NaN in sample 1's latent: sample 0's rows keep their bits
        d["x"][1] = float("nan")
        bad = fused(ops, d)
        assert torch.equal(bad[0], want[0]) and bool(torch.isfinite(bad[0]).all()) and bool(torch.isnan(bad[1]).all())


def test_graph_replays_equal_the_eager_call(ops, dev):
    d = make(dev, "c1152")
    eager = fused(ops, d)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fused(ops, d)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def route_child():
    """(started with VQ_PATCH_EMBED_FUSED=1) the tiny STDiT's forward, switch as found and cleared; PixArtMS's embedder stage"""
    from test_model_gpu import _build
    from viditq_amd import ops
    from viditq_amd.t2i import PixArtMS, pixart
    from viditq_amd.t2v import stdit
    dev = torch.device("cuda:0")
    real, n = ops.patch_embed_f16, []
    ops.patch_embed_f16 = lambda *a, **k: (n.append(1), real(*a, **k))[1]      # (trace_ops sees ops.py's own functions)
    res = {"switch": stdit._PATCH_EMBED_FUSED}
    g = load_npz("tiny_stdit_w8a8.npz")
    qnn = _build(g, dev, 8)
    args = (g["x"].to(dev), torch.tensor([500.0], device=dev), g["y"].half().to(dev)[:1])
    with torch.no_grad():
        for key, sw in (("on", stdit._PATCH_EMBED_FUSED), ("off", False)):
            stdit._PATCH_EMBED_FUSED = sw
            del n[:]
            with trace_ops() as calls:
                out = qnn(*args, mask=g["mask"].to(dev))
            emb = [c for c in calls if c[0] == "linear_f16" and c[1]["w"][1] == [64, 16]]
            res[key] = {"fused": len(n), "linear": len(emb), "out": out.cpu().double().tolist()}
        stdit._PATCH_EMBED_FUSED = res["switch"]
        g = load_npz("tiny_pixart_w8a8.npz")
        m = PixArtMS(input_size=16, depth=2, hidden_size=64, num_heads=4, model_max_length=12, caption_channels=32, dtype=torch.float16)
        m.load_state_dict(state_dict_of(g), strict=True)
        m = m.half().to(dev).eval()
        seen, run = {}, pixart._PixArtBase._run_blocks
        pixart._PixArtBase._run_blocks = lambda self, x, *a: (seen.update(x=x.clone()), run(self, x, *a))[1]
        del n[:]
        x = g["x"].to(dev)
        m(x, g["t"].to(dev), g["y"].half().to(dev), mask=g["mask"].to(dev))
        w, b = m.x_embedder.proj.weight.detach().reshape(64, -1), m.x_embedder.proj.bias.detach()
        d = dict(x=x, w=w, b=b, patch=(2, 2), pos=m._pos_embed(dev, torch.float16)[0])
        res["pixart"] = {"fused": len(n), "equal": torch.equal(seen["x"], pair(ops, d))}
    print("ROUTE " + json.dumps(res))


def test_model_routes_behind_the_switch(dev):         # a child process: the switch is read at import
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VQ_PATCH_EMBED_FUSED="1", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    p = subprocess.run([sys.executable, "-c", "import test_patch_embed_gpu as t; t.route_child()"], env=env, cwd=here,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROUTE ")][-1][6:])
    assert res["switch"] is True and res["on"]["fused"] == 1 and res["on"]["linear"] == 0 and res["pixart"] == {"fused": 1, "equal": True}
    assert res["off"]["fused"] == 0 and res["off"]["linear"] == 1 and res["on"]["out"] == res["off"]["out"]

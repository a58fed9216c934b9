"""PixArt-Sigma key / value compression between the qkv GEMM and the attention: the one HIP launch (ops.kv_compress) against
the torch sequence of AttentionKVCompress.attend it replaces (the q copy, the q / k LayerNorms, permutes, the depthwise
conv2d, the LayerNorm, casts), on q | k | v buffers of the released shapes (GPU only).

    B in (1, 2) x (64 x 64, 128 x 128) tokens, C = 1152, sr = 2: 'conv', 'conv' + qk_norm, 'uniform'

Captured graphs replayed, the buffer rotated so that no launch finds its rows in L2 / MALL, the two routes alternated
--alternate times in one process after a warm-up of both, best against best.  The device copy rate comes from the same
process.  Bytes are the algorithm's: k and v read once ('uniform': the picked quarter of them), k' and v' written once, q
read and written once under qk_norm.

    python tools/kv_compress_time.py [--alternate 3] [--out profiles/kv_compress/times.json]

Exit status 1 when the HIP launch is slower than the torch sequence at any shape.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa: E402,F401
from static_quant_time import graph_time  # noqa: E402
from viditq_amd import ops  # noqa: E402
from viditq_amd.t2i.pixart import AttentionKVCompress  # noqa: E402

C, HEADS, SR = 1152, 16, 2
SHAPES = [(B, g, samp, qk) for B in (1, 2) for g in (64, 128) for samp, qk in (("conv", False), ("conv", True), ("uniform", False))]


def one(dev, B, grid, samp, qk, alternate):
    N = grid * grid
    attn = AttentionKVCompress(C, HEADS, sampling=samp, sr_ratio=SR, qk_norm=qk).half().to(dev).eval()
    for p in attn.parameters():                              # not the average-pool / identity initialisation
        p.data.add_(0.05 * torch.randn_like(p))
    n_buf = max(2, min(12, (1 << 30) // (B * N * 3 * C * 2)))
    bufs = [(torch.randn(B * N, 3 * C, device=dev) + 2.0).half() for _ in range(n_buf)]
    i = [0]

    def qkv():
        i[0] = (i[0] + 1) % n_buf
        return bufs[i[0]]

    def old():                                               # AttentionKVCompress.attend up to ops.attn_fwd
        x = qkv()
        q3 = attn._norm_fp32(attn.q_norm, x[:, :C].reshape(B, N, C)).contiguous()
        k3 = attn.downsample_2d(attn._norm_fp32(attn.k_norm, x[:, C:2 * C].reshape(B, N, C)), grid, grid).contiguous()
        v3 = attn.downsample_2d(x[:, 2 * C:].reshape(B, N, C), grid, grid).contiguous()
        return q3, k3, v3

    f32 = attn._param_f32
    ln3 = lambda ln: None if isinstance(ln, torch.nn.Identity) else (f32(ln.weight), f32(ln.bias), ln.eps)
    conv = samp == "conv"
    par = (f32(attn.sr.weight), f32(attn.sr.bias), ln3(attn.norm)) if conv else (None, None, None)
    assert ops.kv_compress_ok(C, grid, grid, SR, samp, 3 * C)

    def new():
        return ops.kv_compress(qkv(), B, grid, grid, C, SR, samp, *par, ln3(attn.k_norm), ln3(attn.q_norm))

    n = 8
    rows = B * N
    rows_in = rows if conv or qk else rows // SR ** 2            # k rows read (all of them under k_norm)
    mb = ((rows_in + (rows if conv else rows // SR ** 2)) * C * 2 + 2 * (rows // SR ** 2) * C * 2 + (2 * rows * C * 2 if qk else 0)) / 1e6
    keep = [graph_time(old, n=n)[1], graph_time(new, n=n)[1]]                # warm-up of both routes
    t_old, t_new = [], []
    for _ in range(alternate):
        t_old.append(graph_time(old, n=n)[0])
        t_new.append(graph_time(new, n=n)[0])
    del keep
    ba, bb = min(t_old), min(t_new)
    name = "B %d, %3d x %3d, %s%s" % (B, grid, grid, samp, " + qk_norm" if qk else "")
    print("%-34s torch %s -> best %.1f us | HIP %s -> best %.1f us (%.2f TB/s of %.1f MB) | %s" % (
        name, ["%.1f" % t for t in t_old], ba, ["%.1f" % t for t in t_new], bb, mb / bb, mb,
        "not slower" if bb <= ba else "SLOWER"), flush=True)
    return dict(shape=name, MB=round(mb, 1), torch_us=[round(t, 1) for t in t_old], hip_us=[round(t, 1) for t in t_new],
                torch_best_us=round(ba, 1), hip_best_us=round(bb, 1), hip_TBps=round(mb / bb, 2), not_slower=bb <= ba)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--alternate", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kv_compress_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src = torch.empty(16384 * 4608, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)
    copy_us, _ = graph_time(lambda: dst.copy_(src), n=8, reps=8)
    copy_tbs = 2 * src.numel() * 2 / copy_us / 1e6
    del src, dst
    print("device copy: %.1f us = %.2f TB/s" % (copy_us, copy_tbs), flush=True)
    try:
        mhz = torch.cuda.clock_rate()                        # the shader clock the driver reports, MHz (when it can be read)
    except Exception as e:  # noqa: BLE001
        mhz = "not read (%s)" % type(e).__name__
    rec = dict(device=torch.cuda.get_device_name(0), clock_mhz=mhz, copy_us=round(copy_us, 1), copy_TBps=round(copy_tbs, 2), shapes=[])
    with torch.no_grad():
        for B, grid, samp, qk in SHAPES:
            rec["shapes"].append(one(dev, B, grid, samp, qk, args.alternate))
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(rec, f, indent=1)
    return 0 if all(r["not_slower"] for r in rec["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())

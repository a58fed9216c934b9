"""Temporal attention + attn_temp.proj's static tensor-wise quantizer: the two-launch route (attn_temporal /
attn_temporal_long, then vq_rowquant on the static grid) against the fused entry point
vq_attn_temporal_rowquant_static, at the STDiT-XL/2 shapes (GPU only).

Captured graphs replayed, q | k | v rotated over 12 buffers so that no launch finds its input in L2 / MALL, the two
routes alternated three times in one process after a warm-up, best of three against best of three.  The device copy
rate comes from the same process.  Bytes are the algorithm's: the fused route reads rows * 3 C * 2 and writes rows * Kp;
the two-launch route also writes and reads the fp16 attention output (rows * C * 2 each way).

    python tools/static_attn_quant_time.py [--out profiles/static_quant/attn_fused.json]

Exit status 1 when the fused route is slower than the two-launch route at any shape.
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

H, D, S = 16, 72, 1024
C = H * D
# (B, T, n_bits)
SHAPES = [(1, 16, 8), (1, 16, 6), (2, 16, 8), (2, 16, 6), (1, 64, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("static_attn_quant_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src = torch.empty(16384 * 4608, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)
    copy_us, _ = graph_time(lambda: dst.copy_(src), n=8, reps=8)
    copy_tbs = 2 * src.numel() * 2 / copy_us / 1e6
    del src, dst
    print("device copy: %.1f us = %.2f TB/s" % (copy_us, copy_tbs))
    rows_out = []
    for B, T, n_bits in SHAPES:
        rows = B * T * S
        bufs = [torch.randn(rows, 3 * C, device=dev).half() for _ in range(12)]
        i = [0]

        def qkv():
            i[0] = (i[0] + 1) % len(bufs)
            return bufs[i[0]]
        o = torch.empty(rows, C, dtype=torch.float16, device=dev)
        # a grid that covers the attention output of Gaussian inputs (|o| < 1 mostly)
        qmax = 2 ** n_bits - 1
        delta = torch.tensor([2.0 / qmax], device=dev)
        zp = torch.tensor([float(round(qmax / 2))], device=dev)

        def two():
            x = qkv()
            if T <= 16:
                ops.attn_temporal(x, x[:, C:], x[:, 2 * C:], o, B, T, S, H, D, 3 * C, C)
            else:
                ops.attn_temporal_long(x, x[:, C:], x[:, 2 * C:], B, T, S, H, D, 3 * C, o=o)
            return ops.rowquant(o.view(B, T * S, C), n_bits=n_bits, delta=delta, zp=zp)

        def fused():
            x = qkv()
            return ops.attn_temporal_rowquant_static(x, x[:, C:], x[:, 2 * C:], B, T, S, H, D, 3 * C, delta, zp, n_bits=n_bits)

        n = 24 if T <= 16 else 8
        mb_fused = rows * (3 * C * 2 + C) / 1e6
        mb_two = mb_fused + 2 * rows * C * 2 / 1e6
        t_two, t_fused = [], []
        keep = [graph_time(two, n=n)[1], graph_time(fused, n=n)[1]]          # warm-up of both routes
        for _ in range(3):
            t_two.append(graph_time(two, n=n)[0])
            t_fused.append(graph_time(fused, n=n)[0])
        del keep
        ba, bb = min(t_two), min(t_fused)
        name = "B=%d T=%d S=%d H=%d D=%d, %d bits" % (B, T, S, H, D, n_bits)
        rows_out.append(dict(shape=name, two_launch_MB=round(mb_two, 1), fused_MB=round(mb_fused, 1),
                             two_launch_us=[round(t, 1) for t in t_two], fused_us=[round(t, 1) for t in t_fused],
                             two_launch_best_us=round(ba, 1), fused_best_us=round(bb, 1), fused_TBps=round(mb_fused / bb, 2),
                             not_slower=bb <= ba))
        print("%-36s two launches %s -> best %.1f us | fused %s -> best %.1f us (%.2f TB/s of %.1f MB) | %s" % (
            name, ["%.1f" % t for t in t_two], ba, ["%.1f" % t for t in t_fused], bb, mb_fused / bb, mb_fused,
            "not slower" if bb <= ba else "SLOWER"), flush=True)
        del bufs
        torch.cuda.empty_cache()
    rec = dict(device=torch.cuda.get_device_name(0), copy_us=round(copy_us, 1), copy_TBps=round(copy_tbs, 2), shapes=rows_out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if all(r["not_slower"] for r in rows_out) else 1


if __name__ == "__main__":
    sys.exit(main())

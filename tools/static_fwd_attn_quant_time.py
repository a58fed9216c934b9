"""Spatial / cross attention + proj's static tensor-wise quantizer: the two-launch route (vq_attn_fwd, then vq_rowquant
on the static grid) against the fused entry point vq_attn_fwd_rowquant_static, at the STDiT-XL/2 and PixArt-alpha 512^2
shapes (GPU only).

Captured graphs replayed, the inputs rotated over 12 buffers so that no launch finds its input in L2 / MALL, the two
routes alternated three times in one process after a warm-up, best of three against best of three.  The device copy
rate comes from the same process.  Bytes are the algorithm's: the fused route reads q, k, v and writes rows * Kp codes;
the two-launch route also writes and reads the fp16 attention output (rows * C * 2 each way).

    python tools/static_fwd_attn_quant_time.py [--out profiles/static_quant/attn_fwd_fused.json]

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

H, D = 16, 72
C = H * D
PROMPT = 120
# (name, kind, n_seq, Lq): spatial = self-attention over L tokens of a q | k | v buffer; cross = Lq queries per sample over
# PROMPT prompt tokens per sample (packed by offsets, known bound)
LAUNCHES = [("STDiT spatial 16 x 1024", "spatial", 16, 1024), ("STDiT spatial 32 x 1024 (cond | uncond)", "spatial", 32, 1024),
            ("STDiT cross 1 x 16384 over 120", "cross", 1, 16384), ("STDiT cross 2 x 16384 over 120", "cross", 2, 16384),
            ("PixArt-alpha 512^2 self 2 x 1024", "spatial", 2, 1024), ("PixArt-alpha 512^2 cross 2 x 1024 over 120", "cross", 2, 1024)]
BITS = (8, 6)
NBUF = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("static_fwd_attn_quant_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src = torch.empty(16384 * 4608, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)
    copy_us, _ = graph_time(lambda: dst.copy_(src), n=8, reps=8)
    copy_tbs = 2 * src.numel() * 2 / copy_us / 1e6
    del src, dst
    print("device copy: %.1f us = %.2f TB/s" % (copy_us, copy_tbs))
    rows_out = []
    for name, kind, n_seq, Lq in LAUNCHES:
        rows = n_seq * Lq
        if kind == "spatial":
            bufs = [torch.randn(rows, 3 * C, device=dev).half() for _ in range(NBUF)]
            kvs, off, Lk = None, None, Lq
            mb_in = rows * 3 * C * 2 / 1e6
        else:
            bufs = [torch.randn(rows, C, device=dev).half() for _ in range(NBUF)]
            kvs = [torch.randn(n_seq * PROMPT, 2 * C, device=dev).half() for _ in range(NBUF)]
            off = torch.arange(n_seq + 1, dtype=torch.int32, device=dev) * PROMPT
            Lk = PROMPT
            mb_in = (rows * C * 2 + n_seq * PROMPT * 2 * C * 2) / 1e6
        i = [0]

        def launch_args():
            """(q, k, v, n_seq, Lq, Lk, H, D, q_seq, q_tok, kv_seq, kv_tok) of the next rotated input"""
            i[0] = (i[0] + 1) % NBUF
            x = bufs[i[0]]
            if kind == "spatial":
                return x, x[:, C:], x[:, 2 * C:], n_seq, Lq, Lk, H, D, Lq * 3 * C, 3 * C, Lq * 3 * C, 3 * C
            kv = kvs[i[0]]
            return x, kv, kv[:, C:], n_seq, Lq, Lk, H, D, Lq * C, C, 0, 2 * C
        o = torch.empty(rows, C, dtype=torch.float16, device=dev)
        for n_bits in BITS:
            # a grid that covers the attention output of Gaussian inputs (|o| < 1 mostly)
            qmax = 2 ** n_bits - 1
            delta = torch.tensor([2.0 / qmax], device=dev)
            zp = torch.tensor([float(round(qmax / 2))], device=dev)
            assert ops.attn_fwd_static_ok(n_seq, Lq, Lk, H, D, 3 * C if kind == "spatial" else C, 3 * C if kind == "spatial" else 2 * C,
                                          C, n_bits, kv_off=off is not None)

            def two():
                a = launch_args()
                ops.attn_fwd(*a[:3], o, *a[3:], Lq * C, C, kv_off=off)
                return ops.rowquant(o.view(1, rows, C), n_bits=n_bits, delta=delta, zp=zp)

            def fused():
                a = launch_args()
                return ops.attn_fwd_rowquant_static(*a, delta, zp, n_bits=n_bits, kv_off=off)

            n = 24 if rows <= 4096 else 12
            mb_fused = mb_in + rows * C / 1e6
            mb_two = mb_fused + 2 * rows * C * 2 / 1e6
            t_two, t_fused = [], []
            keep = [graph_time(two, n=n)[1], graph_time(fused, n=n)[1]]          # warm-up of both routes
            for _ in range(3):
                t_two.append(graph_time(two, n=n)[0])
                t_fused.append(graph_time(fused, n=n)[0])
            del keep
            ba, bb = min(t_two), min(t_fused)
            label = "%s, %d bits" % (name, n_bits)
            rows_out.append(dict(shape=label, two_launch_MB=round(mb_two, 1), fused_MB=round(mb_fused, 1),
                                 two_launch_us=[round(t, 1) for t in t_two], fused_us=[round(t, 1) for t in t_fused],
                                 two_launch_best_us=round(ba, 1), fused_best_us=round(bb, 1), not_slower=bb <= ba))
            print("%-52s two launches %s -> best %.1f us | fused %s -> best %.1f us | %s" % (
                label, ["%.1f" % t for t in t_two], ba, ["%.1f" % t for t in t_fused], bb,
                "not slower" if bb <= ba else "SLOWER"), flush=True)
            if args.out:                                   # (written after every row: a partial table survives a time limit)
                rec = dict(device=torch.cuda.get_device_name(0), copy_us=round(copy_us, 1), copy_TBps=round(copy_tbs, 2),
                           shapes=rows_out)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(rec, f, indent=1)
        del bufs, kvs
        torch.cuda.empty_cache()
    return 0 if all(r["not_slower"] for r in rows_out) else 1


if __name__ == "__main__":
    sys.exit(main())

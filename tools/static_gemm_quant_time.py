"""mlp.fc1 + GELU + mlp.fc2's static tensor-wise quantizer: the two-launch route (vq_gemm_i8 with the GELU epilogue, then
vq_rowquant on the static grid) against the fused entry point vq_gemm_i8_rowquant_static, at the fc1 shapes of STDiT-XL/2
and PixArt (GPU only).

Captured graphs replayed, the activation codes rotated over 12 buffers so that no launch finds its input in L2 / MALL
(the 5.3 MB weight stays, as it does in a step), the two routes alternated three times in one process after a warm-up,
best of three against best of three.  The device copy rate comes from the same process.  Bytes are the algorithm's: the
fused route reads M K + N K and writes M Kp_out codes and 12 M bytes of row terms; the two-launch route also writes and
reads the fp16 activation (M N 2 each way).  Two sections: without and with a smoothing vector on fc2.

    python tools/static_gemm_quant_time.py [--out profiles/static_quant/gemm_fused.json]

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

N, K = 4608, 1152
ROWS = [16384, 32768, 2048, 8192]
# n_bits -> (delta, zp): grids on which both clamps of a GELU output of standard deviation ~2 act
GRIDS = {8: (2.0 ** -6, 64.0), 6: (2.0 ** -5, 16.0)}


def operands(M, bits, dev):
    """12 activations of random codes and one weight whose pre-activation has a standard deviation of about 2."""
    a = (2.0 / (58.0 * 58.0 * K ** 0.5)) ** 0.5
    acts = []
    for _ in range(12):
        xs = torch.randint(-100, 101, (M, K), dtype=torch.int8, device=dev)
        zx = torch.randint(-6, 7, (M,), dtype=torch.int32, device=dev)
        sx = (a * (0.8 + 0.4 * torch.rand(M, device=dev))).float()
        acts.append(ops.QAct(xs, sx, zx, (xs.int().sum(1) - K * zx).int(), K, 8))
    ws = torch.randint(-100, 101, (N, K), dtype=torch.int8, device=dev)
    zw = torch.randint(-6, 7, (N,), dtype=torch.int32, device=dev)
    sw = (a * (0.8 + 0.4 * torch.rand(N, device=dev))).float()
    pw = ops.PackedWeight(ws, sw, zw, ws.int().sum(1).int(), N, K, K, bits)
    bias = (torch.randn(N, device=dev) * 0.3).float()
    return acts, pw, bias


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("static_gemm_quant_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src = torch.empty(16384 * 4608, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)
    copy_us, _ = graph_time(lambda: dst.copy_(src), n=8, reps=8)
    copy_tbs = 2 * src.numel() * 2 / copy_us / 1e6
    del src, dst
    print("device copy: %.1f us = %.2f TB/s" % (copy_us, copy_tbs))
    smooth = torch.exp(torch.randn(N, device=dev) * 0.6).float()
    assert ops.smooth_rcp(smooth) is not None
    rows_out = []
    for s in (None, smooth):
        for M in ROWS:
            for bits in (8, 6):
                acts, pw, bias = operands(M, bits, dev)
                i = [0]

                def act():
                    i[0] = (i[0] + 1) % len(acts)
                    return acts[i[0]]
                delta = torch.tensor([GRIDS[bits][0]], device=dev)
                zp = torch.tensor([GRIDS[bits][1]], device=dev)

                def two():
                    h = ops.gemm_i8(act(), pw, bias=bias, epilogue=ops.EPI_GELU)
                    return ops.rowquant(h.view(1, M, N), n_bits=bits, delta=delta, zp=zp, s=s)

                def fused():
                    return ops.gemm_i8_rowquant_static(act(), pw, bias, delta, zp, bits, s=s)

                ref = two()
                got = ops.gemm_i8_rowquant_static(acts[i[0]], pw, bias, delta, zp, bits, s=s)      # the same input
                assert all(torch.equal(getattr(ref, f), getattr(got, f)) for f in ("xq", "sx", "zx", "R")), "routes disagree"
                n = 24 if M <= 16384 else 12
                mb_fused = (M * K + N * K + M * ops.pad128(N) + 12 * M) / 1e6
                mb_two = mb_fused + 2 * M * N * 2 / 1e6
                t_two, t_fused = [], []
                keep = [graph_time(two, n=n)[1], graph_time(fused, n=n)[1]]          # warm-up of both routes
                for _ in range(3):
                    t_two.append(graph_time(two, n=n)[0])
                    t_fused.append(graph_time(fused, n=n)[0])
                del keep
                ba, bb = min(t_two), min(t_fused)
                name = "%d x %d x %d, %d bits%s" % (M, N, K, bits, ", smoothed" if s is not None else "")
                rows_out.append(dict(shape=name, two_launch_MB=round(mb_two, 1), fused_MB=round(mb_fused, 1),
                                     two_launch_us=[round(t, 1) for t in t_two], fused_us=[round(t, 1) for t in t_fused],
                                     two_launch_best_us=round(ba, 1), fused_best_us=round(bb, 1), not_slower=bb <= ba))
                print("%-40s two launches %s -> best %.1f us | fused %s -> best %.1f us | %s" % (
                    name, ["%.1f" % t for t in t_two], ba, ["%.1f" % t for t in t_fused], bb,
                    "not slower" if bb <= ba else "SLOWER"), flush=True)
                del acts, pw
                torch.cuda.empty_cache()
    rec = dict(device=torch.cuda.get_device_name(0), copy_us=round(copy_us, 1), copy_TBps=round(copy_tbs, 2), shapes=rows_out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if all(r["not_slower"] for r in rows_out) else 1


if __name__ == "__main__":
    sys.exit(main())

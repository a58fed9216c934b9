"""T2IFinalLayer on the fp16 GPU route: the one HIP launch (ops.final_layer_f16) against the two launches it replaces
(ops.ln_modulate_rowquant taken for its fp16 by-product, then ops.linear_f16), on token matrices of the released shapes
(GPU only).

    (M, C, N_out) = (16384, 1152, 32), (32768, 1152, 32), (4096, 1152, 32), (1024, 1152, 32); one sample (B = 1)

Captured graphs replayed, the token matrix rotated so that no launch finds its rows in L2 / MALL, the two routes alternated
--alternate times in one process after a warm-up of both, best against best and alternation by alternation.  The device
copy rate comes from the same process.  Bytes are the algorithm's: x read once, out written once, the weight and the two
modulation vectors once.

    python tools/final_layer_time.py [--alternate 3] [--out profiles/final_layer/times.json]

--i8: the quantized arm instead - the one launch of ops.final_layer_i8 against the three it replaces
(ops.ln_modulate_rowquant for xm, ops.rowquant, ops.gemm_i8) at M = B x rows in {1024, 4096, 8192, 16384}, C 1152 -> 32,
for the joint forward B = 2, 8-bit and 4-bit weights, measured the same way.

Exit status 1 when the one launch is slower than the pair at any shape in any alternation (the flip criterion of
DESIGN.md section 8).
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

SHAPES = [(16384, 1152, 32), (32768, 1152, 32), (4096, 1152, 32), (1024, 1152, 32)]
SHAPES_I8 = [(1024, 1152, 32), (4096, 1152, 32), (8192, 1152, 32), (16384, 1152, 32)]


def rotating(dev, B, M, C):
    """x(): the next of enough [B, M / B, C] token matrices that no launch finds its rows in L2 / MALL"""
    n_buf = max(2, min(12, (1 << 30) // (M * C * 2)))
    bufs = [(torch.randn(B, M // B, C, device=dev) * 1.5 + 0.3).half() for _ in range(n_buf)]
    i = [0]

    def x():
        i[0] = (i[0] + 1) % n_buf
        return bufs[i[0]]
    return x


def one(dev, M, C, N, alternate):
    x = rotating(dev, 1, M, C)
    shift, scale = [torch.randn(1, C, device=dev) * 0.3 for _ in range(2)]
    w, b = (torch.randn(N, C, device=dev) / C ** 0.5).half(), (torch.randn(N, device=dev) * 0.1).half()

    def old():
        return ops.linear_f16(ops.ln_modulate_rowquant(x(), shift, scale, 1e-6, want_xm=True)[1], w, b)

    assert ops.final_layer_f16_ok(M, M, C, N, C, C)

    def new():
        return ops.final_layer_f16(x(), shift, scale, 1e-6, w, b)

    mb = (M * C * 2 + M * N * 2 + N * C * 2 + 2 * C * 4) / 1e6
    return alternations("M %5d, C %d, N_out %d" % (M, C, N), mb, old, new, alternate)


def one_i8(dev, M, C, N, w_bits, alternate, B=2):
    x = rotating(dev, B, M, C)
    shift, scale = [torch.randn(B, C, device=dev) * 0.3 for _ in range(2)]
    w, b = (torch.randn(N, C, device=dev) / C ** 0.5).half(), torch.randn(N, device=dev) * 0.1
    pw = ops.pack_weight(w, *ops.weight_minmax(w, w_bits), w_bits)

    def old():
        xm = ops.ln_modulate_rowquant(x(), shift, scale, 1e-6, want_xm=True)[1]
        return ops.gemm_i8(ops.rowquant(xm, n_bits=8), pw, b)

    assert ops.final_layer_i8_ok(M, M // B, C, pw.Kp, N, C, 8, w_bits)

    def new():
        return ops.final_layer_i8(x(), shift, scale, 1e-6, pw, b)

    mb = (M * C * 2 + M * N * 2 + pw.wq.numel() + 2 * B * C * 4) / 1e6
    return alternations("M %5d, C %d, N_out %d, B %d, W%d" % (M, C, N, B, w_bits), mb, old, new, alternate)


def alternations(name, mb, old, new, alternate):
    n = 8
    keep = [graph_time(old, n=n)[1], graph_time(new, n=n)[1]]                # warm-up of both routes
    t_old, t_new = [], []
    for _ in range(alternate):
        t_old.append(graph_time(old, n=n)[0])
        t_new.append(graph_time(new, n=n)[0])
    del keep
    ba, bb = min(t_old), min(t_new)
    ok = all(tn <= to for to, tn in zip(t_old, t_new))
    print("%-34s parent launches %s -> best %.1f us | one launch %s -> best %.1f us (%.2f TB/s of %.1f MB) | %s" % (
        name, ["%.1f" % t for t in t_old], ba, ["%.1f" % t for t in t_new], bb, mb / bb, mb, "not slower" if ok else "SLOWER"),
        flush=True)
    return dict(shape=name, MB=round(mb, 1), pair_us=[round(t, 1) for t in t_old], fused_us=[round(t, 1) for t in t_new],
                pair_best_us=round(ba, 1), fused_best_us=round(bb, 1), fused_TBps=round(mb / bb, 2), not_slower=ok)


def _read(what):
    try:
        return what()
    except Exception as e:  # noqa: BLE001
        return "not read (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--alternate", type=int, default=3)
    ap.add_argument("--i8", action="store_true", help="the quantized arm: ops.final_layer_i8 against its three launches")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("final_layer_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src = torch.empty(16384 * 4608, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)
    copy_us, _ = graph_time(lambda: dst.copy_(src), n=8, reps=8)
    copy_tbs = 2 * src.numel() * 2 / copy_us / 1e6
    del src, dst
    print("device copy: %.1f us = %.2f TB/s" % (copy_us, copy_tbs), flush=True)
    rec = dict(device=torch.cuda.get_device_name(0), clock_mhz=_read(torch.cuda.clock_rate), power_mw=_read(torch.cuda.power_draw),
               copy_us=round(copy_us, 1), copy_TBps=round(copy_tbs, 2), shapes=[])
    with torch.no_grad():
        runs = [(one_i8, (M, C, N, wb)) for wb in (8, 4) for M, C, N in SHAPES_I8] if args.i8 else [(one, s) for s in SHAPES]
        for fn, shape in runs:
            rec["shapes"].append(fn(dev, *shape, args.alternate))
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(rec, f, indent=1)
    rec["clock_mhz_after"], rec["power_mw_after"] = _read(torch.cuda.clock_rate), _read(torch.cuda.power_draw)
    print("clock %s -> %s MHz, power %s -> %s mW" % (rec["clock_mhz"], rec["clock_mhz_after"], rec["power_mw"], rec["power_mw_after"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if all(r["not_slower"] for r in rec["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())

"""The patch embedding on the fp16 GPU route: the one HIP launch (ops.patch_embed_f16) against the launches it replaces - the
lines of the forwards as they stand with VQ_PATCH_EMBED_FUSED unset: the latent's cast, the patchify copy, the Linear
(STDiT: ops.linear_f16; PixArt: F.linear, a hipBLASLt kernel) and torch's "+ pos_embed" - at the released shapes (GPU only).

    STDiT 16x64x64, B = 1 and B = 2 (patch (1, 2, 2), 16384 tokens per sample, pos [1024, 1152])
    PixArt 128x128 and 256x256 latents, B = 2 (patch (2, 2), 4096 / 16384 tokens per sample, pos [N, 1152])

fp32 latents (what the samplers hand over), C = 1152, Cin = 4.  Captured graphs replayed, the latent rotated, the two routes
alternated --alternate times in one process after a warm-up of both, best against best and alternation by alternation.  The
device copy rate comes from the same process.  Bytes are the algorithm's: the latent read once, out written once, the
weight, the bias and the position table once.

    python tools/patch_embed_time.py [--alternate 3] [--out profiles/patch_embed/times.json]

Exit status 1 when the one launch is slower than the launches it replaces at any shape in any alternation (the flip
criterion of DESIGN.md section 8, item 10e).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa: E402,F401
from final_layer_time import _read  # noqa: E402
from static_quant_time import graph_time  # noqa: E402
from viditq_amd import ops  # noqa: E402

C, CIN = 1152, 4
SHAPES = [("STDiT 16x64x64, B 1", "stdit", 1, (16, 64, 64), (1, 2, 2)), ("STDiT 16x64x64, B 2", "stdit", 2, (16, 64, 64), (1, 2, 2)),
          ("PixArt 128x128, B 2", "pixart", 2, (128, 128), (2, 2)), ("PixArt 256x256, B 2", "pixart", 2, (256, 256), (2, 2))]


def one(dev, name, model, B, dims, patch, alternate):
    pt, ph, pw = (1,) * (3 - len(patch)) + patch
    D, H, W = (1,) * (3 - len(dims)) + dims
    K, T, S = CIN * pt * ph * pw, D // pt, (H // ph) * (W // pw)
    N = T * S
    bufs = [torch.randn(B, CIN, *dims, device=dev) for _ in range(12)]
    w = (torch.randn(C, CIN, *patch, device=dev) / K ** 0.5).half()          # the Conv weight; w2 its matmul view
    w2, b, pos = w.reshape(C, -1), (torch.randn(C, device=dev) * 0.1).half(), torch.randn(1, S, C, device=dev).half()
    i = [0]

    def x():
        i[0] = (i[0] + 1) % len(bufs)
        return bufs[i[0]]

    def old(xv=None):                                         # t2v/stdit.py STDiT.forward / t2i/pixart.py PixArt(MS).forward
        xh = (x() if xv is None else xv).to(torch.float16)
        if model == "stdit":
            xp = xh.reshape(B, CIN, T, pt, H // ph, ph, W // pw, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B * N, K)
            o = ops.linear_f16(xp.to(w.dtype).contiguous(), w2, b).reshape(B, -1, C)
            return (o.reshape(B, T, S, C) + pos).reshape(B, N, C).contiguous()
        xp = xh.reshape(B, CIN, H // ph, ph, W // pw, pw).permute(0, 2, 4, 1, 3, 5).reshape(-1, K)
        return F.linear(xp.to(w.dtype), w2, b).reshape(B, -1, C) + pos

    assert ops.patch_embed_f16_ok(B, CIN, D, H, W, (pt, ph, pw), C, S, K)

    def new(xv=None):
        return ops.patch_embed_f16(x() if xv is None else xv, w2, b, pos, patch)

    same = torch.equal(old(bufs[0]), new(bufs[0]))          # (promised against linear_f16; against PixArt's vendor GEMM only observed)
    n = 8
    mb = (B * CIN * D * H * W * 4 + B * N * C * 2 + C * K * 2 + C * 2 + S * C * 2) / 1e6
    keep = [graph_time(old, n=n)[1], graph_time(new, n=n)[1]]                # warm-up of both routes
    t_old, t_new = [], []
    for _ in range(alternate):
        t_old.append(graph_time(old, n=n)[0])
        t_new.append(graph_time(new, n=n)[0])
    del keep
    ba, bb = min(t_old), min(t_new)
    ok = all(tn <= to for to, tn in zip(t_old, t_new))
    print("%-20s replaced %s -> best %.1f us | one launch %s -> best %.1f us (%.2f TB/s of %.1f MB) | bit-equal %s | %s" % (
        name, ["%.1f" % t for t in t_old], ba, ["%.1f" % t for t in t_new], bb, mb / bb, mb, same, "not slower" if ok else "SLOWER"),
        flush=True)
    return dict(shape=name, rows=B * N, MB=round(mb, 1), replaced_us=[round(t, 1) for t in t_old],
                fused_us=[round(t, 1) for t in t_new], replaced_best_us=round(ba, 1), fused_best_us=round(bb, 1),
                fused_TBps=round(mb / bb, 2), bit_equal=same, not_slower=ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--alternate", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("patch_embed_time.py needs a GPU: a CPU run gives no time")
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
        for shape in SHAPES:
            rec["shapes"].append(one(dev, *shape, args.alternate))
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

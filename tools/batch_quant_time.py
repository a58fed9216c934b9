"""The one-pass per-token quantizers of a batched forward (vq_rowquant_batch, 3 <= B <= 16) against the launches they replace,
arm by arm (GPU only).

    plain / smoothed x 3, C = 1152   today 1 or 3 x vq_rowquant(B): the generic two-pass rowquant_kernel
    LN x 1, LN x 3, C = 1152         today vq_ln_modulate_rowquant(B): the generic four-pass kernel; B = 16 has no parent
                                     (VQ_ESHAPE) and is reported against the copy probe alone
    GELU, plain, smoothed, C = 4608  today the fc1 GEMM's GELU epilogue (not timed: it rides on the GEMM) + vq_rowquant(B);
                                     plain / smoothed: vq_rowquant(B)

for B in (4, 8, 16) at 1024 and 4096 tokens.  Captured graphs replayed, the input rotated over enough buffers that no
launch finds its rows in L2 / MALL, the two routes alternated three times in one process after a warm-up.  The device copy
rate and the box's telemetry come from the same process.  Bytes are the algorithm's: rows * (2 C + G (Kp + 12)).

    python tools/batch_quant_time.py [--out profiles/batch_quant/times.json]

Exit status 1 when a one-pass launch is slower than what it replaces in any alternation (the flip criterion of DESIGN
section 8 item 8 (f)).
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
from t2v_dpm_time import copy_rates  # noqa: E402
from viditq_amd import ops  # noqa: E402

# (name, C, arm, outputs, smoothed)
ARMS = [("plain", 1152, "plain", 1, False), ("smoothed x 3", 1152, "plain", 3, True), ("LN x 1", 1152, "ln", 1, False),
        ("LN x 3", 1152, "ln", 3, True), ("GELU", 4608, "gelu", 1, False), ("plain", 4608, "plain", 1, False),
        ("smoothed", 4608, "plain", 1, True)]


def telemetry(dev):
    p = torch.cuda.get_device_properties(dev)
    return dict(device=p.name, cus=p.multi_processor_count, hbm_GiB=round(p.total_memory / 2 ** 30, 1), torch=torch.__version__,
                hip=torch.version.hip)


def measure(dev):
    out = []
    gen = torch.Generator().manual_seed(1)
    for B in (4, 8, 16):
        for n_tok in (1024, 4096):
            for name, C, arm, G, smoothed in ARMS:
                sv = [torch.exp(torch.randn(C, generator=gen) * 0.6).float().to(dev) if smoothed else None for _ in range(G)]
                assert all(s is None or ops.smooth_rcp(s) is not None for s in sv)
                shift, scale = [(torch.randn(B, C, generator=gen) * 0.3).float().to(dev) for _ in range(2)]
                assert ops.rowquant_batch_ok(B, C, ops.pad128(C), 8, G, int(arm == "gelu"), arm == "ln")
                nbuf = max(2, min(12, -(-(3 << 29) // (B * n_tok * C * 2))))        # 1.5 GB of rows in rotation
                bufs = [torch.randn(B, n_tok, C, device=dev).half() for _ in range(nbuf)]
                i = [0]

                def x():
                    i[0] = (i[0] + 1) % nbuf
                    return bufs[i[0]]

                def old():
                    if arm == "ln":
                        return ops.ln_modulate_rowquant(x(), shift, scale, 1e-6, smooth=sv, n_bits=8)
                    xx = x()
                    return [ops.rowquant(xx, n_bits=8, s=s) for s in sv]

                def new():
                    if arm == "ln":
                        return ops.ln_modulate_rowquant_batch(x(), shift, scale, 1e-6, sv, 8)
                    return ops.gelu_rowquant_batch(x(), 8, sv[0]) if arm == "gelu" else ops.rowquant_batch(x(), 8, sv)
                parent = not (arm == "ln" and B > 8)
                n = 12
                keep = [graph_time(f, n=n)[1] for f in ((old, new) if parent else (new,))]   # warm-up of both routes
                t_old, t_new = [], []
                for _ in range(3):
                    if parent:
                        t_old.append(graph_time(old, n=n)[0])
                    t_new.append(graph_time(new, n=n)[0])
                del keep, bufs
                mb = B * n_tok * (2 * C + G * (ops.pad128(C) + 12)) / 1e6
                ok = all(b <= a for a, b in zip(t_old, t_new))
                out.append(dict(B=B, n_tok=n_tok, C=C, arm=name, MB=round(mb, 1), today_us=[round(t, 1) for t in t_old],
                                one_pass_us=[round(t, 1) for t in t_new], one_pass_TBps=round(mb / min(t_new), 2),
                                not_slower=ok if parent else None))
                print("B %2d n %4d C %4d %-12s today %s | one pass %s (%.2f TB/s of %.1f MB) | %s" % (
                    B, n_tok, C, name, ["%.1f" % t for t in t_old] if parent else "no parent (VQ_ESHAPE)",
                    ["%.1f" % t for t in t_new], mb / min(t_new), mb, "not slower" if ok else "SLOWER"), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("batch_quant_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    res = dict(telemetry=telemetry(dev), copy=copy_rates(dev), rows=measure(dev))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(0 if all(r["not_slower"] is not False for r in res["rows"]) else 1)


if __name__ == "__main__":
    main()

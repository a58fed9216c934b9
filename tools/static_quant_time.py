"""Static-grid quantizers: the layerwise route (LayerNorm launch + one generic pass per Linear) against the one-pass
kernels of csrc/rowquant_static.hip, at the STDiT-XL/2 shapes (GPU only).

Captured graphs replayed (eager timing of these kernels measures the Python wrappers), inputs rotated over 12 buffers
so that no launch finds its input in L2 / MALL, the two routes alternated three times in one process after a warm-up,
best of three against best of three.  The device copy rate (a 151 MB fp16 buffer copied device to device) comes from
the same process.  Bytes are the algorithm's: rows * (2 C read + n_out * Kp written).

    python tools/static_quant_time.py [--out profiles/static_quant/kernels.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa: E402,F401
from viditq_amd import ops  # noqa: E402

M = 16384


def graph_time(fn, n=24, reps=12):
    """us per call of fn: n calls captured into one graph, replayed reps times after a warm replay phase"""
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(gr, stream=st):
            for _ in range(n):
                fn()
    for _ in range(10):
        gr.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (n * reps) * 1e3, gr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("static_quant_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    def rotating(C):
        bufs = [torch.randn(1, M, C, generator=g).half().to(dev) for _ in range(12)]
        i = [0]

        def nxt():
            i[0] = (i[0] + 1) % len(bufs)
            return bufs[i[0]]
        return nxt

    x1, x4 = rotating(1152), rotating(4608)
    sh = (torch.randn(1, 1152, generator=g) * 0.3).float().to(dev)
    sc = (torch.randn(1, 1152, generator=g) * 0.3).float().to(dev)
    tpe = (torch.randn(16, 1152, generator=g) * 0.5).half().to(dev)
    ds = [torch.tensor([d], device=dev) for d in (0.031, 0.027, 0.035)]
    zs = [torch.tensor([z], device=dev) for z in (128.0, 121.0, 133.0)]
    d4, z4 = torch.tensor([0.02], device=dev), torch.tensor([9.0], device=dev)

    def ln_old():
        _, xm = ops.ln_modulate_rowquant(x1(), sh, sc, 1e-6, smooth=[None], n_bits=8, want_xm=True)
        return [ops.rowquant(xm, delta=d, zp=z, want_zp=True) for d, z in zip(ds, zs)]    # want_zp: the generic kernel

    def add_old():
        x = x1()
        return [ops.rowquant(x, add_rows=tpe, add_div=M // 16, delta=d, zp=z, want_zp=True) for d, z in zip(ds, zs)]

    shapes = [
        ("LN + 3 outputs, 16384 x 1152", 94.4, ln_old,
         lambda: ops.rowquant_static(x1(), ds, zs, shift=sh, scale=sc, eps=1e-6)),
        ("add_rows + 3 outputs, 16384 x 1152", 94.4, add_old,
         lambda: ops.rowquant_static(x1(), ds, zs, add_rows=tpe, add_div=M // 16)),
        ("1 output, 16384 x 4608", 226.5, lambda: ops.rowquant(x4(), delta=d4, zp=z4, want_zp=True),
         lambda: ops.rowquant_static(x4(), [d4], [z4])),
    ]
    src = torch.empty(M * 4608, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)
    copy_us, _ = graph_time(lambda: dst.copy_(src), n=8, reps=8)
    copy_tbs = 2 * src.numel() * 2 / copy_us / 1e6
    print("device copy: %.1f us for 2 x %.0f MB = %.2f TB/s" % (copy_us, src.numel() * 2 / 1e6, copy_tbs))
    rows = []
    for name, mb, old, new in shapes:
        t_old, t_new = [], []
        keep = [graph_time(old)[1], graph_time(new)[1]]                      # warm-up of both routes
        for _ in range(3):
            t_old.append(graph_time(old)[0])
            t_new.append(graph_time(new)[0])
        del keep
        bo, bn = min(t_old), min(t_new)
        rows.append(dict(shape=name, model_MB=mb, layerwise_us=[round(t, 1) for t in t_old], one_pass_us=[round(t, 1) for t in t_new],
                         layerwise_best_us=round(bo, 1), one_pass_best_us=round(bn, 1), one_pass_TBps=round(mb / bn, 2),
                         not_slower=bn <= bo))
        print("%-36s layerwise %s -> best %.1f us | one pass %s -> best %.1f us (%.2f TB/s of %.1f MB) | %s" % (
            name, ["%.1f" % t for t in t_old], bo, ["%.1f" % t for t in t_new], bn, mb / bn, mb,
            "not slower" if bn <= bo else "SLOWER"))
    rec = dict(device=torch.cuda.get_device_name(0), rows_per_launch=M, copy_us=round(copy_us, 1), copy_TBps=round(copy_tbs, 2),
               shapes=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if all(r["not_slower"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())

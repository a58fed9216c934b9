"""64-frame temporal attention (OpenSORA 64x512x512) on the MI355X: what the long-video kernel buys.

  --kernel   A/B in one process at T = 64, S = 1024, H = 16, D = 72: the fused long kernel (attention + attn_temp.proj's
             8-bit per-token quantizer, one launch) vs the route the project had before it (the generic flash kernel
             over strided sequences, one launch per sample, then rowquant), alternated, device events; plus the box's
             copy rate measured in the same call.  Byte model of the fused call: q | k | v read once (453 MB) + codes
             (75.5 MB) + grids (0.8 MB).
  --step     denoising steps/s of W8A8 STDiT-XL/2 at 64x512x512, two chains replayed from one HIP graph as bench.py
             does it: the new route vs the fallback route (QuantAttention patched in-process), alternated.
  --trace    one eager 64-frame forward pair (depth --depth) for a `rocprofv3 --kernel-trace --stats` run.
  --fused-only N   N launches of the fused kernel alone, for `rocprofv3 --pmc` counter runs.
Prints one JSON line per mode."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

T, S, H, D = 64, 1024, 16, 72
C = H * D


def _events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernel_ab(reps, iters):
    from viditq_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(T * S, 3 * C, generator=g)).half().to(dev)
    out = torch.empty((T * S, C), dtype=torch.float16, device=dev)
    ld = qkv.stride(0)

    def fused():
        return ops.attn_temporal_long(qkv, qkv[:, C:], qkv[:, 2 * C:], 1, T, S, H, D, ld, quant=True)

    def fallback():
        ops.attn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], out, S, T, T, H, D, ld, S * ld, ld, S * ld, C, S * C)
        return ops.rowquant(out.view(1, T * S, C))
    # same codes on both routes up to fp16 rounding of the attention output
    a, b = fused(), fallback()
    torch.cuda.synchronize()
    agree = float((a.xq == b.xq).float().mean())
    src = torch.empty(453 * 2 ** 20 // 2, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        fused(), fallback(), dst.copy_(src)
    res = {"fused_us": [], "fallback_us": [], "copy_TBps": []}
    for _ in range(reps):
        res["fused_us"].append(1e3 * _events_ms(fused, iters))
        res["fallback_us"].append(1e3 * _events_ms(fallback, iters))
        ms = _events_ms(lambda: dst.copy_(src), iters)
        res["copy_TBps"].append(2 * src.numel() * 2 / (ms * 1e-3) / 1e12)
    model_bytes = T * S * 3 * C * 2 + T * S * C + T * S * 12
    best = min(res["fused_us"])
    res.update(mode="kernel", T=T, S=S, H=H, D=D, reps=reps, iters=iters, byte_model_MB=model_bytes / 1e6,
               fused_best_us=best, fused_TBps=model_bytes / (best * 1e-6) / 1e12,
               fallback_best_us=min(res["fallback_us"]), code_agreement=agree)
    return res


def fused_only(n):
    """n launches of the fused kernel alone (codes mode, full size): the process a counter run profiles."""
    from viditq_amd import ops
    dev = torch.device("cuda:0")
    qkv = torch.randn(T * S, 3 * C, generator=torch.Generator().manual_seed(0)).half().to(dev)
    for _ in range(n):
        ops.attn_temporal_long(qkv, qkv[:, C:], qkv[:, 2 * C:], 1, T, S, H, D, qkv.stride(0), quant=True)
    torch.cuda.synchronize()
    return {"mode": "fused_only", "launches": n}


def _model(depth):
    from viditq_amd import synth
    from viditq_amd.config import loads_yaml
    dev = torch.device("cuda:0")
    m = synth.build_stdit(dev, depth=depth, input_size=(T, 64, 64), time_scale=2 / 3)
    qnn = synth.quantize_model(m, loads_yaml(synth.W8A8_DYNAMIC))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    embeds, _ = synth.synthetic_prompts(1, dev)
    y = embeds["y"][0:1].permute(1, 0, 2, 3, 4).reshape(2, 1, 120, 4096)
    x = torch.randn(1, 4, T, 64, 64, generator=torch.Generator().manual_seed(0)).to(dev)
    return qnn, x, y[:1], y[1:], embeds["mask"][0:1]


class _Fallback:
    """The route before the long kernel: temporal attention through the generic flash kernel, quantizer separate."""

    def __enter__(self):
        from viditq_amd.qdiff.models.quant_block import QuantAttention
        self.cls = QuantAttention
        self.saved = (QuantAttention._long_ok, QuantAttention.temporal_quantized)
        orig_tq = QuantAttention.temporal_quantized
        QuantAttention._long_ok = lambda self, T_: False
        QuantAttention.temporal_quantized = lambda self, qkv, B, T_, S_, **k: None if T_ > 16 else orig_tq(self, qkv, B, T_, S_, **k)
        return self

    def __exit__(self, *exc):
        self.cls._long_ok, self.cls.temporal_quantized = self.saved


def step_ab(depth, reps, iters):
    from viditq_amd import graph
    qnn, x, yc, yu, mask = _model(depth)
    gs_new = graph.GraphedSampler(qnn, yc, yu, mask, two_streams=True)
    gs_new.forward_pair(x, 500)
    gs_old = graph.GraphedSampler(qnn, yc, yu, mask, two_streams=True)
    with _Fallback():
        gs_old.forward_pair(x, 500)                 # captured with the fallback route baked in
    c_new, u_new = [t.clone() for t in gs_new.forward_pair(x, 500)]
    c_old, u_old = [t.clone() for t in gs_old.forward_pair(x, 500)]
    rel = float((c_new.float() - c_old.float()).norm() / c_old.float().norm())
    res = {"new_steps_per_s": [], "fallback_steps_per_s": []}
    for _ in range(reps):
        res["new_steps_per_s"].append(1e3 / _events_ms(lambda: gs_new.forward_pair(x, 500), iters))
        res["fallback_steps_per_s"].append(1e3 / _events_ms(lambda: gs_old.forward_pair(x, 500), iters))
    res.update(mode="step", depth=depth, reps=reps, iters=iters, routes_rel_l2=rel,
               new_best=max(res["new_steps_per_s"]), fallback_best=max(res["fallback_steps_per_s"]))
    return res


def trace(depth):
    qnn, x, yc, yu, mask = _model(depth)
    t = torch.tensor([500], device=x.device)
    for _ in range(2):
        qnn(x, t, yc, mask=mask, timestep_id=500)
        qnn(x, t, yu, mask=mask, timestep_id=500)
    torch.cuda.synchronize()
    return {"mode": "trace", "depth": depth}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--fused-only", type=int, default=0, help="launch only the fused kernel this many times (counter runs)")
    ap.add_argument("--depth", type=int, default=28)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    import viditq_amd  # noqa: F401
    from viditq_amd import _lib
    _lib.load()
    t0 = time.time()
    lines = []
    with torch.no_grad():
        if a.kernel:
            lines.append(kernel_ab(a.reps, a.iters))
        if a.step:
            lines.append(step_ab(a.depth, a.reps, max(1, a.iters // 4)))
        if a.trace:
            lines.append(trace(a.depth))
        if a.fused_only:
            lines.append(fused_only(a.fused_only))
    for ln in lines:
        ln["wall_s"] = round(time.time() - t0, 1)
        s = json.dumps(ln)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()

"""What the STDiT DPM-Solver++ routes cost per model-call pair, against the graphed DDIM step (GPU box only):

    python tools/t2v_dpm_time.py [--depth 28] [--alternate 3] [--out FILE.json]

One STDiT-XL/2 (16 x 64 x 64 latent, W8A8 dynamic, cfg_split, one prompt) is built once; every arm is warmed up
(packing, caches, tables, graph captures) and then timed ``--alternate`` times in turn, in ONE process:
  ddim_graphed      IDDPM(100).ddim_sample_loop(graphed=True): ms per step.  Its captures are taken inside the call, so
                    the clock starts at the callback of the first step (after a synchronise) and covers the other 99.
  dpm_eager         DMP_SOLVER(20).sample(cfg_split=True, fused=False): ms per model-call pair
  dpm_fused         ... fused=True: forward(patch_major=True) x 2 + ops.cfg_dpmpp_step_patch, eager launches
  dpm_fused_graph   DMP_SOLVER(20).step_graph(...).run(z): one replay per model-call pair
Each reading is the host clock around the loop ending in a device synchronise (``started_s``: when it began).  Also reported: the spread (max - min) of
the ddim_graphed readings and 3 x that (the margin of the criterion in profiles/t2v_dpm_step/README.md), whether the four
DPM results are the same bits, the step kernel alone (event-timed launches on the loop's own buffers: us, the bytes it
moves against its algorithmic minimum, GB/s) and the box's copy rates.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa: E402,F401
from viditq_amd import ops, synth  # noqa: E402
from viditq_amd.config import loads_yaml  # noqa: E402
from viditq_amd.t2v import DMP_SOLVER, IDDPM  # noqa: E402


class Prompt:
    """The text-encoder interface around one synthetic prompt."""

    def __init__(self, y_c, y_u, mask):
        self.y_c, self.y_u, self.mask = y_c, y_u, mask

    def encode(self, prompts):
        return dict(y=self.y_c, mask=self.mask)

    def null(self, n):
        return self.y_u


def copy_rates(dev):
    """A 1 GiB device copy (HBM) and a 48 MiB one (Infinity Cache resident), TB/s of traffic, best of three."""
    out = {}
    for name, nbytes, reps in (("hbm_copy_1GiB_TBps", 1 << 30, 6), ("mall_copy_48MiB_TBps", 48 << 20, 40)):
        a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        b.copy_(a)
        best = None
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1) * 1e-3 / reps
            best = t if best is None or t < best else best
        out[name] = round(2.0 * nbytes / best / 1e12, 3)
        del a, b
    return out


def step_kernel(graph, reps=200):
    """The patch-major step alone, on the captured loop's buffers (order-2 row): us per launch and its traffic."""
    s = graph.solver
    eps = s._forward_patch(graph.xm, graph.t, graph.t_id)
    row = 5
    for _ in range(10):
        ops.cfg_dpmpp_step_patch(eps[0], eps[1], graph.x, graph.hist, graph.rows, row, graph.patch, x_model=graph.xm)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = torch.empty_like(graph.x)
    e0.record()
    for _ in range(reps):
        ops.cfg_dpmpp_step_patch(eps[0], eps[1], graph.x, graph.hist, graph.rows, row, graph.patch, x_out=out, x_model=graph.xm)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    total, es, ms = graph.x.numel(), eps[0].element_size(), graph.xm.element_size()
    c_out = eps[0].shape[2] // (graph.patch[0] * graph.patch[1] * graph.patch[2])
    dense = 4 * total * 4 + graph.xm.numel() * ms              # x, m_{k-1} read; m_k, x_out written; x_model written
    minimum = dense + 2 * total * es                           # the 4 read channels of both outputs
    moved = dense + 2 * total * es * c_out // graph.x.shape[1]  # whole 32-byte sectors: the learned-sigma half rides along
    # what the DDIM tail moves for the same latent: two unpatchify + fp32-cast passes over both full outputs (fp16 read, fp32
    # written), then vq_cfg_ddim_step (reads both fp32 outputs' used half in whole sectors and x, writes x_out)
    full = total * c_out // graph.x.shape[1]
    ddim_tail = 2 * full * (es + 4) + 2 * full * 4 + 2 * total * 4
    return dict(us_per_launch=round(us, 2), bytes_moved=moved, bytes_minimum=minimum, moved_over_minimum=round(moved / minimum, 3),
                GBps_moved=round(moved / us / 1e3, 1), ddim_tail_bytes=ddim_tail, elements=total,
                eps_dtype=str(eps[0].dtype), x_model_dtype=str(graph.xm.dtype))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=28)
    ap.add_argument("--alternate", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with torch.no_grad():
        qnn = synth.quantize_model(synth.build_stdit(dev, depth=a.depth), loads_yaml(synth.W8A8_DYNAMIC))
        qnn.cfg_split = True
        assert all(b.fused_ok() for b in qnn.model.blocks)
        embeds, _ = synth.synthetic_prompts(1, dev)
        y = embeds["y"][0:1].permute(1, 0, 2, 3, 4).reshape(2, 1, 120, 4096)
        mask = embeds["mask"][0:1]
        enc = Prompt(y[:1], y[1:], mask)
        z = synth.synthetic_latent(0, device=dev).float()
        z_size = tuple(z.shape[1:])
        ddim, dpm = IDDPM(num_sampling_steps=100, cfg_scale=4.0), DMP_SOLVER(20, 4.0)
        graph = dpm.step_graph(qnn, enc, z_size, [""], dev, cfg_split=True)

        def ddim_graphed():
            t0 = [None]

            def cb(i, x):
                if t0[0] is None:
                    torch.cuda.synchronize()
                    t0[0] = time.perf_counter()
            out = ddim.ddim_sample_loop(qnn, z, dict(y=y, mask=mask), graphed=True, step_callback=cb)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0[0]) * 1e3 / (ddim.num_timesteps - 1), out

        def timed(fn, calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / calls, out

        arms = {
            "ddim_graphed": ddim_graphed,
            "dpm_eager": lambda: timed(lambda: dpm.sample(qnn, enc, z_size, [""], dev, init_noise=z, cfg_split=True, fused=False), 20),
            "dpm_fused": lambda: timed(lambda: dpm.sample(qnn, enc, z_size, [""], dev, init_noise=z, cfg_split=True, fused=True), 20),
            "dpm_fused_graph": lambda: timed(lambda: graph.run(z), 20),
        }
        outs = {}
        for name, fn in arms.items():                          # warm-up: packing, caches, tables, captures
            if name != "ddim_graphed":
                outs[name] = fn()[1]
        readings = {name: [] for name in arms}
        started = {name: [] for name in arms}                 # seconds into the timed region: a change of the box's state shows
        t_begin = time.perf_counter()
        for _ in range(a.alternate):
            for name, fn in arms.items():
                started[name].append(round(time.perf_counter() - t_begin, 1))
                readings[name].append(round(fn()[0], 3))
        kernel = step_kernel(graph)
        rates = copy_rates(dev)
    base = readings["ddim_graphed"]
    spread = max(base) - min(base)
    line = dict(tool="t2v_dpm_time", depth=a.depth, z_size=list(z_size), plan="w8a8 dynamic, cfg_split, 1 prompt",
                ms_per_step_or_pair=readings, started_s=started, ddim_graphed_spread_ms=round(spread, 3), margin_ms=round(3 * spread, 3),
                within_margin={name: [v <= b + 3 * spread for v, b in zip(readings[name], base)]
                               for name in ("dpm_fused", "dpm_fused_graph")},
                dpm_results_bit_identical=bool(all(torch.equal(outs["dpm_eager"], v) for v in outs.values())),
                graph_captures=len(graph.graphs), step_kernel=kernel, copy_rates=rates)
    text = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

"""What the STDiT DDIM routes cost per step (GPU box only):

    python tools/t2v_ddim_time.py [--depth 28] [--alternate 3] [--steps 10] [--out FILE.json]

One STDiT-XL/2 (16 x 64 x 64 latent, W8A8 dynamic, one prompt) is built once; every arm is warmed up (packing, caches,
tables, graph captures) and then timed ``--alternate`` times in turn, in ONE process, ``--steps`` steps per reading:
  a_eager_split     ddim_sample_loop(fused=False) with cfg_split: eager launches
  b_graphed_split   ddim_sample_loop(graphed=True) with cfg_split (the parent's best).  Its captures are taken inside the
                    call, so it runs steps + 1 steps and the clock starts at the callback of the first (after a synchronise)
  c_eager_joint     ddim_sample_loop(fused=False), joint forward (the parent's only joint route)
  d_fused_split     ddim_sample_loop(fused=True) with cfg_split: patch-major forwards + ops.cfg_ddim_step_patch, eager launches
  d_fused_joint     the same, joint forward
  e_graph_split     IDDPM.step_graph(...).run(z) with cfg_split: one replay per step
  e_graph_joint     the same, joint forward
Each reading is the host clock around the loop ending in a device synchronise, in ms per step (``started_s``: when it
began).  Also reported: the spread (max - min) of the two parent arms' readings and 3 x that (the margin of the flip
criterion) with the verdict per alternation, whether the results of the split arms and of the joint
arms are the same bits, the step alone - ops.cfg_ddim_step_patch against unpatchify + cast + ops.cfg_ddim_step on the
loop's own buffers, event-timed back to back -, the board's clocks and power before and after the timed region (rocm-smi,
read only) and the box's copy rates.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa: E402,F401
from viditq_amd import ops, synth  # noqa: E402
from viditq_amd.config import loads_yaml  # noqa: E402
from viditq_amd.t2v import IDDPM  # noqa: E402

from t2v_dpm_time import copy_rates  # noqa: E402


def board():
    """Clock and power lines of rocm-smi (read only), or None when the tool is not there."""
    try:
        r = subprocess.run(["rocm-smi", "--showpower", "--showclocks"], capture_output=True, text=True, timeout=30)
    except (OSError, subprocess.TimeoutExpired):
        return None
    keep = [" ".join(ln.split()) for ln in r.stdout.splitlines()
            if any(k in ln.lower() for k in ("sclk", "mclk", "fclk", "power")) and "GPU[0]" in ln]
    return keep or None


def step_alone(graph, model, reps=200, rounds=3):
    """The step on the loop's buffers: the patch-major launch against the three it replaces, us per step, alternating."""
    eps_c, eps_u = graph._forward(serial=True)
    rows, x, xm, patch = graph.rows, graph.x, graph.xm, graph.patch
    r = rows[5].tolist()
    scal = tuple(r[i] for i in range(5))
    out = torch.empty_like(x)

    def fused():
        ops.cfg_ddim_step_patch(eps_c, eps_u, x, rows, 5, patch, x_out=out, x_model=xm)

    def dense():
        cond, unc = model.unpatchify(eps_c).to(torch.float32), model.unpatchify(eps_u).to(torch.float32)
        ops.cfg_ddim_step(cond, unc, x, *scal, out=out)

    def clock(fn):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / reps, 2)

    res = dict(patch_us=[], unpatchify_cast_dense_us=[])
    for _ in range(rounds):
        res["patch_us"].append(clock(fused))
        res["unpatchify_cast_dense_us"].append(clock(dense))
    fused()
    a = out.clone()
    dense()
    total, es = x.numel(), eps_c.element_size()
    c_out = eps_c.shape[2] // (patch[0] * patch[1] * patch[2])
    full = total * c_out // x.shape[1]
    res.update(same_bits=bool(torch.equal(a, out)), elements=total, eps_dtype=str(eps_c.dtype), x_model_dtype=str(xm.dtype),
               patch_bytes_moved=2 * full * es + 2 * total * 4 + xm.numel() * xm.element_size(),
               dense_bytes_moved=2 * full * (es + 4) + 2 * full * 4 + 2 * total * 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=28)
    ap.add_argument("--alternate", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    with torch.no_grad():
        qnn = synth.quantize_model(synth.build_stdit(dev, depth=a.depth), loads_yaml(synth.W8A8_DYNAMIC))
        assert all(b.fused_ok() for b in qnn.model.blocks)
        embeds, _ = synth.synthetic_prompts(1, dev)
        y = embeds["y"][0:1].permute(1, 0, 2, 3, 4).reshape(2, 1, 120, 4096)         # (cond | null)
        args = dict(y=y, mask=embeds["mask"][0:1])
        z = synth.synthetic_latent(0, device=dev).float()
        ddim, ddim1 = IDDPM(num_sampling_steps=a.steps, cfg_scale=4.0), IDDPM(num_sampling_steps=a.steps + 1, cfg_scale=4.0)
        graphs = {}
        for split in (True, False):
            qnn.cfg_split = split
            graphs[split] = ddim.step_graph(qnn, z, args)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / a.steps, out

        def loop(split, **kw):
            def run():
                qnn.cfg_split = split
                return timed(lambda: ddim.ddim_sample_loop(qnn, z.clone(), args, **kw))
            return run

        def graphed():
            qnn.cfg_split = True
            t0 = [None]

            def cb(i, x):
                if t0[0] is None:
                    torch.cuda.synchronize()
                    t0[0] = time.perf_counter()
            out = ddim1.ddim_sample_loop(qnn, z.clone(), args, graphed=True, step_callback=cb)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0[0]) * 1e3 / a.steps, out

        arms = {
            "a_eager_split": loop(True, fused=False),
            "b_graphed_split": graphed,
            "c_eager_joint": loop(False, fused=False),
            "d_fused_split": loop(True, fused=True),
            "d_fused_joint": loop(False, fused=True),
            "e_graph_split": lambda: timed(lambda: graphs[True].run(z)),
            "e_graph_joint": lambda: timed(lambda: graphs[False].run(z)),
        }
        outs = {}
        for name, fn in arms.items():                           # warm-up: packing, caches, tables, captures
            outs[name] = fn()[1]
            print("warmed up", name, file=sys.stderr, flush=True)
        readings = {name: [] for name in arms}
        started = {name: [] for name in arms}                   # seconds into the timed region: a change of the box's state shows
        board_before = board()
        t_begin = time.perf_counter()
        for _ in range(a.alternate):
            for name, fn in arms.items():
                started[name].append(round(time.perf_counter() - t_begin, 1))
                readings[name].append(round(fn()[0], 3))
        board_after = board()
        alone = step_alone(graphs[True], qnn)
        rates = copy_rates(dev)
    spread = {p: round(max(readings[p]) - min(readings[p]), 3) for p in ("b_graphed_split", "c_eager_joint")}
    not_above = {
        "e_graph_split_vs_b": [v <= b + 3 * spread["b_graphed_split"]
                               for v, b in zip(readings["e_graph_split"], readings["b_graphed_split"])],
        "e_graph_joint_vs_c": [v <= c + 3 * spread["c_eager_joint"]
                               for v, c in zip(readings["e_graph_joint"], readings["c_eager_joint"])],
    }
    same = lambda names: bool(all(torch.equal(outs[names[0]], outs[n]) for n in names))  # noqa: E731
    line = dict(tool="t2v_ddim_time", depth=a.depth, z_size=list(z.shape[1:]), steps_per_reading=a.steps,
                plan="w8a8 dynamic, 1 prompt, cfg 4.0", ms_per_step=readings, started_s=started, parent_spread_ms=spread,
                margin_ms={k: round(3 * v, 3) for k, v in spread.items()}, not_above=not_above,
                flip_criterion_met=bool(all(all(v) for v in not_above.values())),
                split_results_bit_identical=same(["a_eager_split", "d_fused_split", "e_graph_split"]),
                joint_results_bit_identical=same(["c_eager_joint", "d_fused_joint", "e_graph_joint"]),
                graph_captures={("split" if k else "joint"): len(g.graphs) for k, g in graphs.items()},
                step_alone=alone, board_before=board_before, board_after=board_after, copy_rates=rates)
    text = json.dumps(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

"""Temporal attention + attn_temp.proj's dynamic per-token quantizer for joint forwards and sub-8-bit grids: the two-launch
route (attn_temporal, then vq_rowquant with the token's grid shared over B) against the fused entry point
vq_attn_temporal_rowquant_shared, at the STDiT-XL/2 shapes (GPU only).

Captured graphs replayed, q | k | v rotated over 12 buffers so that no launch finds its input in L2 / MALL, the two
routes alternated three times in one process after a warm-up, best of three against best of three.  The device copy
rate comes from the same process.  Bytes are the algorithm's: the fused route reads rows * 3 C * 2 and writes rows * Kp;
the two-launch route also writes and reads the fp16 attention output (rows * C * 2 each way).

    python tools/temporal_shared_time.py [--out profiles/temporal_shared/fused.json] [--step [--depth 28]]

--step adds the forward: one STDiT-XL/2 W6A6 joint forward (cfg_split False, B = 2; the values of w6a6_naive_cb.yaml) as a
replayed graph with VQ_ATTN_QUANT_JOINT's switch on and off, three alternations.

Exit status 1 when the fused call is slower than the two launches at any shape.
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
SHAPES = [(2, 16, 8), (2, 16, 6), (1, 16, 6)]

W6A6_JOINT = """
cfg_split: False
mixed_precision: [4,6,8]
quant:
    weight:
        quantizer: {n_bits: 6, per_group: channel, channel_dim: 0, scale_method: min_max, round_mode: nearest}
    activation:
        quantizer:
            n_bits: 6
            per_group: token
            scale_method: min_max
            round_mode: nearest_ste
            running_stat: False
            dynamic: True
            sym: False
            n_spatial_token: 1024
            n_temporal_token: 16
            n_prompt: 120
            smooth_quant: {enable: False, channel_wise_scale_type: momentum_act_max, momentum: 0.95, alpha: 0.625}
"""


def kernels(dev):
    rows_out = []
    for B, T, n_bits in SHAPES:
        rows = B * T * S
        assert ops.attn_temporal_shared_ok(B, T, H, D, ops.pad128(C), n_bits)
        bufs = [torch.randn(rows, 3 * C, device=dev).half() for _ in range(12)]
        i = [0]

        def qkv():
            i[0] = (i[0] + 1) % len(bufs)
            return bufs[i[0]]
        o = torch.empty(rows, C, dtype=torch.float16, device=dev)

        def two():                                         # the parent's route
            x = qkv()
            ops.attn_temporal(x, x[:, C:], x[:, 2 * C:], o, B, T, S, H, D, 3 * C, C)
            return ops.rowquant(o.view(B, T * S, C), n_bits=n_bits)

        def fused():
            x = qkv()
            return ops.attn_temporal_rowquant_shared(x, x[:, C:], x[:, 2 * C:], B, T, S, H, D, 3 * C, n_bits=n_bits)

        n = 24
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
    return rows_out


def step(dev, depth):
    """ms per joint W6A6 forward, the block's switch off / on, each route captured once and replayed."""
    from viditq_amd import synth
    from viditq_amd.config import loads_yaml
    from viditq_amd.graph import ForwardGraph
    from viditq_amd.t2v import stdit
    qnn = synth.quantize_model(synth.build_stdit(dev, depth=depth), loads_yaml(W6A6_JOINT))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    embeds, _ = synth.synthetic_prompts(1, dev)
    y = embeds["y"][0:1].permute(1, 0, 2, 3, 4).reshape(2, 1, 120, 4096)
    x = synth.synthetic_latent(0, device=dev).float()
    x2, t2 = torch.cat([x, x]), torch.tensor([500, 500], device=dev)
    kw = dict(mask=embeds["mask"][0:1], timestep_id=500)
    graphs, outs = {}, {}
    saved = stdit._ATTN_QUANT_JOINT
    try:
        for sw in (False, True):
            stdit._ATTN_QUANT_JOINT = sw                   # read at launch time: baked into the captured graph
            graphs[sw] = ForwardGraph(qnn, x2, t2, y, kw)
            outs[sw] = graphs[sw].run(x2, t2, y).float().clone()
    finally:
        stdit._ATTN_QUANT_JOINT = saved

    def ms(g, iters=5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g.graph.replay()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            g.graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    off, on = [], []
    for _ in range(3):
        off.append(round(ms(graphs[False]), 3))
        on.append(round(ms(graphs[True]), 3))
    rel = float((outs[True] - outs[False]).norm() / outs[False].norm())
    rec = dict(depth=depth, switch_off_ms=off, switch_on_ms=on, routes_rel_l2=rel,
               not_slower_in_any_alternation=all(b <= a for a, b in zip(off, on)))
    print("W6A6 joint forward, depth %d: switch off %s ms | on %s ms | rel-L2 between the routes %.2e" % (depth, off, on, rel),
          flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help="also time one joint W6A6 STDiT-XL/2 forward, switch on / off")
    ap.add_argument("--depth", type=int, default=28)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("temporal_shared_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    src = torch.empty(16384 * 4608, dtype=torch.float16, device=dev)
    dst = torch.empty_like(src)
    copy_us, _ = graph_time(lambda: dst.copy_(src), n=8, reps=8)
    copy_tbs = 2 * src.numel() * 2 / copy_us / 1e6
    del src, dst
    print("device copy: %.1f us = %.2f TB/s" % (copy_us, copy_tbs))
    rec = dict(device=torch.cuda.get_device_name(0), copy_us=round(copy_us, 1), copy_TBps=round(copy_tbs, 2))

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)
    rec["shapes"] = kernels(dev)
    write()
    if args.step:
        with torch.no_grad():
            rec["forward"] = step(dev, args.depth)
        write()
    return 0 if all(r["not_slower"] for r in rec["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())

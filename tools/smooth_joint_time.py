"""The smoothed q | k | v quantizers of a joint forward (x [2, n_tok, C], a token's grid shared by its two samples): the
launches the block makes today against the one-pass entry point vq_rowquant_smooth_multi_shared, at the STDiT-XL/2 shape
2 x 16384 x 1152 (GPU only).

    plain, G outputs   today G x vq_rowquant(B = 2, s_j) (smooth_rowquant_half_kernel<.., PAIR>)
    LN, 3 outputs      today vq_ln_modulate_rowquant(B = 2, n_out = 3): the generic ln_modulate_rowquant_kernel<3>
    LN, 1 output       today vq_ln_modulate_rowquant(B = 2, n_out = 1): vq_lnq_pair_fast (the block keeps it for fc1)

Captured graphs replayed, the input rotated over 12 buffers so that no launch finds its rows in L2 / MALL, the two routes
alternated three times in one process after a warm-up, best of three against best of three.  The device copy rate comes
from the same process.  Bytes are the algorithm's: one pass reads rows * C * 2 and writes G * rows * (C + 12).

    python tools/smooth_joint_time.py [--out profiles/smooth_joint/one_pass.json] [--step [--depth 28]]

--step adds the forward: one STDiT-XL/2 joint forward (cfg_split False, B = 2) of the W8A8 smooth-quant plan (synthetic
calibration) as a replayed graph with VQ_SMOOTH_JOINT's switch off and on, three alternations.

Exit status 1 when the one-pass call is slower than the launches it replaces at any shape.
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

N_TOK, C = 16384, 1152
# (LN arm, outputs, n_bits)
SHAPES = [(ln, g, b) for ln in (False, True) for g in (1, 3) for b in (8, 6)]


def kernels(dev):
    rows_out = []
    gen = torch.Generator().manual_seed(1)
    sv = [torch.exp(torch.randn(C, generator=gen) * 0.6).float().to(dev) for _ in range(3)]
    assert all(ops.smooth_rcp(s) is not None for s in sv)
    shift, scale = [(torch.randn(2, C, generator=gen) * 0.3).float().to(dev) for _ in range(2)]
    bufs = [torch.randn(2, N_TOK, C, device=dev).half() for _ in range(12)]
    i = [0]

    def x():
        i[0] = (i[0] + 1) % len(bufs)
        return bufs[i[0]]
    for ln, G, n_bits in SHAPES:
        assert ops.rowquant_multi_shared_ok(2, N_TOK, C, ops.pad128(C), n_bits, G)
        s = sv[:G]

        def old():                                          # the parent's route
            xx = x()
            if ln:
                return ops.ln_modulate_rowquant(xx, shift, scale, 1e-6, smooth=s, n_bits=n_bits)
            return [ops.rowquant(xx, n_bits=n_bits, s=sj) for sj in s]

        def new():
            return ops.rowquant_multi_shared(x(), s, n_bits=n_bits, shift=shift if ln else None, scale=scale if ln else None)

        n = 24
        rows = 2 * N_TOK
        mb_new = rows * (C * 2 + G * (C + 12)) / 1e6
        mb_old = mb_new if ln else G * rows * (C * 2 + C + 12) / 1e6
        t_old, t_new = [], []
        keep = [graph_time(old, n=n)[1], graph_time(new, n=n)[1]]            # warm-up of both routes
        for _ in range(3):
            t_old.append(graph_time(old, n=n)[0])
            t_new.append(graph_time(new, n=n)[0])
        del keep
        ba, bb = min(t_old), min(t_new)
        name = "%s, %d output%s, %d bits" % ("LN" if ln else "plain", G, "s" if G > 1 else "", n_bits)
        rows_out.append(dict(shape=name, today_MB=round(mb_old, 1), one_pass_MB=round(mb_new, 1),
                             today_us=[round(t, 1) for t in t_old], one_pass_us=[round(t, 1) for t in t_new],
                             today_best_us=round(ba, 1), one_pass_best_us=round(bb, 1), one_pass_TBps=round(mb_new / bb, 2),
                             not_slower=bb <= ba))
        print("%-26s today %s -> best %.1f us | one pass %s -> best %.1f us (%.2f TB/s of %.1f MB) | %s" % (
            name, ["%.1f" % t for t in t_old], ba, ["%.1f" % t for t in t_new], bb, mb_new / bb, mb_new,
            "not slower" if bb <= ba else "SLOWER"), flush=True)
    return rows_out


def step(dev, depth):
    """ms per joint smoothed W8A8 forward, the block's switch off / on, each route captured once and replayed."""
    from viditq_amd import synth
    from viditq_amd.config import loads_yaml
    from viditq_amd.graph import ForwardGraph
    from viditq_amd.t2v import stdit
    text = synth.W4A8_TIMESTEP_AWARE.replace("cfg_split: True", "cfg_split: False").replace("quantizer: {n_bits: 4,", "quantizer: {n_bits: 8,")
    qnn = synth.quantize_model(synth.build_stdit(dev, depth=depth), loads_yaml(text))
    assert all(b.fused_ok() for b in qnn.model.blocks)
    embeds, _ = synth.synthetic_prompts(1, dev)
    y = embeds["y"][0:1].permute(1, 0, 2, 3, 4).reshape(2, 1, 120, 4096)
    x = synth.synthetic_latent(0, device=dev).float()
    x2, t2 = torch.cat([x, x]), torch.tensor([500, 500], device=dev)
    kw = dict(mask=embeds["mask"][0:1], timestep_id=500)
    graphs, outs = {}, {}
    saved = stdit._SMOOTH_JOINT
    try:
        for sw in (False, True):
            stdit._SMOOTH_JOINT = sw                       # read at launch time: baked into the captured graph
            graphs[sw] = ForwardGraph(qnn, x2, t2, y, kw)
            outs[sw] = graphs[sw].run(x2, t2, y).float().clone()
    finally:
        stdit._SMOOTH_JOINT = saved

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
    print("W8A8 smoothed joint forward, depth %d: switch off %s ms | on %s ms | rel-L2 between the routes %.2e" % (
        depth, off, on, rel), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help="also time one joint smoothed STDiT-XL/2 forward, switch off / on")
    ap.add_argument("--depth", type=int, default=28)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("smooth_joint_time.py needs a GPU: a CPU run gives no time")
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
    with torch.no_grad():
        rec["shapes"] = kernels(dev)
    write()
    if args.step:
        with torch.no_grad():
            rec["forward"] = step(dev, args.depth)
        write()
    return 0 if all(r["not_slower"] for r in rec["shapes"]) else 1


if __name__ == "__main__":
    sys.exit(main())

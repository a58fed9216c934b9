"""The running smooth-quant statistic on the device (VQ_RUNNING_SMOOTH_DEVICE) at the PixArt-Sigma 1024^2 shapes: B = 2,
4096 tokens, mlp.fc2 K = 4608 -> N = 1152, 4-bit weights (GPU only).  Three measurements, the routes alternated three
times in one process after a warm-up, best of three against best of three:

  kernel  vq_act_scale_momentum (zero + column max + finalize: three launches) as a captured graph, the input rotated over
          12 buffers so that no launch finds it in L2 / MALL; beside it the device copy rate and the C = 4608 row quantizer
          measured the same way in the same process.  Bytes are the algorithm's: the kernel reads x once.
  layer   mlp.fc2's forward: QuantLayer.forward (host-visible statistic: three synchronisations, fresh packed buffers - it
          cannot be captured, so both routes are timed as eager calls between two device synchronisations) against
          QuantLayer.running_stat_step + its GEMM; the latter also as a captured graph.
  step    one batched (uncond | cond) forward of the depth-D model whose last block's mlp.fc2 keeps its statistic running
          (quant_txt2img.py:297-300), switch off (that block layer by layer) against switch on (every block fused), eager;
          and whether the switched-on forward captures into a graph and what a replay takes.

Weights are synthetic, weight grids data-free min-max of W (not of W*s: the grid only decides how many codes clamp, not
what a launch costs).

    python tools/running_smooth_time.py [--depth 28] [--out profiles/running_smooth/times.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa: E402,F401
from static_quant_time import graph_time  # noqa: E402
from viditq_amd import ops, synth  # noqa: E402
from viditq_amd.config import to_config  # noqa: E402
from viditq_amd.qdiff.models import QuantModel  # noqa: E402
from viditq_amd.t2v import stdit  # noqa: E402

B, TOK, K, N = 2, 4096, 4608, 1152
NBUF = 12
LP = 300


def eager_time(fn, n):
    """us per call: n eager calls between two device synchronisations (host clock)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def alternate(fa, fb, rounds=3):
    a, b = [], []
    fa(), fb()                                              # warm-up of both
    for _ in range(rounds):
        a.append(fa())
        b.append(fb())
    return a, b


def build_model(dev, depth):
    from viditq_amd.t2i import PixArtMS_XL_2
    lat = 128
    m = PixArtMS_XL_2(input_size=lat, model_max_length=LP, pe_interpolation=lat / 64, dtype=torch.float16)
    if depth != 28:
        m.blocks = m.blocks[:depth]
    synth.redraw_zero_init(m, 1)
    m = m.half().to(dev).eval()
    wq = to_config(dict(n_bits=4, per_group="channel", channel_dim=0, scale_method="min_max", round_mode="nearest",
                        mixed_precision=[4, 6, 8]))
    aq = to_config(dict(n_bits=8, per_group="token", scale_method="min_max", round_mode="nearest_ste", running_stat=False,
                        dynamic=True, sym=False, n_spatial_token=(lat // 2) ** 2, n_temporal_token=1, n_prompt=LP,
                        smooth_quant=dict(enable=True, channel_wise_scale_type="momentum_act_max", momentum=0.95, alpha=0.3)))
    qnn = QuantModel(m, wq, aq, model_type="pixart")
    qnn.set_module_name_for_quantizer(qnn.model)
    qnn.fp_layer_list = ["x_embedder", "t_embedder", "t_block", "y_embedder", "csize_embedder", "ar_embedder"]
    qnn.set_smooth_quant(smooth_quant=False, smooth_quant_running_stat=False)
    synth.init_weight_quantizers(qnn)
    # the released script's arrangement: channel balancing on the last block's mlp.fc2 only, its statistic still running
    qnn.set_layer_smooth_quant(model=qnn, module_name_list=["blocks.%d.mlp.fc2" % (depth - 1)], smooth_quant=True,
                               smooth_quant_running_stat=True)
    qnn.set_quant_state(True, True)
    return qnn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=28)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("running_smooth_time.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rec = dict(device=torch.cuda.get_device_name(0), shape=dict(B=B, n_tok=TOK, K=K, N=N, w_bits=4))

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)

    with torch.no_grad():
        # ---------------------------------------------------------------- kernel
        src = torch.empty(16384 * 4608, dtype=torch.float16, device=dev)
        dst = torch.empty_like(src)
        copy_us, _ = graph_time(lambda: dst.copy_(src), n=8, reps=8)
        copy_tbs = 2 * src.numel() * 2 / copy_us / 1e6
        del src, dst
        bufs = [torch.nn.functional.gelu(torch.randn(B, TOK, K, device=dev), approximate="tanh").half() for _ in range(NBUF)]
        i = [0]

        def nxt():
            i[0] = (i[0] + 1) % NBUF
            return bufs[i[0]]
        stat = torch.zeros(K, device=dev)
        scratch = torch.empty(B * K, dtype=torch.int32, device=dev)
        t_stat, t_rq = alternate(lambda: graph_time(lambda: ops.act_scale_momentum(nxt(), stat, 0.95, scratch=scratch), n=12)[0],
                                 lambda: graph_time(lambda: ops.rowquant(nxt(), n_bits=8), n=12)[0])
        mb = B * TOK * K * 2 / 1e6
        mb_rq = mb + B * TOK * K / 1e6
        rec["kernel"] = dict(copy_us=round(copy_us, 1), copy_TBps=round(copy_tbs, 2), read_MB=round(mb, 1),
                             act_scale_momentum_us=[round(t, 1) for t in t_stat],
                             act_scale_momentum_TBps=round(mb / min(t_stat), 2),           # MB / us = TB/s
                             rowquant_c4608_us=[round(t, 1) for t in t_rq], rowquant_MB=round(mb_rq, 1),
                             rowquant_c4608_TBps=round(mb_rq / min(t_rq), 2))
        rec["kernel"]["share_of_copy_rate"] = dict(act_scale_momentum=round(mb / min(t_stat) / copy_tbs, 3),
                                                   rowquant_c4608=round(mb_rq / min(t_rq) / copy_tbs, 3))
        print(json.dumps(rec["kernel"]), flush=True)
        save()

        # ---------------------------------------------------------------- layer
        qnn = build_model(dev, args.depth)
        fc2 = qnn.model.blocks[-1].mlp.fc2
        assert fc2.running_stat_device_ok() and tuple(fc2.weight.shape) == (N, K)
        lw = copy.deepcopy(fc2)

        def layerwise():
            return lw(nxt())

        def device():
            qa, pw = fc2.running_stat_step(nxt())
            return ops.gemm_i8(qa, pw, bias=fc2.bias_f32())
        t_lw, t_dev = alternate(lambda: eager_time(layerwise, 20), lambda: eager_time(device, 20))
        t_graph = [graph_time(device, n=12)[0] for _ in range(3)]
        rec["layer"] = dict(layerwise_eager_us=[round(t, 1) for t in t_lw], device_step_eager_us=[round(t, 1) for t in t_dev],
                            device_step_graph_us=[round(t, 1) for t in t_graph],
                            not_slower=min(t_dev) <= min(t_lw))
        print(json.dumps(rec["layer"]), flush=True)
        save()
        del fc2, lw, bufs
        torch.cuda.empty_cache()

        # ---------------------------------------------------------------- step
        g = torch.Generator().manual_seed(1)
        x = torch.randn(2, 4, 128, 128, generator=g).to(dev)
        y = (torch.randn(2, 1, LP, 4096, generator=g) * 0.1).half().to(dev)
        mask = torch.zeros(2, LP, dtype=torch.int64, device=dev)
        mask[0, :180] = 1
        mask[1, :143] = 1
        t = torch.tensor([500, 500], device=dev)
        last = qnn.model.blocks[-1]

        def forward(flag):
            stdit._RUNNING_SMOOTH_DEVICE = flag
            assert stdit.takes_fused(last) == flag and not last.fused_ok()
            return qnn(x, t, y, mask=mask, timestep_id=500)         # (without it QuantModel.forward reads t[0] on the host)

        t_off, t_on = alternate(lambda: eager_time(lambda: forward(False), 5), lambda: eager_time(lambda: forward(True), 5))
        rec["step"] = dict(depth=args.depth, flag_off_eager_ms=[round(v / 1e3, 3) for v in t_off],
                           flag_on_eager_ms=[round(v / 1e3, 3) for v in t_on], flag_on_not_slower=min(t_on) <= min(t_off))
        print(json.dumps(rec["step"]), flush=True)
        save()
        try:
            us, _ = graph_time(lambda: forward(True), n=1, reps=5)
            rec["step"]["flag_on_replays_from_a_graph"] = True
            rec["step"]["flag_on_graph_replay_ms"] = round(us / 1e3, 3)
        except Exception as e:                              # a host read of device data fails the capture
            rec["step"]["flag_on_replays_from_a_graph"] = False
            rec["step"]["capture_error"] = str(e)[:300]
        stdit._RUNNING_SMOOTH_DEVICE = False
        rec["step"]["status_word"] = qnn.check_status()
        print(json.dumps(rec["step"]), flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())

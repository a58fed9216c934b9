"""PixArt-Sigma 1024x1024 (N = 4096 tokens, Lp <= 300) W4A8 / W8A8 sampling-step rate on one MI355X: the parity
configuration 5 of BASELINE.json as a timing run (not the bench.py metric).  Synthetic weights / latents /
text embeds; weights min-max per channel (data-free), activations dynamic per token; DPM-Solver++ 2M loop,
cfg 4.5, the reference's ONE batched (uncond | cond) forward per step (B = 2: token scales shared over the
pair, as base_quantizer.py:185 does).  GPU box only.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viditq_amd  # noqa
from viditq_amd import synth
from viditq_amd.config import to_config
from viditq_amd.qdiff.models import QuantModel
from viditq_amd.t2i import DPMS_sigma, IDDPM, PixArtMS_XL_2, SASolverSampler

ap = argparse.ArgumentParser()
ap.add_argument("--w-bits", type=int, default=4)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--depth", type=int, default=28)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--graph", action="store_true", help="replay the forward as one captured HIP graph (graph.GraphedModel) instead of eager launches")
ap.add_argument("--fused-step", action="store_true",
                help="guidance + x0 + multistep update in one launch per model call (ops.cfg_dpmpp_step); with --graph the whole "
                     "step {forward, fused step, counter advance} is ONE captured graph replayed per timestep (graph.DPMStepGraph)")
ap.add_argument("--sampler", choices=("dpm", "iddpm", "sa"), default="dpm",
                help="iddpm: the ancestral loop of --sampling_algo iddpm (t2i/iddpm.py, IDDPM(str(steps)).p_sample_loop("
                     "forward_with_cfg)); --fused-step is then ops.cfg_ddpm_step and --fused-step --graph graph.DDPMStepGraph.  "
                     "sa: the SA-Solver loop of --sampling_algo sa-solver (t2i/sa_solver.py, SASolverSampler.sample: few_steps, "
                     "PEC, predictor 2, corrector 2, eta 1); --fused-step is then ops.cfg_sa_step and --fused-step --graph "
                     "graph.SAStepGraph")
ap.add_argument("--alternate", type=int, default=0,
                help="N > 0: time the arms eager / fused-step / graph / fused-step+graph N times in turn in THIS process "
                     "(same weights, same latent) and print one JSON line with every figure, the GEMM clock probe and the "
                     "copy probe of bench.py beside them")
a = ap.parse_args()
dev = torch.device("cuda:0")
lat = a.size // 8
Lp = 300
with torch.no_grad():
    torch.manual_seed(0)
    m = PixArtMS_XL_2(input_size=lat, model_max_length=Lp, pe_interpolation=lat / 64, dtype=torch.float16)
    if a.depth != 28:
        m.blocks = m.blocks[:a.depth]
    synth.redraw_zero_init(m, 1)
    m = m.half().to(dev).eval()
    wq = to_config(dict(n_bits=a.w_bits, per_group="channel", channel_dim=0, scale_method="min_max", round_mode="nearest",
                        mixed_precision=[4, 6, 8]))
    aq = to_config(dict(n_bits=8, per_group="token", scale_method="min_max", round_mode="nearest_ste", running_stat=False,
                        dynamic=True, sym=False, n_spatial_token=(lat // 2) ** 2, n_temporal_token=1, n_prompt=Lp,
                        smooth_quant=dict(enable=False)))
    qnn = QuantModel(m, wq, aq, model_type="pixart")
    qnn.set_module_name_for_quantizer(qnn.model)
    qnn.fp_layer_list = ["x_embedder", "t_embedder", "t_block", "y_embedder", "csize_embedder", "ar_embedder"]
    synth.init_weight_quantizers(qnn)
    qnn.set_quant_state(True, True)
    assert all(b.fused_ok() for b in qnn.model.blocks)
    g = torch.Generator().manual_seed(1)
    y = (torch.randn(1, 1, Lp, 4096, generator=g) * 0.1).half().to(dev)
    null_y = (torch.randn(1, 1, Lp, 4096, generator=g) * 0.1).half().to(dev)
    mask = torch.zeros(1, Lp, dtype=torch.int64, device=dev)
    mask[0, :180] = 1
    z = torch.randn(1, 4, lat, lat, generator=g).to(dev)
    from viditq_amd.graph import GraphedModel
    kw = dict(condition=y, uncondition=null_y, cfg_scale=4.5, model_kwargs=dict(data_info=None, mask=mask))

    def make_iddpm_arm(graph, fused):
        """The same four arms for the IDDPM loop.  Every run draws its noise from a generator seeded alike, so the arms
        see the same stack (the eager arms and the fused ones then differ by their exp only)."""
        z2 = z.repeat(2, 1, 1, 1)
        kw2 = dict(y=torch.cat([y, null_y]), cfg_scale=4.5, data_info=None, mask=mask)
        ds, sgs = {}, {}
        gm = GraphedModel(qnn.forward_with_cfg, qnn=qnn)
        model = (lambda x, timestep, y, **k: gm(x, timestep, y, **k)) if graph and not fused else qnn.forward_with_cfg

        def run(steps):
            d = ds.get(steps)
            if d is None:
                d = ds[steps] = IDDPM(str(steps))
                if fused:
                    d.model_input_dtype = torch.float16
            gen = torch.Generator(device=dev).manual_seed(3)
            if graph and fused:
                if steps not in sgs:
                    sgs[steps] = d.p_sample_graph(qnn.forward_with_cfg, z2, clip_denoised=False, model_kwargs=kw2)
                return sgs[steps].run(z2, generator=gen).chunk(2, dim=0)[0]
            return d.p_sample_loop(model, z2.shape, z2, clip_denoised=False, model_kwargs=kw2, fused=fused,
                                   generator=gen).chunk(2, dim=0)[0]
        return run

    def make_sa_arm(graph, fused):
        """The same four arms for the SA-Solver loop.  Every run draws its noise from a generator seeded alike, so the arms
        see the same 1 + steps draws."""
        gm = GraphedModel(qnn.forward_with_dpmsolver, qnn=qnn)
        smp = SASolverSampler(gm if graph and not fused else qnn.forward_with_dpmsolver, device=dev)
        if fused:
            smp.model_input_dtype = torch.float16
        sgs = {}
        tau = lambda t: 1 if 0.2 <= t <= 0.8 else 0   # noqa: E731  (sa_sampler.py:90 with eta = 1)

        def run(steps):
            gen = torch.Generator(device=dev).manual_seed(3)
            if graph and fused:
                if steps not in sgs:
                    sgs[steps] = smp.solver(y, null_y, 4.5, kw["model_kwargs"]).step_graph(z, tau, steps)
                return sgs[steps].run(z, generator=gen)
            return smp.sample(steps, z.shape[0], tuple(z.shape[1:]), conditioning=y, unconditional_conditioning=null_y,
                              unconditional_guidance_scale=4.5, eta=1, x_T=z, model_kwargs=kw["model_kwargs"], fused=fused,
                              generator=gen)[0]
        return run

    def make_arm(graph, fused):
        """sample(steps) -> latent for one arm; built (and its graphs captured) once."""
        if a.sampler == "iddpm":
            return make_iddpm_arm(graph, fused)
        if a.sampler == "sa":
            return make_sa_arm(graph, fused)
        if graph and fused:
            s = DPMS_sigma(qnn.forward_with_dpmsolver, **kw)
            s.model_input_dtype = torch.float16
            sgs = {}

            def run(steps):
                if steps not in sgs:
                    sgs[steps] = s.step_graph(z, steps=steps, order=2)
                return sgs[steps].run(z)
            return run
        s = DPMS_sigma(GraphedModel(qnn.forward_with_dpmsolver, qnn=qnn) if graph else qnn.forward_with_dpmsolver, **kw)
        if fused:
            s.model_input_dtype = torch.float16
        return lambda steps: s.sample(z, steps=steps, order=2, fused=fused)

    def timed(run, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(steps)
        t_host = time.perf_counter() - t0                  # host done enqueuing (the GPU may still be running)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        assert torch.isfinite(out).all()
        return out, {"ms_per_step": el / steps * 1e3, "host_enqueue_ms_per_step": t_host / steps * 1e3}

    workload = "PixArt-Sigma %dx%d W%dA8, %d tokens, Lp %d, %s, cfg 4.5, batched %s forward" % (
        a.size, a.size, a.w_bits, (lat // 2) ** 2, Lp,
        {"dpm": "DPM-Solver++ 2M", "iddpm": "IDDPM ancestral (learned-range variance)",
         "sa": "SA-Solver few_steps PEC P2/C2 eta 1"}[a.sampler], "cond|uncond" if a.sampler == "iddpm" else "uncond|cond")
    if a.alternate > 0:
        import bench
        arms = {"eager": make_arm(False, False), "fused_step": make_arm(False, True), "graph": make_arm(True, False),
                "fused_step_graph": make_arm(True, True)}
        outs = {}
        for name, run in arms.items():                     # warm-up: packing, caches, captures (at the timed step count)
            run(2)
            outs[name] = run(a.steps)
        torch.cuda.synchronize()
        res = {name: [] for name in arms}
        for _ in range(a.alternate):
            for name, run in arms.items():
                res[name].append(timed(run, a.steps)[1])
        print(json.dumps({"workload": workload, "steps": a.steps, "depth": a.depth, "alternations": a.alternate,
                          "arms": res, "bit_identical_to_eager": {n: bool(torch.equal(o, outs["eager"])) for n, o in outs.items()},
                          "max_abs_diff_to_eager": {n: float((o - outs["eager"]).abs().max()) for n, o in outs.items()},
                          "gemm_shader_clock": bench.gemm_clock_probe(dev), "memory": bench.memory_probe(dev),
                          "status_word": qnn.check_status()}))
        sys.exit(0)
    run = make_arm(a.graph, a.fused_step)
    run(2)                                                 # warm-up: packing, caches
    if a.graph and a.fused_step:
        run(a.steps)                                       # the capture for the timed step count
    out, t = timed(run, a.steps)
    print(json.dumps({"workload": workload, "steps": a.steps, "depth": a.depth, "hip_graph": a.graph,
                      "fused_step": a.fused_step, "steps_per_s": 1e3 / t["ms_per_step"], "ms_per_step": t["ms_per_step"],
                      "host_enqueue_ms_per_step": t["host_enqueue_ms_per_step"], "status_word": qnn.check_status()}))

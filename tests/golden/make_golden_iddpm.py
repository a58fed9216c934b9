"""Generate the IDDPM golden vectors by IMPORTING THE REFERENCE (authoring container only).

Run:  python tests/golden/make_golden_iddpm.py        (needs the reference checkout oracle/ref_import.py locates; writes tests/golden/t2i_iddpm.npz)

From the reference's own ``diffusion.iddpm.IDDPM`` (t2i/diffusion/iddpm.py) on the CPU:
  * for the respacings "100", "20", "10" and "ddim25": timestep_map and the float64 arrays sqrt_recip_alphas_cumprod,
    sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2, posterior_log_variance_clipped, log(betas);
  * for "10": two full ``p_sample_loop_progressive`` trajectories (clip_denoised False and True) of the analytic
    forward_with_cfg-shaped model of tests/ddpm_step_cases.py on a duplicated [2, 4, 8, 8] latent, with the start latent,
    the noise stack (the draws ``randn_like`` makes after ``torch.manual_seed(SEED)``, shared by both trajectories),
    every step's ``sample`` and ``pred_xstart``, and the timesteps the model was called with.
Only data is written; no reference source text.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_import  # noqa: E402
import ddpm_step_cases as pc  # noqa: E402

RESPACINGS = ("100", "20", "10", "ddim25")
ARRAYS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
          "posterior_log_variance_clipped")
SEED, CFG, SHAPE = 7, 4.5, (2, 4, 8, 8)


def reference_iddpm():
    ref_import.load_t2i()
    return importlib.import_module("diffusion.iddpm").IDDPM


def start_latent(seed):
    z = torch.from_numpy(pc.gauss((SHAPE[0] // 2,) + SHAPE[1:], seed))
    return z.repeat(2, 1, 1, 1)


def noise_stack(seed, steps):
    torch.manual_seed(seed)
    return torch.stack([torch.randn(*SHAPE) for _ in range(steps)])


def reference_trajectory(IDDPM, respacing, clip, seed, half=False):
    """(samples [steps, ...], pred_xstarts [steps, ...], timesteps seen) of the reference's own loop."""
    d = IDDPM(respacing)
    calls = []
    model = pc.analytic_cfg_model(half, calls)
    torch.manual_seed(seed)
    outs = list(d.p_sample_loop_progressive(model, SHAPE, start_latent(seed), clip_denoised=clip,
                                            model_kwargs=dict(cfg_scale=CFG), device="cpu"))
    return (torch.stack([o["sample"] for o in outs]), torch.stack([o["pred_xstart"] for o in outs]),
            [int(t[0][0]) for t in calls])


def main():
    IDDPM = reference_iddpm()
    out = {}
    for resp in RESPACINGS:
        d = IDDPM(resp)
        out["%s.timestep_map" % resp] = np.asarray(d.timestep_map, dtype=np.int64)
        for name in ARRAYS:
            out["%s.%s" % (resp, name)] = np.asarray(getattr(d, name), dtype=np.float64)
        out["%s.log_betas" % resp] = np.log(np.asarray(d.betas, dtype=np.float64))
    out["traj.z"] = start_latent(SEED).numpy()
    out["traj.noise"] = noise_stack(SEED, 10).numpy()
    for clip in (False, True):
        samples, x0s, seen = reference_trajectory(IDDPM, "10", clip, SEED)
        key = "traj.clip%d" % int(clip)
        out[key + ".sample"], out[key + ".pred_xstart"] = samples.numpy(), x0s.numpy()
        out[key + ".timesteps"] = np.asarray(seen, dtype=np.int64)
    path = os.path.join(HERE, "t2i_iddpm.npz")
    np.savez(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()

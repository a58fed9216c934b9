"""Generate the STDiT DPM-Solver++ golden vectors by IMPORTING THE REFERENCE (authoring container only).

Run:  python tests/golden/make_golden_t2v_dpms.py     (needs the reference checkout oracle/ref_import.py locates; writes tests/golden/t2v_dpm_solver.npz)

From the reference's own ``opensora.schedulers.dpms`` (t2v/opensora/schedulers/dpms/__init__.py, dpm_solver.py) on the CPU:
  * the fp32 schedule arrays of the NoiseScheduleVP that DPMS builds (t_array, log_alpha_array) and get_time_steps(
    'time_uniform') for every step count of t2v_dpm_cases.STEPS;
  * per (steps, cfg_scale) of STEPS x CFGS: ``DMP_SOLVER(steps, cfg).sample(model, text_encoder, z_size, prompts, 'cpu')``
    - which is DPMS(partial(forward_with_dpmsolver, model), ...).sample(z, steps, order=2, skip_type='time_uniform',
    method='multistep') - on the analytic model and the toy text encoder of tests/t2v_dpm_cases.py, n = 2: the start
    latent (the draw ``torch.randn`` makes after ``torch.manual_seed``), for every model call its input, time and
    [2n, 8, 2, 4, 6] output, and the final sample.  The input of call k + 1 is the sample after step k, so the calls are
    the trajectory.  A step count the reference refuses (steps < order trips its assertion) is recorded as refused.
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
import t2v_dpm_cases as tc  # noqa: E402


def main():
    ref_import.install()
    pkg = importlib.import_module("opensora.schedulers.dpms")
    sol = importlib.import_module("opensora.schedulers.dpms.dpm_solver")
    out = {}
    solver = sol.DPMS(None, condition=None, uncondition=None, cfg_scale=4.0)
    ns = solver.noise_schedule
    out["ns.t_array"] = ns.t_array.reshape(-1).numpy()
    out["ns.log_alpha_array"] = ns.log_alpha_array.reshape(-1).numpy()
    out["ns.total_N"] = np.array(ns.total_N)
    for steps in tc.STEPS:
        out["ts.%d" % steps] = solver.get_time_steps("time_uniform", ns.T, 1.0 / ns.total_N, steps, "cpu").numpy()
    enc = tc.ToyTextEncoder()
    refused = []
    for steps in tc.STEPS:
        for cfg in tc.CFGS:
            key = "traj.s%d.cfg%g." % (steps, cfg)
            calls = []
            model = tc.AnalyticSTDiT(calls)
            torch.manual_seed(tc.SEED)
            z = torch.randn(len(tc.PROMPTS), *tc.Z_SIZE)
            torch.manual_seed(tc.SEED)
            try:
                final = pkg.DMP_SOLVER(num_sampling_steps=steps, cfg_scale=cfg).sample(model, enc, tc.Z_SIZE, tc.PROMPTS, "cpu")
            except AssertionError:
                refused.append(steps)
                continue
            assert len(calls) == steps and torch.equal(calls[0][0], torch.cat([z, z])) and torch.isfinite(final).all()
            out[key + "z"], out[key + "final"] = z.numpy(), final.numpy()
            out[key + "x_in"] = torch.stack([c[0] for c in calls]).numpy()
            out[key + "t_in"] = torch.stack([c[1] for c in calls]).numpy()
            out[key + "y_in"] = calls[0][2].numpy()
            assert all(torch.equal(c[2], calls[0][2]) and torch.equal(c[3], calls[0][3]) for c in calls)
            out[key + "mask"] = calls[0][3].numpy()
            out[key + "out"] = torch.stack([tc.analytic_eps(c[0], c[1], c[2]) for c in calls]).numpy()
    out["refused_steps"] = np.array(sorted(set(refused)), dtype=np.int64)
    path = os.path.join(HERE, "t2v_dpm_solver.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes, refused steps %s" % (path, len(out), os.path.getsize(path), sorted(set(refused))))


if __name__ == "__main__":
    main()

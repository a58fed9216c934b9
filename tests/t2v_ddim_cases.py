"""Cases of the patch-major DDIM step (vq_cfg_ddim_step_patch) and the fused STDiT DDIM loop: the step as a model on the
host - the kernel's index map (t2v_dpm_cases.gather) followed by the per-element arithmetic of the dense step
(fp_edge_cases.sampler_reference) -, the exactly computable S1 / S3 operands of fp_edge_cases carried into the patch-major
layout, the mutants that apply plus an index-map one, and a row builder."""
import dataclasses

import numpy as np
import torch

import fp_edge_cases as fe
import t2v_dpm_cases as tc

ROW = 16
CFG, ONE_PLUS_K, A, BC, ABAR_PREV, T_NEXT = 0, 1, 2, 3, 4, 14

# the mutants of fp_edge_cases that have a meaning here, and two of this layout's own
MUTANTS = ("cfg_all_channels", "sigma_half", "no_k", "cond_uncond_swapped", "second_pass_missing", "hw_swapped")
MUTANT_FAMILY = dict({m: fe.SAMPLER_MUTANT_FAMILY[m] for m in MUTANTS[:4]}, second_pass_missing="S3", hw_swapped="S1")
FIRST_PASS_ITEMS = 1024 * 256             # items one pass of the patch-major grid covers


def row(cfg, one_plus_k, a, bc, abar_prev, t_next=0.0):
    r = np.zeros(ROW, dtype=np.float32)
    r[[CFG, ONE_PLUS_K, A, BC, ABAR_PREV, T_NEXT]] = [cfg, one_plus_k, a, bc, abar_prev, t_next]
    return r


def rows_of(params_list):
    """[len, ROW] fp32 table of (cfg, 1 + k, A, Bc, abar_prev) tuples."""
    return torch.from_numpy(np.stack([row(*p) for p in params_list]))


def params_of(r):
    """(cfg, 1 + k, A, Bc, abar_prev) of a table row as Python floats (what the dense entry point is passed)."""
    return tuple(float(r[i]) for i in (CFG, ONE_PLUS_K, A, BC, ABAR_PREV))


def gather_hw_swapped(eps_pm, C, T, H, W, Co, patch):
    """t2v_dpm_cases.gather with h and w exchanged inside the column (the index-map mutant)."""
    pt, ph, pw = patch
    n = eps_pm.shape[0]
    b, c, t, h, w = np.meshgrid(np.arange(n), np.arange(C), np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    token = ((t // pt) * (H // ph) + h // ph) * (W // pw) + w // pw
    column = (((t % pt) * pw + w % pw) * ph + h % ph) * Co + c
    return eps_pm[b, token, column]


def scase_of(pm_c, pm_u, x, params, patch, Co, swapped=False):
    """The dense case fp_edge_cases.sampler_reference takes, read from the two patch-major arrays [n, tokens, columns]
    (any float type, widened to fp32) through the index map; the sigma half is NaN."""
    n, C, T, H, W = x.shape
    inner = T * H * W
    g = gather_hw_swapped if swapped else tc.gather

    def dense(pm):
        v = torch.from_numpy(np.ascontiguousarray(g(pm.float().numpy(), C, T, H, W, Co, patch))).reshape(n, C, inner)
        return torch.cat([v, torch.full_like(v, fe.NAN)], dim=1)

    return fe.SCase("patch_%dx%dx%d" % (n, C, inner), "S1", "", n, C, inner, dense(pm_c), dense(pm_u),
                    x.reshape(n, C, inner).float(), *params)


def _item_index(n, C, T, H, W):
    """The grid-stride item that owns each latent element [n, C, T, H, W]: 4 channels x 2 w per item in the 4 x 2 form, the
    dense index in the one-element form."""
    b, c, t, h, w = torch.meshgrid(*(torch.arange(d) for d in (n, C, T, H, W)), indexing="ij")
    if C == 4 and W % 2 == 0:             # (C_out is 2 C in every case here)
        return ((b * T + t) * H + h) * (W // 2) + w // 2
    return (((b * C + c) * T + t) * H + h) * W + w


def reference_step_patch(pm_c, pm_u, x, params, patch, Co, guided=3, mutant=None, dtype=torch.float64):
    """x_next [n, C, T, H, W] of one step: ``params`` = (cfg, 1 + k, A, Bc, abar_prev), every operation rounded to ``dtype``
    and nothing contracted (exact in fp64 on the S1 operands).  ``guided`` other than 3 is put together per channel from
    the two forms sampler_reference has: guidance on every channel, and on none (uncond := cond makes the guided value
    cond exactly)."""
    s = scase_of(pm_c, pm_u, x, params, patch, Co, swapped=mutant == "hw_swapped")
    inner_mutant = mutant if mutant in fe.SAMPLER_MUTANTS and mutant != "second_pass_missing" else None
    if guided == 3 or mutant is not None:
        assert guided == 3
        out = fe.sampler_reference(s, inner_mutant, dtype)
    else:
        on = fe.sampler_reference(s, "cfg_all_channels", dtype)
        off = fe.sampler_reference(dataclasses.replace(s, uncond=s.cond), None, dtype)
        c = torch.arange(s.C)[None, :, None]
        out = torch.where(c < guided, on, off)
    out = out.reshape(x.shape)
    if mutant == "second_pass_missing":
        out = torch.where(_item_index(*x.shape) < FIRST_PASS_ITEMS, out, torch.full_like(out, fe.NAN))
    return out


def s1_patch(shape, params):
    """The S1 operands of fp_edge_cases for a shape of t2v_dpm_cases.SHAPES in the patch-major layout: (pm_c, pm_u, x
    [n, C, T, H, W], the dense case with its fp64-exact result).  The sigma channels of the model outputs are NaN."""
    n, C, Co, T, H, W, patch, _ = shape
    assert Co == 2 * C
    s = fe.s1(n, C, T * H * W, params)
    pm_c = tc.patchify(s.cond.reshape(n, Co, T, H, W), patch)
    pm_u = tc.patchify(s.uncond.reshape(n, Co, T, H, W), patch)
    return pm_c, pm_u, s.x.reshape(n, C, T, H, W), s

"""Cases of the STDiT DPM-Solver++ scheduler (t2v/dpm_solver.py) and its patch-major step (vq_cfg_dpmpp_step_patch): the
analytic video noise model and the toy text encoder the golden trajectories were recorded with
(tests/golden/make_golden_t2v_dpms.py), the kernel's index map and per-element arithmetic in NumPy, and the shape table.

The analytic model uses additions, multiplications and one division only, so that its CPU output is the same bits on
every machine (no transcendental, no reduction whose order a vector width could change)."""
import numpy as np
import torch

import dpm_step_cases as dc

Z_SIZE = (4, 2, 4, 6)                                     # latent [C, T, H, W] of the golden trajectories (n = 2)
PATCH = (1, 2, 2)
C_OUT = 8
PROMPTS = ["a", "b"]
STEPS = (1, 2, 3, 20)
CFGS = (4.0, 7.0)
SEED = 123

# (n, C, C_out, T, H, W, patch, pad): pad = elements added to the dense sample pitch.  The first six rows are the issue's;
# in this kernel one thread owns 4 channels x 2 w (1024 x 256 threads per pass of the grid), so its sixth row runs 128
# blocks in one pass; the last two rows are the second pass of the 4 x 2 form and of the one-element form.
SHAPES = [
    (1, 4, 8, 1, 4, 4, (1, 2, 2), 0),
    (2, 4, 8, 2, 4, 6, (1, 2, 2), 0),
    (1, 4, 8, 4, 4, 4, (2, 2, 2), 0),
    (1, 3, 6, 2, 2, 2, (1, 1, 1), 0),
    (2, 4, 8, 3, 6, 10, (1, 2, 2), 8),
    (2, 4, 8, 16, 64, 64, (1, 2, 2), 0),
    (2, 4, 8, 17, 128, 128, (1, 2, 2), 0),
    (1, 3, 6, 3, 300, 301, (1, 1, 1), 0),
]


def shape_id(s):
    return "n%d_C%d_Co%d_T%d_H%d_W%d_p%d%d%d_pad%d" % (s[:6] + tuple(s[6]) + (s[7],))


class ToyTextEncoder:
    """encode(prompts) -> dict(y [n, 1, L, Cc], mask [n, L]); null(n) -> [n, 1, L, Cc].  Seeded, fp16-representable."""
    L, Cc = 3, 4

    def __init__(self, device="cpu"):
        g = torch.Generator().manual_seed(SEED + 1)
        self.table = (torch.randn(8, 1, self.L, self.Cc, generator=g) * 0.5).half().float().to(device)
        self.y_null = (torch.randn(1, 1, self.L, self.Cc, generator=g) * 0.25).half().float().to(device)

    def encode(self, prompts):
        n = len(prompts)
        mask = torch.ones(n, self.L, dtype=torch.int64, device=self.table.device)
        mask[:, -1] = 0
        return dict(y=self.table[:n].clone(), mask=mask)

    def null(self, n):
        return self.y_null.expand(n, -1, -1, -1).clone()


def analytic_eps(x, t, y):
    """[B, C_OUT, T, H, W] fp32 of the analytic model: the first C channels a noise prediction that moves with the
    model-input time, the condition and the channel; the learned-sigma half something else entirely."""
    x = x.float()
    B = x.shape[0]
    sh = (B, 1, 1, 1, 1)
    w = (0.125 + t.float() / 2048.0).reshape(sh)
    c = y.float()[:, 0, 0, 0].reshape(sh)
    ch = (1.0 + 0.125 * torch.arange(x.shape[1], dtype=torch.float32, device=x.device)).reshape(1, -1, 1, 1, 1)
    eps = x * w * ch + 0.25 * c + 0.0078125 * (x * c)
    return torch.cat([eps, -2.0 * x + 3.0], dim=1)


def patchify(out, patch):
    """The inverse of STDiT.unpatchify: [B, C_out, T, H, W] -> [B, N_t*N_h*N_w, p_t*p_h*p_w*C_out]."""
    B, Co, T, H, W = out.shape
    pt, ph, pw = patch
    v = out.reshape(B, Co, T // pt, pt, H // ph, ph, W // pw, pw).permute(0, 2, 4, 6, 3, 5, 7, 1)
    return v.reshape(B, (T // pt) * (H // ph) * (W // pw), pt * ph * pw * Co).contiguous()


class AnalyticSTDiT:
    """The part of the STDiT interface the schedulers use, around analytic_eps.  ``calls``: a list that receives
    (x, t, y, mask) of every forward.  ``dtype``: the type final_layer's output has (what patch_major=True returns)."""
    cfg_split = False

    def __init__(self, calls=None, dtype=torch.float32, patch=PATCH):
        self.calls, self.dtype, self.patch_size, self.out_channels = calls, dtype, patch, C_OUT

    def forward(self, x, timestep, y, mask=None, patch_major=False):
        if self.calls is not None:
            self.calls.append((x.detach().clone(), timestep.detach().clone(), y.detach().clone(), mask))
        out = analytic_eps(x.to(self.dtype), timestep, y).to(self.dtype)
        if patch_major:
            return patchify(out, self.patch_size)
        return out.to(torch.float32)

    def unpatchify(self, pm):
        """STDiT.unpatchify for this model's patch: [B, tokens, columns] -> [B, C_OUT, T, H, W]."""
        pt, ph, pw = self.patch_size
        _, T, H, W = Z_SIZE
        v = pm.reshape(pm.shape[0], T // pt, H // ph, W // pw, pt, ph, pw, C_OUT).permute(0, 7, 1, 4, 2, 5, 3, 6)
        return v.reshape(pm.shape[0], C_OUT, T, H, W)

    __call__ = forward


# ---------------------------------------------------------------------------------------------- the kernel, in NumPy
def patch_index(b, c, t, h, w, T, H, W, Co, patch):
    """(sample, token, column) of latent element (b, c, t, h, w): include/viditq.h, vq_cfg_dpmpp_step_patch.  Arrays."""
    pt, ph, pw = patch
    Nh, Nw = H // ph, W // pw
    token = ((t // pt) * Nh + h // ph) * Nw + w // pw
    column = (((t % pt) * ph + h % ph) * pw + w % pw) * Co + c
    return b, token, column


def gather(eps_pm, C, T, H, W, Co, patch):
    """[n, C, T, H, W] read from a patch-major array [n, tokens, columns] through patch_index."""
    n = eps_pm.shape[0]
    b, c, t, h, w = np.meshgrid(np.arange(n), np.arange(C), np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    bi, tok, col = patch_index(b, c, t, h, w, T, H, W, Co, patch)
    return eps_pm[bi, tok, col]


def reference_step_patch(row, eps_u, eps_c, x, hist, k, patch, Co, div_form="reciprocal"):
    """One patch-major step number k: eps_u / eps_c [n, tokens, columns] of any float type, widened to fp32 first; every
    operation fp32 (dpm_step_cases._tree with no fp16 rounding); ``div_form`` 'reciprocal' is the kernel's (and torch's on
    a GPU) product with RN(1 / alpha_t), 'divide' what torch computes on the CPU.  Returns (x_out [n, C, T, H, W], hist_new)."""
    n, C, T, H, W = x.shape
    u = gather(np.asarray(eps_u).astype(np.float32), C, T, H, W, Co, patch)
    c = gather(np.asarray(eps_c).astype(np.float32), C, T, H, W, Co, patch)
    out, hist = dc.reference_step(row, np.concatenate([u, c]).reshape(2 * n, C, -1), x.reshape(n, C, -1), hist, k, False,
                                  div_form)
    return out.reshape(x.shape), hist

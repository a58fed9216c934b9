"""Tensor-level wrappers of vq_cfg_dpmpp_step_patch2d, vq_cfg_ddpm_step_patch2d and vq_cfg_sa_step_patch2d
(include/viditq.h): the three PixArt sampler steps on the patch-major output of ``forward(patch_major=True)``.

Reached as ``ops.cfg_*_step_patch2d`` / ``ops.cfg_*_step_patch2d_ok`` (ops.py re-exports them at its end; import ``ops``,
not this module; they live here for the reason ops_kv.py gives).  Each takes the arguments of its dense sibling
(ops.cfg_dpmpp_step, ops.cfg_ddpm_step, ops.cfg_sa_step) with ``eps`` [2n, tokens, p*p*C_out] in place of the unpatchified
view; the patch extent follows from the token count.  Every operand check is ops.py's (``_step_front``, ``_req``).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib, ops
from ._lib import check

GRID_MAX = 65535                 # csrc/sampler.hip: samples and token rows are grid extents


def _geometry(eps, x, elem_mult):
    """(n, C, C_out, H, W, p, ld_eps) of a patch2d step, or None when ``eps`` is not the final_layer output [2n, (H/p)*(W/p),
    p*p*C_out] (a sample dense, the sample pitch free) of a square patch p for the dense latent ``x`` [n, C, H, W], or holds
    fewer than elem_mult * C channels per patch position.  Shapes and strides only (no tensor is touched)."""
    es, xs = tuple(int(d) for d in eps.shape), tuple(int(d) for d in x.shape)
    if len(xs) != 4 or len(es) != 3 or min(es + xs) <= 0 or es[0] != 2 * xs[0]:
        return None
    n, Cc, H, W = xs
    p = math.isqrt(H * W // es[1])
    if p <= 0 or H % p or W % p or es[1] * p * p != H * W or es[2] % (p * p) or elem_mult * Cc * p * p > es[2]:
        return None
    if tuple(x.stride()) != ops._dense_strides(xs) or tuple(eps.stride())[1:] != (es[2], 1):
        return None
    return n, Cc, es[2] // (p * p), H, W, p, int(eps.stride()[0])


def _ok(eps, x, elem_mult) -> bool:
    """The refusals of a patch2d entry point (include/viditq.h) that depend on eps and x, asked before the launch from
    shapes, strides and addresses: GPU tensors, fp32 x, fp16 / fp32 eps and p of 1 or 2 (VQ_EUNSUP), positive extents
    (VQ_EINVAL), and VQ_ESHAPE: the layout, elem_mult * C <= C_out, ld_eps >= H*W*C_out, the grid extents, both addresses
    on their own element (an address or pitch that is on no more selects the one-element form; it is not refused)."""
    if not (eps.is_cuda and x.is_cuda):
        return False
    if x.dtype != torch.float32 or eps.dtype not in (torch.float16, torch.float32):
        return False
    geo = _geometry(eps, x, elem_mult)
    if geo is None:
        return False
    n, Cc, Co, H, W, p, ld = geo
    return (p in (1, 2) and ld >= H * W * Co and n <= GRID_MAX and H // p <= GRID_MAX
            and eps.data_ptr() % eps.element_size() == 0 and x.data_ptr() % 4 == 0)


def cfg_dpmpp_step_patch2d_ok(eps, x) -> bool:
    """Whether vq_cfg_dpmpp_step_patch2d takes a patch-major model output ``eps`` and a latent ``x`` [n, C, H, W] (_ok)."""
    return _ok(eps, x, 1)


def cfg_ddpm_step_patch2d_ok(eps, x) -> bool:
    """Whether vq_cfg_ddpm_step_patch2d takes them (_ok): the variance channels make it 2C <= C_out."""
    return _ok(eps, x, 2)


def cfg_sa_step_patch2d_ok(eps, x) -> bool:
    """Whether vq_cfg_sa_step_patch2d takes them (_ok)."""
    return _ok(eps, x, 1)


_LAYOUT = "the patch-major [2n, (H/p)*(W/p), p*p*C_out]"


def cfg_dpmpp_step_patch2d(eps: torch.Tensor, x: torch.Tensor, hist: torch.Tensor, coef: torch.Tensor, row: int,
                           step: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None,
                           x_model: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.cfg_dpmpp_step on the (uncond | cond) patch-major output ``eps`` [2n, tokens, p*p*C_out] of one
    ``forward(patch_major=True)`` (vq_cfg_dpmpp_step_patch2d): bit for bit cfg_dpmpp_step on ``unpatchify(eps)[:, :C]``,
    without that copy.  ``x`` [n, C, H, W]; every other argument as there."""
    bad = hist.numel() != 3 * x.numel() or coef.dim() != 2 or coef.shape[1] != _lib.DPMPP_ROW
    n, Cc, Co, H, W, p, ld, x_out, xm16 = ops._step_front(
        eps, x, hist, "hist", coef, 1, _LAYOUT,
        (bad, "hist must hold 3 x %d fp32 and coef rows of %d floats" % (x.numel(), _lib.DPMPP_ROW)), step, x_out, x_model,
        geometry=_geometry)
    P = ops._p
    check(ops._L().vq_cfg_dpmpp_step_patch2d(P(eps), P(x), P(hist), P(coef), P(step), P(x_out), P(x_model), n, Cc, Co, H, W,
                                             p, ld, int(row), coef.shape[0], int(eps.dtype == torch.float16), xm16,
                                             ops._stream()), "vq_cfg_dpmpp_step_patch2d")
    return x_out


def cfg_ddpm_step_patch2d(eps: torch.Tensor, x: torch.Tensor, noise: torch.Tensor, coef: torch.Tensor, row: int,
                          step: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None,
                          x0_out: Optional[torch.Tensor] = None, x_model: Optional[torch.Tensor] = None,
                          guided: int = 3) -> torch.Tensor:
    """ops.cfg_ddpm_step on the (cond | uncond) patch-major output ``eps`` [2n, tokens, p*p*C_out], C_out >= 2C, of one
    ``forward(patch_major=True)`` (vq_cfg_ddpm_step_patch2d): bit for bit cfg_ddpm_step on ``unpatchify(eps)``, without
    that copy.  ``x`` and ``noise`` [n, C, H, W]; every other argument as there."""
    bad = noise.shape != x.shape or coef.dim() != 2 or coef.shape[1] != _lib.DDPM_ROW
    n, Cc, Co, H, W, p, ld, x_out, xm16 = ops._step_front(
        eps, x, noise, "noise", coef, 2, _LAYOUT,
        (bad, "noise must have x's shape and coef rows of %d floats" % _lib.DDPM_ROW), step, x_out, x_model,
        geometry=_geometry)
    if x0_out is not None:
        ops._req(x0_out, torch.float32, "x0_out")
        assert x0_out.shape == x.shape
    P = ops._p
    check(ops._L().vq_cfg_ddpm_step_patch2d(P(eps), P(x), P(noise), P(coef), P(step), P(x_out), P(x0_out), P(x_model), n, Cc,
                                            Co, H, W, p, ld, int(guided), int(row), coef.shape[0],
                                            int(eps.dtype == torch.float16), xm16, ops._stream()),
          "vq_cfg_ddpm_step_patch2d")
    return x_out


def cfg_sa_step_patch2d(eps: torch.Tensor, x: torch.Tensor, xp: torch.Tensor, hist: torch.Tensor, noise: torch.Tensor,
                        coef: torch.Tensor, row: int, step: Optional[torch.Tensor] = None,
                        x_out: Optional[torch.Tensor] = None, xp_out: Optional[torch.Tensor] = None,
                        x_model: Optional[torch.Tensor] = None):
    """ops.cfg_sa_step on the (uncond | cond) patch-major output ``eps`` [2n, tokens, p*p*C_out] of one
    ``forward(patch_major=True)`` (vq_cfg_sa_step_patch2d): bit for bit cfg_sa_step on ``unpatchify(eps)[:, :C]``, without
    that copy.  ``x`` and ``xp`` [n, C, H, W]; every other argument as there.  Returns (x_out, xp_out)."""
    for t, name in ((xp, "xp"), (noise, "noise")):
        ops._req(t, torch.float32, name)
    bad = (hist.numel() != 2 * x.numel() or noise.numel() != 2 * x.numel() or xp.shape != x.shape or coef.dim() != 2
           or coef.shape[1] != _lib.SA_ROW)
    n, Cc, Co, H, W, p, ld, x_out, xm16 = ops._step_front(
        eps, x, hist, "hist", coef, 1, _LAYOUT,
        (bad, "xp must have x's shape, hist and the noise ring must hold 2 x %d fp32 and coef rows of %d floats"
              % (x.numel(), _lib.SA_ROW)), step, x_out, x_model, geometry=_geometry)
    if xp_out is None:
        xp_out = torch.empty_like(x)
    else:
        ops._req(xp_out, torch.float32, "xp_out")
        assert xp_out.shape == x.shape
    P = ops._p
    check(ops._L().vq_cfg_sa_step_patch2d(P(eps), P(x), P(xp), P(hist), P(noise), P(coef), P(step), P(x_out), P(xp_out),
                                          P(x_model), n, Cc, Co, H, W, p, ld, int(row), coef.shape[0],
                                          int(eps.dtype == torch.float16), xm16, ops._stream()), "vq_cfg_sa_step_patch2d")
    return x_out, xp_out

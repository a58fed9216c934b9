"""Tensor-level wrapper of vq_patch_embed_f16 (include/viditq.h): the patch embedding's gather, Linear and position-embedding
add in one launch (csrc/patch_embed.hip).

Reached as ``ops.patch_embed_f16`` / ``ops.patch_embed_f16_ok`` (ops.py re-exports both at its end; import ``ops``, not
this module; they live here for the reason ops_kv.py gives).  Every operand check is the one of ops.py (``_req``,
``_req_gpu``, ``_req_rows``, ``_req_opt``).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from ._lib import VQError, check

PATCH_MAX_C, PATCH_MAX_K = 1536, 32      # csrc/patch_embed.hip: PE_MAX_C, PE_MAX_K


def patch_embed_f16_ok(B: int, Cin: int, D: int, H: int, W: int, patch: Sequence[int], Cc: int, pos_rows: Optional[int],
                       ldw: int) -> bool:
    """Whether vq_patch_embed_f16 takes this launch: every refusal of the entry point (include/viditq.h) that these
    arguments decide, mirrored for callers that choose a route BEFORE they launch - a refused shape keeps the launches it
    would replace, it does not raise.  ``pos_rows``: None without a position table.  (The pointers, their alignment and
    the latent's type stay with the entry point.)"""
    pt, ph, pw = patch
    if min(B, Cin, D, H, W, pt, ph, pw, Cc, ldw) <= 0 or (pos_rows is not None and pos_rows <= 0):      # VQ_EINVAL
        return False
    if D % pt or H % ph or W % pw:                                                                       # VQ_ESHAPE
        return False
    K = Cin * pt * ph * pw
    if K % 8 or K > PATCH_MAX_K or Cc % 16 or Cc > PATCH_MAX_C or B * Cin * D * H * W >= 1 << 31:
        return False
    if pos_rows is not None and ((D // pt) * (H // ph) * (W // pw)) % pos_rows:
        return False
    return not (ldw % 8 or ldw < K)                                                                      # the pitch


def patch_embed_f16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None,
                    patch: Sequence[int] = (1, 2, 2)) -> torch.Tensor:
    """out [B, N, C] fp16 = patchify(x).half() @ w.T + bias (+ pos[n % pos_rows]): x a dense latent [B, Cin, H, W] or
    [B, Cin, D, H, W], fp32 or fp16 (fp32 is rounded to fp16 first); w [C, K] fp16, K = Cin pt ph pw in the flatten order of
    the Conv weight (rows may be strided); bias [C] fp16 or None; pos [..., pos_rows, C] fp16 or None; ``patch`` (pt, ph, pw)
    or (ph, pw).  Tokens run row-major over (D / pt, H / ph, W / pw).  Bit for bit what ``linear_f16`` of the patchified
    fp16 latent followed by torch's fp16 ``+ pos`` returns.  A launch ``patch_embed_f16_ok`` refuses raises."""
    ops._req_gpu(x, "x")
    if x.dtype not in (torch.float16, torch.float32) or not x.is_contiguous() or x.dim() not in (4, 5):
        raise VQError("patch_embed_f16: x must be a dense fp16 or fp32 latent [B, Cin, (D,) H, W]")
    ops._req_rows(w, torch.float16, "w")
    ops._req_opt(bias, torch.float16, "bias")
    ops._req_opt(pos, torch.float16, "pos")
    patch = tuple(int(p) for p in patch)
    if len(patch) == 2:
        patch = (1,) + patch
    B, Cin = x.shape[0], x.shape[1]
    D, H, W = (1,) * (5 - x.dim()) + tuple(x.shape[2:])
    if w.dim() != 2 or len(patch) != 3 or min(patch) <= 0 or w.shape[1] != Cin * patch[0] * patch[1] * patch[2]:
        raise VQError("patch_embed_f16: w [C, Cin * pt * ph * pw] and patch (pt, ph, pw)")
    Cc = w.shape[0]
    if (bias is not None and bias.numel() != Cc) or (pos is not None and (pos.dim() < 2 or pos.shape[-1] != Cc)):
        raise VQError("patch_embed_f16: bias must be [C] and pos [pos_rows, C]")
    pos_rows = None if pos is None else pos.numel() // Cc
    if not patch_embed_f16_ok(B, Cin, D, H, W, patch, Cc, pos_rows, w.stride(0)):
        raise VQError("patch_embed_f16: a shape vq_patch_embed_f16 refuses (patch_embed_f16_ok)")
    N = (D // patch[0]) * (H // patch[1]) * (W // patch[2])
    out = torch.empty((B, N, Cc), dtype=torch.float16, device=x.device)
    p = ops._p
    check(ops._L().vq_patch_embed_f16(p(x), int(x.dtype == torch.float32), p(w), p(bias), p(pos), p(out), B, Cin, D, H, W,
                                      patch[0], patch[1], patch[2], Cc, pos_rows or 0, w.stride(0), ops._stream()),
          "vq_patch_embed_f16")
    return out

"""Tensor-level wrappers of vq_final_layer_f16 and vq_final_layer_i8 (include/viditq.h): T2IFinalLayer's LayerNorm +
modulate + Linear in one launch, for an FP Linear (csrc/final_layer.hip) and for a quantized one (csrc/final_layer_i8.hip).

Reached as ``ops.final_layer_f16`` / ``ops.final_layer_f16_ok`` / ``ops.final_layer_i8`` / ``ops.final_layer_i8_ok`` (ops.py
re-exports them at its end; import ``ops``, not this module; they live here for the reason ops_kv.py gives).  Every operand check is the one of ops.py (``_req``,
``_req_rows``, ``_req_opt``).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from ._lib import VQError, check

FINAL_MAX_C, FINAL_MAX_N = 1536, 64      # csrc/final_layer.hip: FL_MAX_C, FL_MAX_N


def _row_pitch(x3) -> Optional[int]:
    """The one pitch between all B * n_tok rows of x3 [B, n_tok, C] (dense last dimension), or None."""
    B, n_tok = x3.shape[0], x3.shape[1]
    sb, st, sc = x3.stride()
    if sc != 1 or (B > 1 and n_tok > 1 and sb != n_tok * st):
        return None
    return st if n_tok > 1 else sb


def final_layer_f16_ok(M: int, rows_per_sample: int, Cc: int, N: int, ldx: int, ldw: int) -> bool:
    """Whether vq_final_layer_f16 takes this launch: every refusal of the entry point (include/viditq.h) that these six
    arguments decide, mirrored for callers that choose a route BEFORE they launch - a refused shape keeps the two
    launches, it does not raise.  (The pointers and their alignment stay with the entry point.)"""
    if min(M, rows_per_sample, Cc, N, ldx, ldw) <= 0 or M % rows_per_sample:           # VQ_EINVAL
        return False
    if Cc % 32 or Cc > FINAL_MAX_C or N % 16 or N > FINAL_MAX_N:                       # VQ_ESHAPE: the shapes served
        return False
    return not (ldx % 8 or ldw % 8 or ldx < Cc or ldw < Cc)                            # VQ_ESHAPE: the pitches


def final_layer_f16(x3: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float, w: torch.Tensor,
                    bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [B, n_tok, N] fp16 = Linear(fp16(LN(x3) * (1 + scale) + shift)): x3 [B, n_tok, C] fp16 (rows may be strided),
    shift / scale [B, C] fp32 as ``adaln_table`` returns them, w [N, C] fp16 (rows may be strided), bias [N] fp16 or None;
    LayerNorm without affine in fp32, fp32 accumulation.  What ``linear_f16(ln_modulate_rowquant(x3, shift, scale, eps,
    want_xm=True)[1], w, bias)`` returns up to the order of the fp32 sums.  A launch ``final_layer_f16_ok`` refuses raises."""
    ops._req_rows(x3, torch.float16, "x3")
    ops._req_rows(w, torch.float16, "w")
    ops._req(shift, torch.float32, "shift")
    ops._req(scale, torch.float32, "scale")
    ops._req_opt(bias, torch.float16, "bias")
    if x3.dim() != 3 or w.dim() != 2 or w.shape[1] != x3.shape[2]:
        raise VQError("final_layer_f16: x3 [B, n_tok, C] and w [N, C]")
    B, n_tok, Cc = x3.shape
    N = w.shape[0]
    ldx = _row_pitch(x3)
    if ldx is None:
        raise VQError("final_layer_f16: the rows of x3 must be one pitch apart")
    if shift.numel() != B * Cc or scale.numel() != B * Cc or (bias is not None and bias.numel() != N):
        raise VQError("final_layer_f16: shift / scale must be [B, C] and bias [N]")
    out = torch.empty((B, n_tok, N), dtype=torch.float16, device=x3.device)
    p = ops._p
    check(ops._L().vq_final_layer_f16(p(x3), p(shift), p(scale), float(eps), p(w), p(bias), p(out), B * n_tok, n_tok, Cc, N,
                                      ldx, w.stride(0), ops._stream()), "vq_final_layer_f16")
    return out


FINAL_I8_BATCHES = (1, 2, 4, 8, 16)      # csrc/final_layer_i8.hip: samples whose rows of one token share a 16-row tile


def final_layer_i8_ok(M: int, rows_per_sample: int, Cc: int, Kp: int, N: int, ldx: int, n_bits: int, w_bits: int) -> bool:
    """Whether vq_final_layer_i8 takes this launch: every refusal of the entry point (include/viditq.h) that these eight
    arguments decide, mirrored for callers that choose a route BEFORE they launch - a refused shape keeps the three
    launches, it does not raise.  (The pointers and their alignment stay with the entry point.)"""
    if min(M, rows_per_sample, Cc, Kp, N, ldx) <= 0 or M % rows_per_sample:            # VQ_EINVAL
        return False
    if Cc % 32 or Cc > FINAL_MAX_C or Kp != (Cc + 127) // 128 * 128 or N % 16 or N > FINAL_MAX_N:   # VQ_ESHAPE: the shapes
        return False
    if M // rows_per_sample not in FINAL_I8_BATCHES or ldx % 8 or ldx < Cc:            # VQ_ESHAPE: the batch, the pitch
        return False
    return 2 <= n_bits <= 8 and 2 <= w_bits <= 8                                       # VQ_EUNSUP


def final_layer_i8(x3: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float, pw, bias: Optional[torch.Tensor] = None,
                   s: Optional[torch.Tensor] = None, n_bits: int = 8, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [B, n_tok, N] fp16 = the quantized Linear ``pw`` (an ``ops.PackedWeight``) of fp16(LN(x3) * (1 + scale) + shift)
    on the Linear's dynamic per-token grid of ``n_bits``, shared over the B samples of a token: x3 [B, n_tok, C] fp16 (rows
    may be strided), shift / scale [B, C] fp32, bias [N] fp32 or None, s [C] fp32 the Linear's smoothing vector or None
    (its reciprocal form when ``ops.smooth_rcp`` has one, else the exact division), status the int32 word that receives
    VQ_ST_EPSFILL.  What ``gemm_i8(rowquant(ln_modulate_rowquant(x3, shift, scale, eps, want_xm=True)[1], n_bits, s=s,
    status=status), pw, bias)`` returns up to the order of the LayerNorm sums.  A launch ``final_layer_i8_ok`` refuses
    raises."""
    ops._req_rows(x3, torch.float16, "x3")
    ops._req(shift, torch.float32, "shift")
    ops._req(scale, torch.float32, "scale")
    ops._req_gpu(pw.wq, "pw.wq")
    ops._req_opt(bias, torch.float32, "bias")
    ops._req_opt(s, torch.float32, "s")
    ops._req_opt(status, torch.int32, "status")
    if x3.dim() != 3 or pw.K != x3.shape[2]:
        raise VQError("final_layer_i8: x3 [B, n_tok, C] and a weight packed for C")
    B, n_tok, Cc = x3.shape
    ldx = _row_pitch(x3)
    if ldx is None:
        raise VQError("final_layer_i8: the rows of x3 must be one pitch apart")
    if shift.numel() != B * Cc or scale.numel() != B * Cc or (bias is not None and bias.numel() != pw.N) or (
            s is not None and s.numel() != Cc):
        raise VQError("final_layer_i8: shift / scale must be [B, C], bias [N] and s [C]")
    s_rcp = ops._rcp_or_none(s)
    if s_rcp is ops._NO_RCP:
        s_rcp = None                                      # no exact reciprocal form: the kernel divides
    out = torch.empty((B, n_tok, pw.N), dtype=torch.float16, device=x3.device)
    p = ops._p
    check(ops._L().vq_final_layer_i8(p(x3), p(shift), p(scale), float(eps), p(s), p(s_rcp), *ops._weight_ptrs(pw), p(bias),
                                     p(out), p(status), B * n_tok, n_tok, Cc, pw.Kp, pw.N, ldx, n_bits, pw.n_bits,
                                     ops._stream()), "vq_final_layer_i8")
    return out

"""Tensor-level wrappers of vq_rowquant_batch (include/viditq.h): the per-token dynamic quantizers of a batched forward of
3 to 16 samples - plain / smoothed, behind GELU, behind LayerNorm + modulate - from one pass over the rows, a token's grid
shared by its B rows.

Reached as ``ops.rowquant_batch`` / ``ops.gelu_rowquant_batch`` / ``ops.ln_modulate_rowquant_batch`` / ``ops.rowquant_batch_ok``
(ops.py re-exports them at its end; import ``ops``, not this module).  They live in a module of their own because
tests/test_abi_cpu.py and tests/helpers.py::trace_ops enumerate the functions DEFINED in ops.py against fixed lists; the
CPU-tensor refusal of these wrappers is in tests/test_rowquant_batch_cpu.py.  Every operand check, allocation and pointer
table is the one of ops.py.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import ops
from ._lib import VQError, check

BATCH_MIN_B, BATCH_MAX_B = 3, 16     # csrc/rowquant_batch.hip: below, the B = 1 / B = 2 kernels; RQB_MAX_B
BATCH_MAX_KP = 4608                  # RQB_MAX_KP
BATCH_LN_MAX_KP = 1536               # RQB_LN_MAX_KP: the LayerNorm arm keeps the modulated row in fp32 registers


def rowquant_batch_ok(B: int, C: int, Kp: int, n_bits: int, n_out: int, act: int = 0, ln: bool = False) -> bool:
    """Whether vq_rowquant_batch takes this launch: the entry point's refusals that these arguments decide, in its order,
    mirrored for callers that choose a route BEFORE they launch - a refused launch takes the calls it would replace.  (The
    pointers and their alignment stay with the entry point; torch allocations are 16-byte aligned.)"""
    if n_out < 1 or min(B, C) <= 0 or act not in (0, 1) or (act == 1 and ln):      # VQ_EINVAL
        return False
    if C % 8 or Kp % 128 or Kp < C:                                                  # VQ_ESHAPE
        return False
    if not 2 <= n_bits <= 8:                                                         # VQ_EUNSUP: the code width
        return False
    if B > BATCH_MAX_B:                                                              # VQ_ESHAPE
        return False
    return B >= BATCH_MIN_B and Kp <= BATCH_MAX_KP and n_out <= 3 and not (n_out > 1 and act == 1) and not (
        ln and Kp > BATCH_LN_MAX_KP)                                                 # VQ_EUNSUP


def _launch(who: str, x3: torch.Tensor, n_bits: int, smooth: Sequence[Optional[torch.Tensor]], status, act: int = 0,
            shift=None, scale=None, eps: float = 0.0, want_xm: bool = False):
    """One vq_rowquant_batch launch -> ([QAct per entry of ``smooth``], xm or None)."""
    ops._req(x3, torch.float16, "x")
    if x3.dim() != 3:
        raise VQError("%s: x must be [B, n_tok, C]" % who)
    B, n_tok, Cc = x3.shape
    Kp = ops.pad128(Cc)
    smooth = list(smooth)
    ln = shift is not None or scale is not None
    if ln:
        ops._req(shift, torch.float32, "shift")
        ops._req(scale, torch.float32, "scale")
        if shift.numel() != B * Cc or scale.numel() != B * Cc:
            raise VQError("%s: shift / scale must be [B, C]" % who)
    for sm in smooth:
        if sm is not None:
            ops._req(sm, torch.float32, "smooth")
            if sm.numel() != Cc:
                raise VQError("%s: one smoothing entry per channel" % who)
    ops._req_opt(status, torch.int32, "status")
    if not rowquant_batch_ok(B, Cc, Kp, n_bits, len(smooth), act, ln):
        raise VQError("%s: B %d, C %d, %d bits, %d outputs is not a launch of vq_rowquant_batch (rowquant_batch_ok)" % (
            who, B, Cc, n_bits, len(smooth)))
    # a vector without an exact reciprocal form (or unseen under graph capture): no reciprocal, the kernel divides
    rcps = [None if r is ops._NO_RCP else r for r in (ops._rcp_or_none(sm) for sm in smooth)]
    outs = [ops._qact_empty(B * n_tok, Kp, Cc, n_bits, x3.device) for _ in smooth]
    xm = torch.empty_like(x3) if want_xm else None
    keep = ops._tables(smooth, rcps) + ops._qact_tables(outs)
    p = ops._p
    check(ops._L().vq_rowquant_batch(p(x3), p(shift), p(scale), float(eps), act, len(smooth), *ops._void(keep), p(xm), B, n_tok,
                                     Cc, Kp, n_bits, p(status), ops._stream()), "vq_rowquant_batch")
    return outs, xm


def rowquant_batch(x3: torch.Tensor, n_bits: int = 8, smooth: Sequence[Optional[torch.Tensor]] = (None,),
                   status: Optional[torch.Tensor] = None) -> List[ops.QAct]:
    """One QAct of x3 [B, n_tok, C] fp16, 3 <= B <= 16, per entry of ``smooth`` (a vector [C] fp32, or None: no division):
    output j is ``ops.rowquant(x3, n_bits, s=smooth[j])``, bit for bit, from one pass over the rows."""
    return _launch("rowquant_batch", x3, n_bits, smooth, status)[0]


def gelu_rowquant_batch(h3: torch.Tensor, n_bits: int = 8, s: Optional[torch.Tensor] = None,
                        status: Optional[torch.Tensor] = None) -> ops.QAct:
    """GELU(tanh), rounded to fp16, then the per-token quantizer of the PRE-activation h3 [B, n_tok, C] fp16 behind ``s``:
    ``ops.gelu_rowquant`` for 3 <= B <= 16."""
    return _launch("gelu_rowquant_batch", h3, n_bits, [s], status, act=1)[0][0]


def ln_modulate_rowquant_batch(x3: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float = 1e-6,
                               smooth: Sequence[Optional[torch.Tensor]] = (None,), n_bits: int = 8,
                               status: Optional[torch.Tensor] = None, want_xm: bool = False):
    """LayerNorm (no affine) + (1 + scale[b]) * y + shift[b] + one per-token quantizer per entry of ``smooth``, for x3
    [B, n_tok, C] fp16 with 3 <= B <= 16 and C <= 1536; ``want_xm``: also the modulated activation, (outs, xm)."""
    if shift is None or scale is None:
        raise VQError("ln_modulate_rowquant_batch: shift and scale come together")
    outs, xm = _launch("ln_modulate_rowquant_batch", x3, n_bits, smooth, status, shift=shift, scale=scale, eps=eps,
                       want_xm=want_xm)
    return (outs, xm) if want_xm else outs

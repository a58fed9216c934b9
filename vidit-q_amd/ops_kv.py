"""Tensor-level wrapper of vq_kv_compress (include/viditq.h): PixArt-Sigma key / value compression and the q / k
LayerNorms on the q | k | v buffer of the fused qkv GEMM, in one launch.

Reached as ``ops.kv_compress`` / ``ops.kv_compress_ok`` (ops.py re-exports both at its end; import ``ops``, not this
module).  The two live in a module of their own because tests/test_abi_cpu.py and tests/helpers.py::trace_ops enumerate
the functions DEFINED in ops.py against fixed lists; the CPU-tensor refusal of this wrapper is in
tests/test_kv_compress_cpu.py.  Every operand check is the one of ops.py (``_req``, ``_req_rows``, ``_req_opt``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, ops
from ._lib import VQError, check

KV_MAX_C = 2048                  # csrc/kv_compress.hip: KVC_MAX_C (four 16-byte pieces per lane)
_MODES = {"conv": _lib.KVC_CONV, "uniform": _lib.KVC_PICK, "ave": _lib.KVC_PICK, "uniform_every": _lib.KVC_PICK_FLAT}


def kv_compress_ok(C: int, H: int, W: int, sr: int, sampling, ld: int) -> bool:
    """Whether vq_kv_compress takes this launch: the entry point's refusals that these six arguments decide, mirrored for
    callers that choose a route BEFORE they launch - a refused shape takes the torch sequence, it does not raise.  (The
    pointers and their alignment stay with the entry point; torch allocations are 16-byte aligned.)"""
    if sampling not in _MODES or min(C, H, W, sr, ld) <= 0:                 # VQ_EUNSUP (mode) / VQ_EINVAL
        return False
    if C % 8 or ld % 8 or ld < 3 * C:                                       # VQ_ESHAPE
        return False
    if (H * W) % sr if sampling == "uniform_every" else (H % sr or W % sr):  # VQ_ESHAPE
        return False
    return sr in (2, 4) and C <= KV_MAX_C                                   # VQ_EUNSUP


def _ln(ln, Cc: int, name: str):
    """(weight, bias, eps) of an affine LayerNorm given as that triple (fp32 [C] vectors), or three Nones."""
    if ln is None:
        return None, None, 0.0
    w, b, eps = ln
    ops._req(w, torch.float32, name + ".weight")
    ops._req(b, torch.float32, name + ".bias")
    if w.numel() != Cc or b.numel() != Cc:
        raise VQError("kv_compress: %s holds one weight and one bias per channel" % name)
    return w, b, float(eps)


def kv_compress(qkv: torch.Tensor, B: int, H: int, W: int, C: int, sr: int, sampling: str,
                sr_weight: Optional[torch.Tensor] = None, sr_bias: Optional[torch.Tensor] = None, norm=None, k_norm=None,
                q_norm=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """qkv [B*H*W, >= 3C] fp16 (q | k | v column blocks, rows may be strided) -> dense (k', v') [B*Lk, C] fp16: the key /
    value tokens of ``AttentionKVCompress.downsample_2d`` for ``sampling`` in ('conv', 'uniform', 'ave', 'uniform_every') at
    factor ``sr``.  'conv': ``sr_weight`` [C, 1, sr, sr] / ``sr_bias`` [C] fp32 and ``norm`` = (weight, bias, eps), fp32
    arithmetic, rounded to fp16 once.  ``k_norm`` = (weight, bias, eps): every k row is normalised (and rounded to fp16)
    before it is compressed; ``q_norm``: the q columns of ``qkv`` are normalised IN PLACE.  A shape ``kv_compress_ok``
    refuses raises."""
    ops._req_rows(qkv, torch.float16, "qkv")
    if qkv.dim() != 2 or qkv.shape[0] != B * H * W or qkv.shape[1] < 3 * C:
        raise VQError("kv_compress: qkv must be [B*H*W, >= 3C]")
    if sampling not in _MODES:
        raise VQError("kv_compress: sampling is one of %r" % (sorted(_MODES),))
    mode = _MODES[sampling]
    conv = mode == _lib.KVC_CONV
    if conv:
        if sr_weight is None or sr_bias is None or norm is None:
            raise VQError("kv_compress: 'conv' takes sr_weight, sr_bias and norm")
        ops._req(sr_weight, torch.float32, "sr_weight")
        ops._req(sr_bias, torch.float32, "sr_bias")
        if sr_weight.numel() != C * sr * sr or sr_bias.numel() != C:
            raise VQError("kv_compress: sr_weight must be [C, 1, sr, sr] and sr_bias [C]")
    nw, nb, neps = _ln(norm if conv else None, C, "norm")
    kw, kb, keps = _ln(k_norm, C, "k_norm")
    qw, qb, qeps = _ln(q_norm, C, "q_norm")
    n_in = H * W
    Lk = n_in // sr if mode == _lib.KVC_PICK_FLAT else (H // sr) * (W // sr)
    k_out = torch.empty((B * max(Lk, 0), C), dtype=torch.float16, device=qkv.device)
    v_out = torch.empty_like(k_out)
    p = ops._p
    check(ops._L().vq_kv_compress(p(qkv), qkv.stride(0), p(sr_weight) if conv else None, p(sr_bias) if conv else None, p(nw),
                                  p(nb), neps, p(kw), p(kb), keps, p(qw), p(qb), qeps, p(k_out), p(v_out), B, H, W, C, sr, mode,
                                  ops._stream()), "vq_kv_compress")
    return k_out, v_out

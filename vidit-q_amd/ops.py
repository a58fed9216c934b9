"""Tensor-level wrappers over the C ABI (include/viditq.h).

PyTorch is plumbing here: device memory (torch tensors), the current HIP stream and nothing
else.  Every function enqueues one or a few HIP kernels on ``torch.cuda.current_stream()`` and
never synchronises.  There is no fallback path: a missing library or a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import EPI_GATE_RESID, EPI_GELU, EPI_NONE, EPI_RESID, VQError, check  # noqa: F401


def _L():
    return _lib.load()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------- operand checks
# One copy of each check, allocation and pointer table of the wrappers below.  All private: tests/helpers.py::trace_ops
# records every call of a public function of this module, the calls one public function makes to another included
# (pad128, smooth_rcp, packed_shapes), so a helper never calls pad128 - its caller passes Kp in.
def _req_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise VQError("%s must be a GPU tensor (no CPU fallback in the product path)" % name)
    return t


def _req(t: torch.Tensor, dtype, name: str):
    _req_gpu(t, name)
    if t.dtype != dtype:
        raise VQError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise VQError("%s must be contiguous" % name)
    return t


def _req_opt(t: Optional[torch.Tensor], dtype, name: str):
    """_req of an operand that may be absent."""
    return None if t is None else _req(t, dtype, name)


def _req_rows(t: torch.Tensor, dtype, name: str):
    """As _req, for an operand whose rows may be strided: only the last dimension has to be dense."""
    _req_gpu(t, name)
    if t.dtype != dtype:
        raise VQError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.stride(-1) != 1:
        raise VQError("%s must be contiguous in its last dimension" % name)
    return t


def _req_f16(*pairs):
    """(tensor, name) pairs of strided fp16 views: the kernel takes their pitches, so only the device and the type."""
    for t, n in pairs:
        if not t.is_cuda or t.dtype != torch.float16:
            raise VQError("%s must be a GPU fp16 tensor" % n)


def _flat_f32(t: torch.Tensor, name: str):
    """A calibrated grid term (delta or zp, any shape) as the dense fp32 vector the kernels read."""
    return _req(t.reshape(-1).contiguous(), torch.float32, name)


def _tensorwise_grid(delta: torch.Tensor, zp: torch.Tensor, who: str):
    """(delta, zp) of wrapper ``who``, which takes one value of each."""
    if delta.numel() != 1 or zp.numel() != 1:
        raise VQError("%s: a tensor-wise grid (one delta, one zero point)" % who)
    return delta, zp


def _attn_scale(D: int, scale: Optional[float]) -> float:
    return float(D) ** -0.5 if scale is None else float(scale)


def _ptr_array(vals, n=3):
    """A NULL-padded table of ``n`` device addresses.  The caller holds it until the C call has returned."""
    arr = (C.c_void_p * n)(*[C.c_void_p(v) if v is not None else None for v in list(vals) + [None] * (n - len(vals))])
    return arr


def pad128(k: int) -> int:
    return (k + 127) // 128 * 128


@dataclass
class QAct:
    """A per-token-quantized activation: int8 codes (minus cx) + per-row dequant terms."""
    xq: torch.Tensor      # [rows, Kp] int8
    sx: torch.Tensor      # [rows] fp32 delta
    zx: torch.Tensor      # [rows] int32 zp - cx
    R: torch.Tensor       # [rows] int32 rowsum - K*zx
    K: int
    n_bits: int = 8
    zpf: Optional[torch.Tensor] = None

    @property
    def rows(self) -> int:
        return self.xq.shape[0]

    @property
    def Kp(self) -> int:
        return self.xq.shape[1]


@dataclass
class PackedWeight:
    """An offline-quantized weight: packed codes + per-out-channel dequant terms."""
    wq: torch.Tensor      # [N, Kp] int8  or [N, Kp/2] uint8 (n_bits <= 4)
    sw: torch.Tensor      # [N] fp32
    zw: torch.Tensor      # [N] int32
    cs: torch.Tensor      # [N] int32
    N: int
    K: int
    Kp: int
    n_bits: int

    def tensors(self):
        return [self.wq, self.sw, self.zw, self.cs]


def _qact_empty(rows: int, Kp: int, K: int, n_bits: int, device, want_zp: bool = False) -> QAct:
    """The outputs of one quantizer launch, unwritten."""
    xq = torch.empty((rows, Kp), dtype=torch.int8, device=device)
    sx = torch.empty(rows, dtype=torch.float32, device=device)
    zx = torch.empty(rows, dtype=torch.int32, device=device)
    R = torch.empty(rows, dtype=torch.int32, device=device)
    return QAct(xq, sx, zx, R, K, n_bits, torch.empty(rows, dtype=torch.float32, device=device) if want_zp else None)


def _qact_ptrs(q: QAct):
    """xq, sx, zx, R: the order every entry point takes the four tensors of one QAct."""
    return q.xq.data_ptr(), q.sx.data_ptr(), q.zx.data_ptr(), q.R.data_ptr()


def _weight_ptrs(w):
    """wq, sw, zw, cs of a PackedWeight or a PackedStack."""
    return w.wq.data_ptr(), w.sw.data_ptr(), w.zw.data_ptr(), w.cs.data_ptr()


def _tables(*lists):
    """One pointer table (_ptr_array) per list of up to three optional tensors."""
    return [_ptr_array([_p(t) for t in ts]) for ts in lists]


def _qact_tables(qs: Sequence[QAct]):
    """The xq / sx / zx / R tables of up to three QActs, in the order every multi-output entry point takes them."""
    return _tables(*([getattr(q, f) for q in qs] for f in ("xq", "sx", "zx", "R")))


def _void(tables):
    return [C.cast(t, C.c_void_p) for t in tables]


def _req_gemm_gpu(a: QAct, w):
    """The operands of a GEMM are on the GPU (the codes stand for the rest: one allocation makes them all)."""
    _req_gpu(a.xq, "a.xq")
    _req_gpu(w.wq, "w.wq")


def _check_k(a: QAct, w):
    if a.K != w.K or a.Kp != w.Kp:
        raise VQError("K mismatch: activation %d/%d weight %d/%d" % (a.K, a.Kp, w.K, w.Kp))


def new_status(device) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


# --------------------------------------------------------------------------- quantizers
# reciprocal of a smooth-quant channel scale, keyed by the tensor (identity + in-place version): computed on first
# sight (one device round trip for the bad-channel count, so: in the eager warm-up pass, never under graph capture),
# None when the reciprocal form of x / s is not guaranteed bit-exact for some channel (the kernels then divide)
_RCP_CACHE: "dict[int, tuple]" = {}
# bumped whenever a device tensor that a captured HIP graph may reference by address is replaced (packed weights:
# qdiff/models/quant_layer.py; reciprocal vectors: below); graph.GraphedSampler drops its graphs when it moves
PACK_EPOCH = [0]


def smooth_rcp(s: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if s is None:
        return None
    key = id(s)
    ent = _RCP_CACHE.get(key)
    if ent is not None and ent[0]() is s and ent[1] == s._version:
        return ent[2]
    _req(s, torch.float32, "s")
    if torch.cuda.is_current_stream_capturing():
        return None                       # an unseen vector under capture: exact division, no host round trip
    r = torch.empty_like(s)
    bad = torch.zeros(1, dtype=torch.int32, device=s.device)
    check(_L().vq_smooth_reciprocal(_p(s), _p(r), s.numel(), _p(bad), _stream()), "vq_smooth_reciprocal")
    out = r if int(bad.item()) == 0 else None
    # entries of dead vectors go on every insert; a LIVE entry is never evicted (its reciprocal may be referenced by
    # address from a captured graph) - only replaced when its vector was modified in place, which moves the epoch
    for k in [k for k, v in _RCP_CACHE.items() if v[0]() is None]:
        _RCP_CACHE.pop(k, None)
    if ent is not None and ent[0]() is s:
        PACK_EPOCH[0] += 1
    _RCP_CACHE[key] = (weakref.ref(s), s._version, out)
    return out


_NO_RCP = object()


def _rcp_or_none(s: Optional[torch.Tensor]):
    """The gate of the fused attention / GEMM + quantizer wrappers: the reciprocal of their smoothing vector (None without
    a vector), or _NO_RCP when it has no exact reciprocal form - the wrapper then returns None before it allocates or
    launches anything, and its caller keeps the two launches."""
    if s is None:
        return None
    r = smooth_rcp(s)
    return _NO_RCP if r is None else r


def act_scale_momentum(x: torch.Tensor, act_scale: torch.Tensor, momentum: float, scratch: Optional[torch.Tensor] = None,
                       cur_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One update of a running smooth-quant statistic on the device: ``act_scale`` [C] fp32 (a contiguous view of one time
    range of ``act_quantizer.act_scale``) moves IN PLACE by the per-channel abs-max of x [B, n_tok, C] fp16 averaged over B,
    first call or momentum form decided on the device, zeros patched to 1e-5 (include/viditq.h: vq_act_scale_momentum).
    ``scratch`` [B*C] int32 work space (allocated when not given; its content on entry does not matter)."""
    _req(x, torch.float16, "x")
    assert x.dim() == 3
    B, n_tok, Cc = x.shape
    _req(act_scale, torch.float32, "act_scale")
    if act_scale.numel() != Cc:
        raise VQError("act_scale must hold one entry per channel of x")
    if scratch is None:
        scratch = torch.empty(B * Cc, dtype=torch.int32, device=x.device)
    _req(scratch, torch.int32, "scratch")
    if scratch.numel() < B * Cc:
        raise VQError("scratch must hold B*C words")
    if cur_out is not None:
        _req(cur_out, torch.float32, "cur_out")
        assert cur_out.numel() == Cc
    m = float(momentum)
    # 1 - momentum in double, rounded once to fp32: what torch makes of the Python scalar in `cur * (1 - momentum)`
    check(_L().vq_act_scale_momentum(_p(x), _p(act_scale), _p(cur_out), _p(scratch), m, 1.0 - m, B, n_tok, Cc, _stream()),
          "vq_act_scale_momentum")
    return act_scale


def smooth_div_check(a: torch.Tensor, b: torch.Tensor):
    """(reciprocal-form quotient, IEEE quotient) of a / b elementwise - test hook."""
    _req(a, torch.float32, "a")
    _req(b, torch.float32, "b")
    fast, exact = torch.empty_like(a), torch.empty_like(a)
    check(_L().vq_smooth_div_check(_p(a), _p(b), _p(fast), _p(exact), a.numel(), _stream()), "vq_smooth_div_check")
    return fast, exact


def rowquant(x: torch.Tensor, n_bits: int = 8, s: Optional[torch.Tensor] = None,
             add_rows: Optional[torch.Tensor] = None, add_div: int = 1,
             status: Optional[torch.Tensor] = None, want_zp: bool = False,
             delta: Optional[torch.Tensor] = None, zp: Optional[torch.Tensor] = None, fast_div: bool = True) -> QAct:
    """Per-token quantizer of x [B, n_tok, C] fp16 (scales shared over B): dynamic min-max, or on a
    static calibrated grid when ``delta``/``zp`` (1 or n_tok entries) are given."""
    _req(x, torch.float16, "x")
    assert x.dim() == 3
    B, n_tok, Cc = x.shape
    Kp = pad128(Cc)
    out = _qact_empty(B * n_tok, Kp, Cc, n_bits, x.device, want_zp)
    if s is not None:
        _req(s, torch.float32, "s")
        assert s.numel() == Cc
    n_add = 0
    if add_rows is not None:
        _req(add_rows, torch.float16, "add_rows")
        n_add = add_rows.shape[0]
    n_param = 0
    if delta is not None:
        delta, zp = _flat_f32(delta, "delta"), _flat_f32(zp, "zp")
        n_param = delta.numel()
    s_rcp = smooth_rcp(s) if fast_div else None
    check(_L().vq_rowquant(_p(x), _p(add_rows), n_add, add_div, _p(s), _p(s_rcp), *_qact_ptrs(out), _p(out.zpf),
                           _p(delta), _p(zp), n_param, B, n_tok, Cc, Kp, n_bits, _p(status), _stream()),
          "vq_rowquant")
    return out


def rowquant_multi(x: torch.Tensor, smooth: Sequence[torch.Tensor], n_bits: int = 8,
                   status: Optional[torch.Tensor] = None) -> List[QAct]:
    """One QAct of x [1, n_tok, C] per smoothing vector (the q / k / v quantizers of a plan that balances each Linear
    against its own weight) in ONE launch when the reciprocal-form kernel covers the shape, else one launch each."""
    _req(x, torch.float16, "x")
    B, n_tok, Cc = x.shape
    rcps = [smooth_rcp(sm) for sm in smooth]
    Kp = pad128(Cc)
    G = len(smooth)
    if B != 1 or G > 3 or any(r is None for r in rcps) or Kp != Cc or Cc % 128 or not (768 <= Cc <= 1280) or n_tok < 2:
        return [rowquant(x, n_bits=n_bits, s=sm, status=status) for sm in smooth]
    outs = [_qact_empty(n_tok, Kp, Cc, n_bits, x.device) for _ in range(G)]
    keep = _tables(smooth, rcps) + _qact_tables(outs)
    check(_L().vq_rowquant_smooth_multi(_p(x), G, *_void(keep), n_tok, Cc, Kp, n_bits, _p(status), _stream()),
          "vq_rowquant_smooth_multi")
    return outs


def rowquant_multi_shared_ok(B: int, n_tok: int, Cc: int, Kp: int, n_bits: int, n_out: int) -> bool:
    """Whether vq_rowquant_smooth_multi_shared takes this launch: every refusal of the entry point (include/viditq.h) that
    these six arguments decide, mirrored for callers that choose a route BEFORE they launch - a refused shape takes one
    launch per output.  (The pointers, their alignment and the shift / scale pair stay with the entry point.)"""
    if not (1 <= n_out <= 3) or min(B, n_tok, Cc) <= 0:              # VQ_EINVAL
        return False
    if Cc % 8 or Kp % 128 or Kp < Cc:                                 # VQ_ESHAPE
        return False
    if not (2 <= n_bits <= 8):                                        # VQ_EUNSUP: the code width
        return False
    return B == 2 and Cc in (768, 1024, 1152, 1280) and Kp == Cc     # VQ_EUNSUP: the half-wave pair kernel's shapes


def rowquant_multi_shared(x: torch.Tensor, smooth: Sequence[torch.Tensor], n_bits: int = 8,
                          status: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                          scale: Optional[torch.Tensor] = None, eps: float = 1e-6) -> Optional[List[QAct]]:
    """One QAct of x [2, n_tok, C] (a joint forward: a token's grid is shared by its rows of both samples) per smoothing
    vector, from ONE pass over the rows.  Plain: output j is ``rowquant(x, n_bits, s=smooth[j])``, bit for bit.  With
    ``shift`` / ``scale`` [2, C] fp32: LayerNorm + modulate first, output j is ``ln_modulate_rowquant(x, shift, scale, eps,
    smooth=[smooth[j]], n_bits)``, bit for bit.  None - nothing launched, nothing written - when the entry point would
    refuse the shape (:func:`rowquant_multi_shared_ok`) or a vector has no exact reciprocal form."""
    _req(x, torch.float16, "x")
    assert x.dim() == 3
    B, n_tok, Cc = x.shape
    Kp = pad128(Cc)
    G = len(smooth)
    if (shift is None) != (scale is None):
        raise VQError("rowquant_multi_shared: shift and scale come together")
    if not rowquant_multi_shared_ok(B, n_tok, Cc, Kp, n_bits, G):
        return None
    for sm in smooth:
        _req(sm, torch.float32, "smooth")
        if sm.numel() != Cc:
            raise VQError("rowquant_multi_shared: one smoothing entry per channel")
    rcps = [smooth_rcp(sm) for sm in smooth]                      # kept alive until the launch is enqueued
    if any(r is None for r in rcps):
        return None
    if shift is not None:
        _req(shift, torch.float32, "shift")
        _req(scale, torch.float32, "scale")
        if shift.numel() != B * Cc or scale.numel() != B * Cc:
            raise VQError("rowquant_multi_shared: shift / scale must be [B, C]")
    outs = [_qact_empty(B * n_tok, Kp, Cc, n_bits, x.device) for _ in range(G)]
    keep = _tables(smooth, rcps) + _qact_tables(outs)
    check(_L().vq_rowquant_smooth_multi_shared(_p(x), _p(shift), _p(scale), float(eps), G, *_void(keep), B, n_tok, Cc, Kp,
                                               n_bits, _p(status), _stream()), "vq_rowquant_smooth_multi_shared")
    return outs


STATIC_MAX_KP = 4608        # rows the one-pass static-grid kernels hold (csrc/rowquant_static.hip)


def rowquant_static_ok(Cc: int, Kp: int, n_bits: int, n_out: int, add_rows: bool = False, ln: bool = False) -> bool:
    """Whether vq_rowquant_static takes this launch: the entry point's refusals (include/viditq.h), mirrored for callers
    that choose a route BEFORE they launch - a refused shape takes the layerwise quantizers, it does not raise."""
    if not (1 <= n_out <= 3) or Cc <= 0 or Kp <= 0:
        return False
    if Cc % 8 or Kp % 128 or Kp < Cc:
        return False
    return not (add_rows and ln) and 2 <= n_bits <= 8 and Kp <= STATIC_MAX_KP


def rowquant_static(x: torch.Tensor, delta: Sequence[torch.Tensor], zp: Sequence[torch.Tensor], n_bits: int = 8,
                    smooth: Optional[Sequence[Optional[torch.Tensor]]] = None, add_rows: Optional[torch.Tensor] = None,
                    add_div: int = 1, shift: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                    eps: float = 1e-6, want_xm: bool = False, fast_div: bool = True, Kp: Optional[int] = None):
    """One pass over x [B, n_tok, C] fp16 -> one QAct per calibrated grid (delta[j], zp[j]) (1 or n_tok entries each, read
    on the device), behind ``smooth[j]`` when given.  Input arm: plain, ``+ add_rows[(r % n_tok) // add_div]``, or - with
    ``shift`` / ``scale`` [B, C] fp32 - LayerNorm + modulate rounded to fp16 (returned too with ``want_xm``).
    ``Kp``: row stride of the codes when it is to be more than C rounded up to 128."""
    _req(x, torch.float16, "x")
    assert x.dim() == 3
    B, n_tok, Cc = x.shape
    n_out = len(delta)
    assert len(zp) == n_out and 1 <= n_out <= 3
    Kp = pad128(Cc) if Kp is None else int(Kp)
    ds = [_flat_f32(d, "delta") for d in delta]
    zs = [_flat_f32(z, "zp") for z in zp]
    n_param = ds[0].numel()
    assert all(d.numel() == n_param for d in ds) and all(z.numel() == n_param for z in zs)
    smooth = [None] * n_out if smooth is None else list(smooth)
    assert len(smooth) == n_out
    for sm in smooth:
        if sm is not None:
            _req(sm, torch.float32, "smooth")
            assert sm.numel() == Cc
    rcps = [smooth_rcp(sm) if fast_div else None for sm in smooth]     # kept alive until the launch is enqueued
    n_add = 0
    if add_rows is not None:
        _req(add_rows, torch.float16, "add_rows")
        assert add_rows.shape[-1] == Cc
        n_add = add_rows.shape[0]
    ln = shift is not None or scale is not None
    if ln:
        _req(shift, torch.float32, "shift")
        _req(scale, torch.float32, "scale")
        assert shift.numel() == B * Cc and scale.numel() == B * Cc
    elif want_xm:
        raise VQError("rowquant_static: xm exists behind LayerNorm + modulate only")
    outs = [_qact_empty(B * n_tok, Kp, Cc, n_bits, x.device) for _ in range(n_out)]
    xm = torch.empty_like(x) if want_xm else None
    grid, codes = _tables(smooth, rcps, ds, zs), _qact_tables(outs)
    check(_L().vq_rowquant_static(_p(x), _p(add_rows), n_add, add_div, _p(shift), _p(scale), float(eps), n_out, *_void(grid),
                                  n_param, *_void(codes), _p(xm), B, n_tok, Cc, Kp, n_bits, _stream()), "vq_rowquant_static")
    return (outs, xm) if want_xm else outs


def gelu_rowquant(x: torch.Tensor, n_bits: int = 8, s: Optional[torch.Tensor] = None,
                  status: Optional[torch.Tensor] = None, fast_div: bool = True) -> QAct:
    """GELU(tanh) then the per-token quantizer of x [B, n_tok, C] fp16 (the fc1 -> act -> fc2-quantizer hand-over);
    B = 1, or B = 2 with the grid of a token shared by its two samples (rows = sample * n_tok + token)."""
    _req(x, torch.float16, "x")
    B, n_tok, Cc = x.shape
    Kp = pad128(Cc)
    out = _qact_empty(B * n_tok, Kp, Cc, n_bits, x.device)
    _req_opt(s, torch.float32, "s")
    s_rcp = smooth_rcp(s) if fast_div else None
    check(_L().vq_gelu_rowquant(_p(x), _p(s), _p(s_rcp), *_qact_ptrs(out), B, n_tok, Cc, Kp, n_bits, _p(status), _stream()),
          "vq_gelu_rowquant")
    return out


def ln_modulate_rowquant(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float = 1e-6,
                         smooth: Sequence[Optional[torch.Tensor]] = (None,), n_bits: int = 8,
                         status: Optional[torch.Tensor] = None, want_xm: bool = False, fast_div: bool = True):
    """LN(no affine) + (1+scale)*.+shift + per-token quant; one QAct per entry of ``smooth``."""
    _req(x, torch.float16, "x")
    B, n_tok, Cc = x.shape
    _req(shift, torch.float32, "shift")
    _req(scale, torch.float32, "scale")
    assert shift.numel() == B * Cc and scale.numel() == B * Cc
    n_out = len(smooth)
    Kp = pad128(Cc)
    outs = [_qact_empty(B * n_tok, Kp, Cc, n_bits, x.device) for _ in range(n_out)]
    for sm in smooth:
        if sm is not None:
            _req(sm, torch.float32, "smooth")
    rcps = [smooth_rcp(sm) if fast_div else None for sm in smooth]     # kept alive until the launch is enqueued
    keep = _tables(smooth, rcps) + _qact_tables(outs)
    xm = torch.empty_like(x) if want_xm else None
    check(_L().vq_ln_modulate_rowquant(_p(x), _p(shift), _p(scale), float(eps), n_out, *_void(keep), _p(xm), B, n_tok, Cc, Kp,
                                       n_bits, _p(status), _stream()), "vq_ln_modulate_rowquant")
    return (outs, xm) if want_xm else outs


def fakequant_act(x: torch.Tensor, n_bits: int = 8, delta: Optional[torch.Tensor] = None,
                  zp: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                  want_codes: bool = False):
    """Exact fake-quant of x [B, n_tok, C] fp16.  delta/zp None -> per-token dynamic."""
    _req(x, torch.float16, "x")
    B, n_tok, Cc = x.shape
    dev = x.device
    out = torch.empty_like(x)
    codes = torch.empty((B, n_tok, Cc), dtype=torch.uint8, device=dev) if want_codes else None
    if delta is None:
        d_out = torch.empty(n_tok, dtype=torch.float32, device=dev)
        z_out = torch.empty(n_tok, dtype=torch.float32, device=dev)
        scratch = torch.empty(1, dtype=torch.float32, device=dev)
        check(_L().vq_fakequant_act(_p(x), _p(out), _p(codes), _p(d_out), _p(z_out), None, None, 0, B, n_tok, Cc,
                                    n_bits, 0, _p(scratch), _p(status), _stream()), "vq_fakequant_act")
        return out, codes, d_out, z_out
    d, z = _flat_f32(delta, "delta"), _flat_f32(zp, "zp")
    assert d.numel() == z.numel() and d.numel() in (1, n_tok)
    check(_L().vq_fakequant_act(_p(x), _p(out), _p(codes), None, None, _p(d), _p(z), d.numel(), B, n_tok, Cc,
                                n_bits, 1, None, _p(status), _stream()), "vq_fakequant_act")
    return out, codes, d, z


def epsfill_fixup(flag: torch.Tensor, x: torch.Tensor, s: Optional[torch.Tensor], wdq: torch.Tensor,
                  bias: Optional[torch.Tensor], out: torch.Tensor, n_bits: int = 8) -> torch.Tensor:
    """In-place global eps-fill fix-up of ``out`` [n_batch, L, N] fp16 = integer-route Linear(s) of the shared input x
    [L, C] fp16: a no-op kernel while ``flag`` (the quantizer's private status word) is clear, the reference's fp16-mode
    result with every token on the 1e-6 grid when it is set (base_quantizer.py:219-223).  wdq [n_batch, N, C] fp16
    dequantized weights, bias [n_batch, N] fp16 or None."""
    _req(x, torch.float16, "x"); _req(wdq, torch.float16, "wdq"); _req(out, torch.float16, "out")
    nb, N, C = wdq.shape
    L = x.shape[-2]
    assert x.shape[-1] == C and x.numel() == L * C and out.numel() == nb * L * N
    assert x.is_contiguous() and wdq.is_contiguous() and out.is_contiguous()
    _req_opt(s, torch.float32, "s")
    if bias is not None:
        _req(bias, torch.float16, "bias")
        assert bias.numel() == nb * N and bias.is_contiguous()
    check(_L().vq_epsfill_fixup(_p(flag), _p(x), _p(s), _p(wdq), _p(bias), _p(out), nb, L, C, N, n_bits, _stream()),
          "vq_epsfill_fixup")
    return out


# --------------------------------------------------------------------------- weights
def weight_minmax(W: torch.Tensor, n_bits: int, s: Optional[torch.Tensor] = None, force_eps: bool = False,
                  status: Optional[torch.Tensor] = None):
    """Per-out-channel min-max (delta, zp) of W*s, W [N,K] fp16."""
    _req(W, torch.float16, "W")
    N, K = W.shape
    delta = torch.empty(N, dtype=torch.float32, device=W.device)
    zp = torch.empty(N, dtype=torch.float32, device=W.device)
    _req_opt(s, torch.float32, "s")
    check(_L().vq_weight_minmax(_p(W), _p(s), _p(delta), _p(zp), N, K, n_bits, int(force_eps), _p(status),
                                _stream()), "vq_weight_minmax")
    return delta, zp


def packed_shapes(N: int, K: int, n_bits: int):
    """(shape, dtype) of the four tensors of a PackedWeight [N, K] at ``n_bits``: codes, sw, zw, cs."""
    Kp = pad128(K)
    wq = ((N, Kp // 2), torch.uint8) if n_bits <= 4 else ((N, Kp), torch.int8)
    return [wq, ((N,), torch.float32), ((N,), torch.int32), ((N,), torch.int32)]


def pack_weight(W: torch.Tensor, delta: torch.Tensor, zp: torch.Tensor, n_bits: int,
                s: Optional[torch.Tensor] = None, out: Optional[Sequence[torch.Tensor]] = None) -> PackedWeight:
    """Quantize W*s on the (delta, zp) grid and pack for the int8 MFMA GEMM.  ``out`` = (wq, sw, zw, cs) pre-allocated
    with :func:`packed_shapes` (e.g. views of one broadcast arena, shard.py) instead of fresh tensors."""
    _req(W, torch.float16, "W")
    N, K = W.shape
    Kp = pad128(K)
    dev = W.device
    d, z = _flat_f32(delta, "delta"), _flat_f32(zp, "zp")
    assert d.numel() == N and z.numel() == N
    if out is not None:
        wq, sw, zw, cs = out
        for t_, (shape, dt) in zip(out, packed_shapes(N, K, n_bits)):
            if tuple(t_.shape) != tuple(shape) or t_.dtype != dt or not t_.is_contiguous() or t_.device != dev:
                raise VQError("pack_weight: out tensors must match packed_shapes() on the weight's device")
    else:
        (wqs, wqd), _, _, _ = packed_shapes(N, K, n_bits)
        wq = torch.empty(wqs, dtype=wqd, device=dev)
        sw = torch.empty(N, dtype=torch.float32, device=dev)
        zw = torch.empty(N, dtype=torch.int32, device=dev)
        cs = torch.empty(N, dtype=torch.int32, device=dev)
    _req_opt(s, torch.float32, "s")
    check(_L().vq_pack_weight(_p(W), _p(s), _p(d), _p(z), _p(wq), _p(sw), _p(zw), _p(cs), N, K, Kp, n_bits,
                              _stream()), "vq_pack_weight")
    return PackedWeight(wq, sw, zw, cs, N, K, Kp, n_bits)


# --------------------------------------------------------------------------- GEMM
# When set to a list, every GEMM launch is bracketed by two events recorded on the launch stream and
# (start, end, int8_ops, algorithmic_bytes) is appended - bench.py's live roofline measurement.
GEMM_TIMING = None
# kernel used when the caller does not choose: -1 = the library's own choice per shape (VQ_GEMM_DEFAULT);
# 11 pins the full-line (128 B of k per row) double-buffered LDS-DMA ring, 256x288 tile (csrc/gemm_wide.h);
# nibble-packed (<= 4 bit) weights take the same kernels with 64-byte packed rows
DEFAULT_GEMM_VARIANT = -1


def _timing_begin():
    """The event pair of one GEMM_TIMING bracket, the first recorded on the launch stream."""
    e0, e1 = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e0.record()
    return e0, e1


def _timing_end(timing: list, events, int8_ops: float, nbytes: int):
    events[1].record()
    timing.append((events[0], events[1], int8_ops, nbytes))


def gemm_i8(a: QAct, w: PackedWeight, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
            epilogue: int = EPI_NONE, resid: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
            rows_per_gate: int = 0, variant: int = -1) -> torch.Tensor:
    """out[M, N] fp16 = dequant(int8 MFMA(a, w)) + bias, with the fused epilogue."""
    _req_gemm_gpu(a, w)
    _check_k(a, w)
    M, N = a.rows, w.N
    if out is None:
        out = torch.empty((M, N), dtype=torch.float16, device=a.xq.device)
    else:
        if not out.is_cuda or out.dtype != torch.float16 or out.dim() != 2 or out.stride(1) != 1:
            raise VQError("out must be a GPU fp16 2-D tensor with unit column stride")
        assert out.shape[0] == M and out.shape[1] >= N
    ldo = out.stride(0)
    _req_opt(bias, torch.float32, "bias")
    if resid is not None:
        if not resid.is_cuda or resid.dtype != torch.float16 or resid.dim() != 2 or resid.stride(1) != 1:
            raise VQError("resid must be a GPU fp16 2-D tensor with unit column stride")
        assert resid.stride(0) == ldo and resid.shape[0] == M
    _req_opt(gate, torch.float32, "gate")
    if variant < 0:
        variant = DEFAULT_GEMM_VARIANT
    timing = GEMM_TIMING
    events = None if timing is None else _timing_begin()
    check(_L().vq_gemm_i8(*_qact_ptrs(a), *_weight_ptrs(w), _p(bias), _p(out), ldo, _p(resid), _p(gate), rows_per_gate,
                          M, N, a.K, a.Kp, w.n_bits, epilogue, variant, _stream()), "vq_gemm_i8")
    if events is not None:
        wbytes = N * a.K // 2 if w.n_bits <= 4 else N * a.K
        _timing_end(timing, events, 2.0 * M * N * a.K, M * a.K + wbytes + 2 * M * N * (2 if resid is not None else 1))
    return out


def gemm_rowquant_static_ok(M: int, N: int, K: int, w_bits: int, n_bits: int, variant: int = -1) -> bool:
    """Whether vq_gemm_i8_rowquant_static takes this launch (Kp and Kp_out the 128-padded K and N, aligned buffers): the
    entry point's refusals (include/viditq.h), mirrored for callers that choose a route BEFORE they launch - a refused
    shape takes the GEMM's GELU epilogue and the quantizer pass, it does not raise."""
    if M <= 0 or N <= 0 or K <= 0:
        return False
    Kp = pad128(K)
    if K > 16384 or M * Kp >= 1 << 32 or N * Kp >= 1 << 32 or N % 8:
        return False
    if not (4 < w_bits <= 8 and 2 <= n_bits <= 8) or variant not in (-1, 11, 16, 19):
        return False
    return variant != 19 or (M % 256 == 0 and N % 288 == 0)


def gemm_i8_rowquant_static(a: QAct, w: PackedWeight, bias: Optional[torch.Tensor], delta: torch.Tensor, zp: torch.Tensor,
                            n_bits: int, s: Optional[torch.Tensor] = None, variant: int = -1) -> Optional[QAct]:
    """fc1 + GELU(tanh) + the consuming Linear's STATIC tensor-wise quantizer - ``delta`` / ``zp``: one fp32 value each,
    read on the device - at ``n_bits`` (2..8) in ONE GEMM launch that never writes the fp16 activation.  Returns what
    ``rowquant(gemm_i8(a, w, bias, epilogue=EPI_GELU, variant=variant).view(1, M, N), n_bits, s=s, delta=delta, zp=zp)``
    returns, bit for bit.  ``s``: the consuming Linear's smoothing vector [N]; None is returned (the caller keeps the two
    launches) when its reciprocal form is not available.  A launch the entry point refuses raises: ask
    :func:`gemm_rowquant_static_ok` first."""
    _req_gemm_gpu(a, w)
    if s is not None:
        _req(s, torch.float32, "s")
        if s.numel() != w.N:
            raise VQError("s must hold one entry per output column")
    s_rcp = _rcp_or_none(s)
    if s_rcp is _NO_RCP:
        return None
    _check_k(a, w)
    delta, zp = _tensorwise_grid(_flat_f32(delta, "delta"), _flat_f32(zp, "zp"), "gemm_i8_rowquant_static")
    _req_opt(bias, torch.float32, "bias")
    M, N = a.rows, w.N
    Kp_out = pad128(N)
    out = _qact_empty(M, Kp_out, N, n_bits, a.xq.device)
    if variant < 0:
        variant = DEFAULT_GEMM_VARIANT
    timing = GEMM_TIMING
    events = None if timing is None else _timing_begin()
    check(_L().vq_gemm_i8_rowquant_static(*_qact_ptrs(a), *_weight_ptrs(w), _p(bias), _p(s), _p(s_rcp), _p(delta), _p(zp),
                                          *_qact_ptrs(out), M, N, a.K, a.Kp, Kp_out, w.n_bits, n_bits, variant, _stream()),
          "vq_gemm_i8_rowquant_static")
    if events is not None:
        # fused byte model: both operands, the codes (pad columns included) and the three row terms; no fp16 matrix
        _timing_end(timing, events, 2.0 * M * N * a.K, M * a.K + N * a.K + M * Kp_out + 12 * M)
    return out


def gemm_i8_cross_attn(a: QAct, w: PackedWeight, bias: Optional[torch.Tensor], k: torch.Tensor, v: torch.Tensor,
                       o: torch.Tensor, n_seq: int, Lq: int, Lk: int, H: int, D: int, kv_seq_stride: int, kv_tok_stride: int,
                       o_seq_stride: int, o_tok_stride: int, kv_off: Optional[torch.Tensor] = None,
                       scale: Optional[float] = None) -> torch.Tensor:
    """cross_attn.q_linear's GEMM and cross attention against the prompt's <= 128 keys in ONE launch that never writes q:
    ``o`` is, bit for bit, what ``attn_fwd(gemm_i8(a, w, bias), k, v, o, n_seq, Lq, Lk, H, D, Lq * N, N, ...)`` writes.
    Shapes the entry point refuses (include/viditq.h) raise: callers choose the route before they launch."""
    _req_gemm_gpu(a, w)
    _req_f16((k, "k"), (v, "v"), (o, "o"))
    _check_k(a, w)
    _req_opt(bias, torch.float32, "bias")
    _req_opt(kv_off, torch.int32, "kv_off")
    check(_L().vq_gemm_i8_cross_attn(*_qact_ptrs(a), *_weight_ptrs(w), _p(bias), _p(k), _p(v), _p(o), a.rows, w.N, a.K, a.Kp,
                                     w.n_bits, n_seq, Lq, Lk, H, D, kv_seq_stride, kv_tok_stride, o_seq_stride, o_tok_stride,
                                     _p(kv_off), _attn_scale(D, scale), _stream()), "vq_gemm_i8_cross_attn")
    return o


def gemm_i8_stamped(a: QAct, w: PackedWeight, bias: Optional[torch.Tensor] = None):
    """Diagnostics: ONE launch of the default 8-bit GEMM (256 x 288 tile, plain epilogue) with per-wave stamps.
    -> (out [M, N] fp16, stamps [tiles, 8, 10] int64: 0-6 shader cycles per phase boundary, 7 / 8 the chip's 100 MHz wall
    clock at entry / exit).  `shader_clock_ghz(stamps)` turns them into the clock the kernel ran at."""
    if a.K != w.K or a.Kp != w.Kp or w.n_bits != 8:
        raise VQError("gemm_i8_stamped: 8-bit weights of the activation's K")
    M, N = a.rows, w.N
    if not a.xq.is_cuda:
        raise VQError("gemm_i8_stamped needs GPU tensors")
    _req_gpu(w.wq, "w.wq")
    out = torch.empty((M, N), dtype=torch.float16, device=a.xq.device)
    tiles = ((M + 255) // 256) * ((N + 287) // 288)
    stamps = torch.zeros((tiles, 8, 10), dtype=torch.int64, device=a.xq.device)
    check(_L().vq_gemm_i8_stamped(*_qact_ptrs(a), *_weight_ptrs(w), _p(bias), _p(out), out.stride(0), M, N, a.K, a.Kp,
                                  _p(stamps), stamps.numel(), _stream()), "vq_gemm_i8_stamped")
    return out, stamps


def shader_clock_ghz(stamps: torch.Tensor) -> dict:
    """Median over waves of (shader cycles) / (10 ns wall-clock ticks) of a stamped GEMM launch, plus the tile phases in
    shader cycles (means over waves): what bench.py records beside its rates."""
    s = stamps.detach().cpu().double()
    cyc = s[:, :, 6] - s[:, :, 0]
    ticks = (s[:, :, 8] - s[:, :, 7]).clamp(min=1)
    ghz = float((cyc / ticks).median()) / 10.0
    ph = (s[:, :, 1:7] - s[:, :, 0:6]).mean(dim=(0, 1))
    names = ["prologue", "main_loop", "barrier_params", "dequant_slab", "store_issue", "store_drain"]
    span_us = float(s[:, :, 8].max() - s[:, :, 7].min()) / 100.0
    return {"ghz": ghz, "tile_cycles": float(cyc.mean()), "launch_span_us": span_us,
            "phase_cycles": {n: float(v) for n, v in zip(names, ph)}}


@dataclass
class PackedStack:
    """nbatch PackedWeights of identical shape stacked for vq_gemm_i8_batched (+ their fp32 biases)."""
    wq: torch.Tensor      # [nbatch, N, Kp] int8
    sw: torch.Tensor      # [nbatch, N]
    zw: torch.Tensor
    cs: torch.Tensor
    bias: Optional[torch.Tensor]
    nbatch: int
    N: int
    K: int
    Kp: int
    n_bits: int


def stack_packed(pws: Sequence[PackedWeight], biases: Sequence[Optional[torch.Tensor]]) -> PackedStack:
    p0 = pws[0]
    assert all(p.N == p0.N and p.K == p0.K and p.Kp == p0.Kp and p.n_bits == p0.n_bits for p in pws)
    if p0.n_bits <= 4:
        raise VQError("stack_packed: 8-bit (int8-stored) weights only")
    has_b = biases[0] is not None
    return PackedStack(torch.stack([p.wq for p in pws]).contiguous(), torch.stack([p.sw for p in pws]).contiguous(),
                       torch.stack([p.zw for p in pws]).contiguous(), torch.stack([p.cs for p in pws]).contiguous(),
                       torch.stack([b.float() for b in biases]).contiguous() if has_b else None,
                       len(pws), p0.N, p0.K, p0.Kp, p0.n_bits)


def gemm_i8_batched(a: QAct, w: PackedStack, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] [M, N] fp16 for every stacked weight set b, all from the same quantized activation ``a``."""
    _req_gemm_gpu(a, w)
    _check_k(a, w)
    M = a.rows
    if out is None:
        out = torch.empty((w.nbatch, M, w.N), dtype=torch.float16, device=a.xq.device)
    check(_L().vq_gemm_i8_batched(*_qact_ptrs(a), *_weight_ptrs(w), _p(w.bias), _p(out), w.nbatch, M, w.N, a.K, a.Kp,
                                  w.n_bits, _stream()), "vq_gemm_i8_batched")
    return out


def gemm_i8_grouped(acts: Sequence[QAct], ws: Sequence[PackedWeight], biases: Optional[Sequence] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """2 or 3 Linears of one shape in one launch: out[:, g*N:(g+1)*N] = Linear_g(acts[g]) (q | k | v blocks)."""
    G = len(acts)
    assert 1 <= G <= 3 and len(ws) == G
    a0, w0 = acts[0], ws[0]
    for a, w in zip(acts, ws):
        _req_gemm_gpu(a, w)
        if (a.K, a.Kp, a.rows) != (a0.K, a0.Kp, a0.rows) or (w.N, w.K, w.Kp, w.n_bits) != (w0.N, w0.K, w0.Kp, w0.n_bits) \
                or a.K != w.K or a.Kp != w.Kp:
            raise VQError("grouped GEMM needs one shape for every group")
    M, N = a0.rows, w0.N
    if out is None:
        out = torch.empty((M, G * N), dtype=torch.float16, device=a0.xq.device)
    assert out.dtype == torch.float16 and out.stride(-1) == 1 and out.shape[-1] >= G * N
    bs = [None] * G if biases is None else [None if b is None else _req(b, torch.float32, "bias") for b in biases]
    keep = _qact_tables(acts) + _tables(*([getattr(w, f) for w in ws] for f in ("wq", "sw", "zw", "cs")), bs)
    check(_L().vq_gemm_i8_grouped(G, *_void(keep), _p(out), out.stride(0), M, N, a0.K, a0.Kp, w0.n_bits, _stream()),
          "vq_gemm_i8_grouped")
    return out


# --------------------------------------------------------------------------- attention
def attn_fwd(q, k, v, o, n_seq, Lq, Lk, H, D, q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride,
             o_seq_stride, o_tok_stride, kv_off: Optional[torch.Tensor] = None, scale: Optional[float] = None):
    """Flash attention over strided fp16 views (pointers are the tensors' data_ptr())."""
    _req_f16((q, "q"), (k, "k"), (v, "v"), (o, "o"))
    _req_opt(kv_off, torch.int32, "kv_off")
    check(_L().vq_attn_fwd(_p(q), _p(k), _p(v), _p(o), n_seq, Lq, Lk, H, D, q_seq_stride, q_tok_stride,
                           kv_seq_stride, kv_tok_stride, o_seq_stride, o_tok_stride, _p(kv_off), _attn_scale(D, scale),
                           _stream()), "vq_attn_fwd")
    return o


def attn_temporal(q, k, v, o, B, T, S, H, D, ld_in, ld_out, scale: Optional[float] = None):
    _req_f16((q, "q"), (k, "k"), (v, "v"), (o, "o"))
    check(_L().vq_attn_temporal(_p(q), _p(k), _p(v), _p(o), B, T, S, H, D, ld_in, ld_out, _attn_scale(D, scale), _stream()),
          "vq_attn_temporal")
    return o


def _check_o(o: Optional[torch.Tensor], rows: int, Cc: int, who: Optional[str], strided: bool = False):
    """The optional fp16 output of an attention + quantizer form, by each wrapper's own rule: a dense [rows, Cc] matrix, else
    a VQError in the name of ``who`` (an assertion for who = None); ``strided``: a view with pitches of its own, of which
    only the device and the type are asked."""
    if o is None:
        return
    if strided:
        _req_f16((o, "o"))
        return
    _req(o, torch.float16, "o")
    if who is None:
        assert o.shape == (rows, Cc)
    elif o.shape != (rows, Cc):
        raise VQError("%s: o must be [B*T*S, H*D]" % who)


def _attn_qact(q, o, rows, Cc, Kp, n_bits, D, scale, who, strided=False):
    """What the five attention + quantizer wrappers share once their own rules have passed and Kp is known: the check of the
    optional fp16 output (_check_o), the quantizer's outputs on q's device and the softmax scale.  -> (QAct, scale)"""
    _check_o(o, rows, Cc, who, strided)
    return _qact_empty(rows, Kp, Cc, n_bits, q.device), _attn_scale(D, scale)


def attn_temporal_rowquant(q, k, v, B, T, S, H, D, ld_in, scale: Optional[float] = None,
                           status: Optional[torch.Tensor] = None, o: Optional[torch.Tensor] = None,
                           s: Optional[torch.Tensor] = None) -> Optional[QAct]:
    """Temporal attention + the consuming Linear's per-token 8-bit dynamic quantizer in one kernel (B == 1 per
    forward: per-token scales are shared over the batch otherwise).  Returns what
    ``rowquant(attn_temporal(...).view(1, T*S, H*D), s=s)`` returns, bit for bit.  ``s``: the consuming Linear's
    smoothing vector; None is returned (caller runs the two kernels) when its reciprocal form is not available."""
    s_rcp = _rcp_or_none(s)
    if s_rcp is _NO_RCP:
        return None
    _req_f16((q, "q"), (k, "k"), (v, "v"))
    if B != 1:
        raise VQError("attn_temporal_rowquant: per-token scales are shared over the batch; B must be 1")
    Cc = H * D
    Kp = pad128(Cc)
    out, scale = _attn_qact(q, o, B * T * S, Cc, Kp, 8, D, scale, None)
    check(_L().vq_attn_temporal_rowquant(_p(q), _p(k), _p(v), _p(s), _p(s_rcp), *_qact_ptrs(out), _p(status), _p(o),
                                         B, T, S, H, D, ld_in, Kp, scale, _stream()), "vq_attn_temporal_rowquant")
    return out


def attn_temporal_shared_ok(B: int, T: int, H: int, D: int, Kp: int, n_bits: int) -> bool:
    """Whether vq_attn_temporal_rowquant_shared takes this launch: every refusal of the entry point (include/viditq.h) that
    these six arguments decide, mirrored for callers that choose a route BEFORE they launch - a refused shape takes
    attention and the quantizer separately.  (S, ld_in and the pointers stay with the entry point.)"""
    if min(B, T, H, D, Kp) <= 0:                                   # VQ_EINVAL
        return False
    Cc = H * D
    if B > 2 or T > 16 or H > 16 or D not in (16, 32, 64, 72) or Cc % 16 != 0 or Kp % 128 != 0 or Kp < Cc:   # VQ_ESHAPE
        return False
    if 16 * (Cc // 8) > 3 * 64 * H or D % 4 != 0:                  # VQ_ESHAPE: the V staging registers of the kernel
        return False
    return 2 <= n_bits <= 8                                        # VQ_EUNSUP


def attn_temporal_rowquant_shared(q, k, v, B, T, S, H, D, ld_in, n_bits: int = 8, scale: Optional[float] = None,
                                  status: Optional[torch.Tensor] = None, o: Optional[torch.Tensor] = None,
                                  s: Optional[torch.Tensor] = None) -> Optional[QAct]:
    """Temporal attention (T <= 16) + the consuming Linear's per-token dynamic quantizer at ``n_bits`` (2..8) for a joint
    forward of B <= 2 samples, whose rows of a token share one grid, in one kernel.  Returns what
    ``rowquant(o.view(B, T*S, H*D), n_bits=n_bits, s=s)`` returns for the kernel's own fp16 output ``o`` (also written when
    given, [B*T*S, H*D]), bit for bit.  ``s``: the consuming Linear's smoothing vector; None is returned (caller runs the
    two kernels) when its reciprocal form is not available."""
    s_rcp = _rcp_or_none(s)
    if s_rcp is _NO_RCP:
        return None
    _req_f16((q, "q"), (k, "k"), (v, "v"))
    Cc = H * D
    Kp = pad128(Cc)
    out, scale = _attn_qact(q, o, B * T * S, Cc, Kp, n_bits, D, scale, "attn_temporal_rowquant_shared")
    check(_L().vq_attn_temporal_rowquant_shared(_p(q), _p(k), _p(v), _p(s), _p(s_rcp), *_qact_ptrs(out), _p(status), _p(o),
                                                B, T, S, H, D, ld_in, Kp, n_bits, scale, _stream()),
          "vq_attn_temporal_rowquant_shared")
    return out


def attn_temporal_long(q, k, v, B, T, S, H, D, ld_in, o: Optional[torch.Tensor] = None, quant: bool = False,
                       scale: Optional[float] = None, status: Optional[torch.Tensor] = None,
                       s: Optional[torch.Tensor] = None):
    """Temporal attention for T <= 64 frames (one kernel; rows [B][T][S] as in :func:`attn_temporal`).
    ``quant=False``: writes and returns ``o`` [B*T*S, H*D] fp16 (row stride ``o.stride(0)``).
    ``quant=True`` (B == 1): returns the ``QAct`` of the consuming Linear's per-token 8-bit quantizer (behind its
    smoothing vector ``s``), bit-identical to ``rowquant`` of the fp16 output, and also writes ``o`` when given; None when
    ``s`` has no exact reciprocal form (the caller then runs attention and the quantizer separately)."""
    _req_f16((q, "q"), (k, "k"), (v, "v"))
    Cc = H * D
    rows = B * T * S
    if o is None and not quant:
        raise VQError("attn_temporal_long: o is required without quant")
    _check_o(o, rows, Cc, "attn_temporal_long")
    scale = _attn_scale(D, scale)
    ld_out = o.stride(0) if o is not None else 0
    if not quant:
        check(_L().vq_attn_temporal_long(_p(q), _p(k), _p(v), None, None, None, None, None, None, None, _p(o), B, T, S,
                                         H, D, ld_in, ld_out, 0, scale, _stream()), "vq_attn_temporal_long")
        return o
    if B != 1:
        raise VQError("attn_temporal_long: per-token scales are shared over the batch; B must be 1")
    s_rcp = _rcp_or_none(s)
    if s_rcp is _NO_RCP:
        return None
    Kp = pad128(Cc)
    out, scale = _attn_qact(q, None, rows, Cc, Kp, 8, D, scale, None)      # o and the scale: settled above, for both forms
    check(_L().vq_attn_temporal_long(_p(q), _p(k), _p(v), _p(s), _p(s_rcp), *_qact_ptrs(out), _p(status), _p(o),
                                     B, T, S, H, D, ld_in, ld_out, Kp, scale, _stream()), "vq_attn_temporal_long")
    return out


ATTN_HEAD_DIMS = (16, 32, 64, 72)     # head dims the attention kernels are compiled for (csrc/vq_common.h)


def attn_temporal_static_ok(T: int, H: int, D: int, Kp: int, n_bits: int) -> bool:
    """Whether vq_attn_temporal_rowquant_static takes this launch: the entry point's refusals (include/viditq.h), mirrored
    for callers that choose a route BEFORE they launch - a refused shape takes attention and the quantizer separately."""
    if not (1 <= T <= 64 and 1 <= H <= 16 and D in ATTN_HEAD_DIMS and Kp > 0):
        return False
    Cc = H * D
    return Cc % 16 == 0 and Kp % 128 == 0 and Kp >= Cc and 2 <= n_bits <= 8


def attn_temporal_rowquant_static(q, k, v, B, T, S, H, D, ld_in, delta: torch.Tensor, zp: torch.Tensor, n_bits: int = 8,
                                  scale: Optional[float] = None, o: Optional[torch.Tensor] = None,
                                  s: Optional[torch.Tensor] = None) -> Optional[QAct]:
    """Temporal attention (T <= 64, any B) + the consuming Linear's STATIC tensor-wise quantizer - ``delta`` / ``zp``: one
    fp32 value each, read on the device - at ``n_bits`` (2..8) in one kernel.  Returns what
    ``rowquant(o.view(B, T*S, H*D), n_bits, s=s, delta=delta, zp=zp)`` returns for the kernel's own fp16 output ``o``
    (also written when given, [B*T*S, H*D]), bit for bit.  ``s``: the consuming Linear's smoothing vector; None is
    returned (caller runs the two kernels) when its reciprocal form is not available."""
    s_rcp = _rcp_or_none(s)
    if s_rcp is _NO_RCP:
        return None
    _req_f16((q, "q"), (k, "k"), (v, "v"))
    delta, zp = _tensorwise_grid(_flat_f32(delta, "delta"), _flat_f32(zp, "zp"), "attn_temporal_rowquant_static")
    Cc = H * D
    Kp = pad128(Cc)
    out, scale = _attn_qact(q, o, B * T * S, Cc, Kp, n_bits, D, scale, "attn_temporal_rowquant_static")
    ld_out = Cc if o is None else o.stride(0)
    check(_L().vq_attn_temporal_rowquant_static(_p(q), _p(k), _p(v), _p(s), _p(s_rcp), _p(delta), _p(zp), *_qact_ptrs(out),
                                                _p(o), B, T, S, H, D, ld_in, ld_out, Kp, n_bits, scale, _stream()),
          "vq_attn_temporal_rowquant_static")
    return out


# routes of vq_attn_fwd_route (VQ_ATTN_K_* of include/viditq.h) whose kernel has a static-grid form
ATTN_FWD_STATIC_ROUTES = (0, 3, 5, 6, 7, 8, 9)     # FWD, FWD32D, FWD64D, CROSS32_2 .. CROSS32_5


def attn_fwd_static_ok(n_seq: int, Lq: int, Lk: int, H: int, D: int, q_tok_stride: int, kv_tok_stride: int, Kp: int,
                       n_bits: int, kv_off: bool = False, q_seq_stride: Optional[int] = None,
                       kv_seq_stride: Optional[int] = None) -> bool:
    """Whether vq_attn_fwd_rowquant_static takes this launch: the entry point's refusals (include/viditq.h), mirrored for
    callers that choose a route BEFORE they launch - a refused shape takes attention and the quantizer separately.  The
    route is asked of vq_attn_fwd_route (dummy pointers: it makes no HIP call and dereferences nothing)."""
    if n_seq <= 0 or Lq <= 0 or H <= 0 or D <= 0 or Kp <= 0 or (Lk <= 0 and not kv_off):
        return False
    if D not in ATTN_HEAD_DIMS or not 2 <= n_bits <= 8:
        return False
    if Kp % 128 != 0 or Kp < H * D or n_seq * Lq > 0x7fffffff:
        return False
    q_seq = Lq * q_tok_stride if q_seq_stride is None else q_seq_stride
    kv_seq = (0 if kv_off else Lk * kv_tok_stride) if kv_seq_stride is None else kv_seq_stride
    one = 256                                           # non-null, 16-byte aligned
    route = _L().vq_attn_fwd_route(one, one, one, one, n_seq, Lq, Lk, H, D, q_seq, q_tok_stride, kv_seq, kv_tok_stride,
                                   Lq * H * D, H * D, one if kv_off else None, 1.0, None)
    return route in ATTN_FWD_STATIC_ROUTES


def attn_fwd_rowquant_static(q, k, v, n_seq, Lq, Lk, H, D, q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride,
                             delta: torch.Tensor, zp: torch.Tensor, n_bits: int = 8,
                             kv_off: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                             o: Optional[torch.Tensor] = None, o_seq_stride: int = 0, o_tok_stride: int = 0,
                             s: Optional[torch.Tensor] = None, Kp: Optional[int] = None) -> Optional[QAct]:
    """:func:`attn_fwd` + the consuming Linear's STATIC tensor-wise quantizer - ``delta`` / ``zp``: one fp32 value each,
    read on the device - at ``n_bits`` (2..8) in one kernel.  Returns what ``rowquant(o.view(1, n_seq*Lq, H*D), n_bits,
    s=s, delta=delta, zp=zp)`` returns for the fp16 output ``o`` of :func:`attn_fwd` (also written when given, with its
    strides; bit-identical to attn_fwd's), bit for bit.  ``s``: the consuming Linear's smoothing vector; None is returned
    (caller runs the two kernels) when its reciprocal form is not available.  A launch the entry point refuses raises:
    ask :func:`attn_fwd_static_ok` first."""
    s_rcp = _rcp_or_none(s)
    if s_rcp is _NO_RCP:
        return None
    _req_f16((q, "q"), (k, "k"), (v, "v"))
    _req_opt(kv_off, torch.int32, "kv_off")
    delta, zp = _tensorwise_grid(_flat_f32(delta, "delta"), _flat_f32(zp, "zp"), "attn_fwd_rowquant_static")
    Cc = H * D
    Kp = pad128(Cc) if Kp is None else Kp
    out, scale = _attn_qact(q, o, n_seq * Lq, Cc, Kp, n_bits, D, scale, None, strided=True)
    check(_L().vq_attn_fwd_rowquant_static(_p(q), _p(k), _p(v), _p(s), _p(s_rcp), _p(delta), _p(zp), *_qact_ptrs(out), _p(o),
                                           n_seq, Lq, Lk, H, D, q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride,
                                           o_seq_stride, o_tok_stride, _p(kv_off), Kp, n_bits, scale, _stream()),
          "vq_attn_fwd_rowquant_static")
    return out


# --------------------------------------------------------------------------- misc
def adaln_table(table: torch.Tensor, t0: torch.Tensor) -> torch.Tensor:
    """mod[J, B, C] fp32 = table[J, C] + t0[B, J*C]  (fp16 inputs); mod[j] is a contiguous [B, C]."""
    _req(table, torch.float16, "table")
    _req(t0, torch.float16, "t0")
    J, Cc = table.shape
    B = t0.shape[0]
    assert t0.numel() == B * J * Cc
    mod = torch.empty((J, B, Cc), dtype=torch.float32, device=table.device)
    check(_L().vq_adaln_table(_p(table), _p(t0), _p(mod), B, J, Cc, _stream()), "vq_adaln_table")
    return mod


ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2


def linear_f16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act_in: int = ACT_NONE,
               act_out: int = ACT_NONE) -> torch.Tensor:
    """act_out(act_in(x) @ w.T + bias) for the FP edge Linears (embedders, t_block, final layer, patch embedding as a
    matmul): x [..., K] fp16, w [N, K] fp16, bias [N] fp16; fp32 accumulation, fp16 result.  Rows of x and w may be
    further apart than K (a column slice of a wider matrix): the kernel takes both pitches."""
    _req_rows(x, torch.float16, "x")
    _req_rows(w, torch.float16, "w")
    K = x.shape[-1]
    N = w.shape[0]
    assert w.dim() == 2 and w.shape[1] == K and w.stride(1) == 1
    x2 = x.reshape(-1, K)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    if bias is not None:
        _req(bias, torch.float16, "bias")
        assert bias.numel() == N and bias.is_contiguous()
    M = x2.shape[0]
    out = torch.empty((M, N), dtype=torch.float16, device=x.device)
    check(_L().vq_linear_f16(_p(x2), _p(w), _p(bias), _p(out), M, N, K, x2.stride(0), w.stride(0), N, act_in, act_out,
                             _stream()), "vq_linear_f16")
    return out.reshape(*x.shape[:-1], N)


def cfg_ddim_step(cond: torch.Tensor, uncond: torch.Tensor, x: torch.Tensor, cfg: float, one_plus_k: float,
                  A: float, Bc: float, abar_prev: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(cond, torch.float32, "cond")
    _req(uncond, torch.float32, "uncond")
    _req(x, torch.float32, "x")
    n, Cc = x.shape[0], x.shape[1]
    inner = x[0, 0].numel()
    assert cond.shape[0] == n and cond.shape[1] == 2 * Cc and cond.shape == uncond.shape
    if out is None:
        out = torch.empty_like(x)
    check(_L().vq_cfg_ddim_step(_p(cond), _p(uncond), _p(x), _p(out), n, Cc, inner, float(cfg), float(one_plus_k),
                                float(A), float(Bc), float(abar_prev), _stream()), "vq_cfg_ddim_step")
    return out


# --------------------------------------------------------------------------- the fused steps of the t2i sampling loops
# DPM-Solver++ (vq_cfg_dpmpp_step) and the IDDPM posterior step (vq_cfg_ddpm_step) read the same kind of model output:
# [2n] elements of elem_mult * C * inner values, an element dense, the batch pitch free.  elem_mult is 1 for DPM-Solver++
# (eps [2n, C, ...]) and 2 for IDDPM (the learned-variance channels are in the element: eps [2n, 2C, ...]).
def _dense_strides(shape):
    out, acc = [], 1
    for d in reversed(shape):
        out.append(acc)
        acc *= int(d)
    return tuple(reversed(out))


def _step_geometry(eps, x, elem_mult):
    """(n, C, inner, ld_eps) of a step, or None when eps is not the model output described above for the latent ``x``
    [n, C, ...].  Shapes and strides only (no tensor is touched)."""
    es, xs = tuple(eps.shape), tuple(x.shape)
    if len(xs) < 2 or len(es) != len(xs) or es[0] != 2 * xs[0] or es[1] != elem_mult * xs[1] or es[2:] != xs[2:]:
        return None
    inner = 1
    for d in xs[2:]:
        inner *= int(d)
    if tuple(x.stride()) != _dense_strides(xs) or tuple(eps.stride())[1:] != _dense_strides(es)[1:]:
        return None
    return int(xs[0]), int(xs[1]), inner, int(eps.stride()[0])


def _step_ok(eps, x, elem_mult) -> bool:
    """The refusals of a step entry point (include/viditq.h) that depend on eps and x, asked before the launch: GPU
    tensors, fp32 x, fp16 / fp32 eps (VQ_EUNSUP), positive extents (VQ_EINVAL), and VQ_ESHAPE: the layout, ld_eps >=
    elem_mult * C * inner, and - the kernel moves 4 elements per access when inner % 4 == 0 - the pitch and both base
    addresses on that many elements."""
    if not (eps.is_cuda and x.is_cuda):
        return False
    if x.dtype != torch.float32 or eps.dtype not in (torch.float16, torch.float32):
        return False
    geo = _step_geometry(eps, x, elem_mult)
    if geo is None:
        return False
    n, Cc, inner, ld = geo
    if n <= 0 or Cc <= 0 or inner <= 0:
        return False
    V = 4 if inner % 4 == 0 else 1
    return (ld >= elem_mult * Cc * inner and ld % V == 0 and eps.data_ptr() % (eps.element_size() * V) == 0
            and x.data_ptr() % (4 * V) == 0)


def _step_front(eps, x, aux, aux_name, coef, elem_mult, layout, refuse, step, x_out, x_model):
    """What both step wrappers do before their launch: GPU tensors, fp32 x / ``aux`` (hist or noise) / coef, fp16 / fp32
    eps, the geometry (else the solver's ``layout`` message), the solver's own clause ``refuse`` = (bad, message), the
    counter, x_out (allocated when None) and x_model.  Returns (n, C, inner, ld_eps, x_out, xm_f16)."""
    for t, name in ((eps, "eps"), (x, "x"), (aux, aux_name), (coef, "coef")):
        _req_gpu(t, name)
    _req(x, torch.float32, "x")
    _req(aux, torch.float32, aux_name)
    _req(coef, torch.float32, "coef")
    if eps.dtype not in (torch.float16, torch.float32):
        raise VQError("eps must be float16 or float32, got %s" % eps.dtype)
    geo = _step_geometry(eps, x, elem_mult)
    if geo is None:
        raise VQError("eps must be %s for x [n, C, ...], dense within a batch element" % layout)
    if refuse[0]:
        raise VQError(refuse[1])
    _req_opt(step, torch.int32, "step")
    if x_out is None:
        x_out = torch.empty_like(x)
    else:
        _req(x_out, torch.float32, "x_out")
        assert x_out.shape == x.shape
    xm16 = 0
    if x_model is not None:
        if not x_model.is_cuda or not x_model.is_contiguous() or x_model.dtype not in (torch.float16, torch.float32):
            raise VQError("x_model must be a contiguous float16 or float32 GPU tensor")
        assert x_model.numel() == 2 * x.numel()
        xm16 = int(x_model.dtype == torch.float16)
    return (*geo, x_out, xm16)


def cfg_dpmpp_step_ok(eps, x) -> bool:
    """Whether vq_cfg_dpmpp_step takes a model output ``eps`` [2n, C, ...] and a latent ``x`` [n, C, ...] (_step_ok)."""
    return _step_ok(eps, x, 1)


def cfg_dpmpp_step(eps: torch.Tensor, x: torch.Tensor, hist: torch.Tensor, coef: torch.Tensor, row: int,
                   step: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None,
                   x_model: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One call of the fused guidance + x0 + DPM-Solver++ multistep update (vq_cfg_dpmpp_step): ``eps`` [2n, C, ...] the
    (uncond | cond) model output (fp16 / fp32, batch pitch free), ``x`` [n, C, ...] fp32, ``hist`` [3, n*C*inner] fp32,
    ``coef`` [n_rows, DPMPP_ROW] fp32 on the device; the row is ``row`` plus the device counter ``step`` (int32, one
    element) when given.  Returns x_out (may be ``x`` itself); ``x_model`` [2n, C, ...] (fp16 / fp32) receives it twice."""
    bad = hist.numel() != 3 * x.numel() or coef.dim() != 2 or coef.shape[1] != _lib.DPMPP_ROW
    n, Cc, inner, ld, x_out, xm16 = _step_front(
        eps, x, hist, "hist", coef, 1, "[2n, C, ...]",
        (bad, "hist must hold 3 x %d fp32 and coef rows of %d floats" % (x.numel(), _lib.DPMPP_ROW)), step, x_out, x_model)
    check(_L().vq_cfg_dpmpp_step(_p(eps), _p(x), _p(hist), _p(coef), _p(step), _p(x_out), _p(x_model), n, Cc, inner, ld,
                                 int(row), coef.shape[0], int(eps.dtype == torch.float16), xm16, _stream()),
          "vq_cfg_dpmpp_step")
    return x_out


def _patch_geometry(eps_u, eps_c, x, patch):
    """(n, C, C_out, T, H, W, ld_eps) of a patch-major step, or None when eps_u / eps_c are not two final_layer outputs
    [n, N_t*N_h*N_w, p_t*p_h*p_w*C_out] (same shape, strides and type, a sample dense, the sample pitch free) for the dense
    latent ``x`` [n, C, T, H, W] and the patch (p_t, p_h, p_w).  Shapes and strides only (no tensor is touched)."""
    es, xs = tuple(eps_u.shape), tuple(x.shape)
    if len(xs) != 5 or len(es) != 3 or len(patch) != 3 or tuple(eps_c.shape) != es or eps_c.dtype != eps_u.dtype:
        return None
    pt, ph, pw = (int(p) for p in patch)
    n, Cc, T, H, W = (int(d) for d in xs)
    if min(pt, ph, pw) <= 0 or T % pt or H % ph or W % pw:
        return None
    P = pt * ph * pw
    if es[0] != n or es[1] * P != T * H * W or es[2] % P:
        return None
    if tuple(x.stride()) != _dense_strides(xs) or tuple(eps_u.stride())[1:] != (es[2], 1) \
            or tuple(eps_c.stride()) != tuple(eps_u.stride()):
        return None
    return n, Cc, int(es[2]) // P, T, H, W, int(eps_u.stride()[0])


def _patch_ok(eps_a, eps_b, x, patch) -> bool:
    """The refusals of a patch-major entry point (include/viditq.h) that depend on the two model outputs and the latent,
    asked before the launch from shapes, strides and addresses: GPU tensors, fp32 x, fp16 / fp32 eps and patch extents of 1
    or 2 (VQ_EUNSUP), positive extents (VQ_EINVAL), and VQ_ESHAPE: the layout, C <= C_out, ld_eps >= T*H*W*C_out and the
    pitch and the base addresses on the elements of an access (4 channels x 2 along w when C == 4, C_out % 4 == 0 and
    W % 2 == 0, else 1 x 1)."""
    if not (eps_a.is_cuda and eps_b.is_cuda and x.is_cuda):
        return False
    if x.dtype != torch.float32 or eps_a.dtype not in (torch.float16, torch.float32):
        return False
    geo = _patch_geometry(eps_a, eps_b, x, patch)
    if geo is None or any(int(p) not in (1, 2) for p in patch):
        return False
    n, Cc, Co, T, H, W, ld = geo
    if min(n, Cc, Co, T, H, W) <= 0 or Cc > Co or ld < T * H * W * Co:
        return False
    wide = Cc == 4 and Co % 4 == 0 and W % 2 == 0
    VC, VW = (4, 2) if wide else (1, 1)
    ea = eps_a.element_size() * VC
    return ld % VC == 0 and eps_a.data_ptr() % ea == 0 and eps_b.data_ptr() % ea == 0 and x.data_ptr() % (4 * VW) == 0


def _patch_front(eps_a, eps_b, names, x, aux, coef, row_len, refuse, patch, step, x_out, x_model):
    """What both patch-major wrappers do before their launch: GPU tensors, fp32 x / ``aux`` (name -> tensor) / coef,
    fp16 / fp32 eps, the geometry, coef rows of ``row_len`` floats and the solver's own clause ``refuse`` = (bad, message),
    the counter, x_out (allocated when None) and x_model.  Returns (n, C, C_out, T, H, W, ld_eps, p_t, p_h, p_w, x_out,
    xm_f16, xm_copies)."""
    for t, name in ((eps_a, names[0]), (eps_b, names[1]), (x, "x"), *((v, k) for k, v in aux.items()), (coef, "coef")):
        _req_gpu(t, name)
    _req(x, torch.float32, "x")
    for k, v in aux.items():
        _req(v, torch.float32, k)
    _req(coef, torch.float32, "coef")
    if eps_a.dtype not in (torch.float16, torch.float32):
        raise VQError("eps must be float16 or float32, got %s" % eps_a.dtype)
    geo = _patch_geometry(eps_a, eps_b, x, patch)
    if geo is None:
        raise VQError("%s / %s must be [n, tokens, p_t*p_h*p_w*C_out] with equal strides for x [n, C, T, H, W]" % names)
    if refuse[0] or coef.dim() != 2 or coef.shape[1] != row_len:
        raise VQError(refuse[1])
    _req_opt(step, torch.int32, "step")
    if x_out is None:
        x_out = torch.empty_like(x)
    else:
        _req(x_out, torch.float32, "x_out")
        assert x_out.shape == x.shape
    xm16, copies = 0, 1
    if x_model is not None:
        if not x_model.is_cuda or not x_model.is_contiguous() or x_model.dtype not in (torch.float16, torch.float32):
            raise VQError("x_model must be a contiguous float16 or float32 GPU tensor")
        copies = x_model.numel() // x.numel()
        assert x_model.numel() == copies * x.numel()
        xm16 = int(x_model.dtype == torch.float16)
    return (*geo, *(int(p) for p in patch), x_out, xm16, copies)


def cfg_dpmpp_step_patch_ok(eps_u, eps_c, x, patch) -> bool:
    """Whether vq_cfg_dpmpp_step_patch takes the two model outputs and the latent (_patch_ok)."""
    return _patch_ok(eps_u, eps_c, x, patch)


def cfg_dpmpp_step_patch(eps_u: torch.Tensor, eps_c: torch.Tensor, x: torch.Tensor, hist: torch.Tensor, coef: torch.Tensor,
                         row: int, patch, step: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None,
                         x_model: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One call of the DPM-Solver++ step of cfg_dpmpp_step on the patch-major model output (vq_cfg_dpmpp_step_patch):
    ``eps_u`` / ``eps_c`` the uncond / cond outputs of final_layer [n, tokens, p_t*p_h*p_w*C_out] (fp16 / fp32, sample pitch
    free; the two halves of one joint output, or the outputs of two forwards), ``x`` [n, C, T, H, W] fp32, ``patch``
    (p_t, p_h, p_w); hist, coef, row and step as for cfg_dpmpp_step.  All arithmetic is fp32.  Returns x_out (may be ``x``
    itself); ``x_model`` [n or 2n, C, T, H, W] (fp16 / fp32) receives it once or twice."""
    n, Cc, Co, T, H, W, ld, pt, ph, pw, x_out, xm16, copies = _patch_front(
        eps_u, eps_c, ("eps_u", "eps_c"), x, {"hist": hist}, coef, _lib.DPMPP_ROW,
        (hist.numel() != 3 * x.numel(), "hist must hold 3 x %d fp32 and coef rows of %d floats" % (x.numel(), _lib.DPMPP_ROW)),
        patch, step, x_out, x_model)
    check(_L().vq_cfg_dpmpp_step_patch(_p(eps_u), _p(eps_c), _p(x), _p(hist), _p(coef), _p(step), _p(x_out), _p(x_model), n,
                                       Cc, Co, T, H, W, pt, ph, pw, ld, int(row), coef.shape[0],
                                       int(eps_u.dtype == torch.float16), xm16, copies, _stream()), "vq_cfg_dpmpp_step_patch")
    return x_out


def cfg_ddim_step_patch_ok(eps_c, eps_u, x, patch) -> bool:
    """Whether vq_cfg_ddim_step_patch takes the two model outputs and the latent (_patch_ok)."""
    return _patch_ok(eps_c, eps_u, x, patch)


def cfg_ddim_step_patch(eps_c: torch.Tensor, eps_u: torch.Tensor, x: torch.Tensor, rows: torch.Tensor, row: int, patch,
                        step: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None,
                        x_model: Optional[torch.Tensor] = None, guided: int = 3) -> torch.Tensor:
    """One call of the DDIM(eta = 0) step of cfg_ddim_step on the patch-major model output (vq_cfg_ddim_step_patch):
    ``eps_c`` / ``eps_u`` the cond / uncond outputs of final_layer [n, tokens, p_t*p_h*p_w*C_out] (fp16 / fp32, sample pitch
    free; the two halves of one joint output, or the outputs of two forwards), ``x`` [n, C, T, H, W] fp32, ``rows``
    [n_rows, DDIM_ROW] fp32 on the device (IDDPM.ddim_rows); the row is ``row`` plus the device counter ``step`` (int32, one
    element) when given.  Guidance on the channels below ``guided``.  Bit for bit cfg_ddim_step on the unpatchified fp32
    tensor.  Returns x_out (may be ``x`` itself); ``x_model`` [n or 2n, C, T, H, W] (fp16 / fp32) receives it once or twice."""
    n, Cc, Co, T, H, W, ld, pt, ph, pw, x_out, xm16, copies = _patch_front(
        eps_c, eps_u, ("eps_c", "eps_u"), x, {}, rows, _lib.DDIM_ROW,
        (int(guided) < 0, "guided must be >= 0 and rows must have %d floats" % _lib.DDIM_ROW), patch, step, x_out, x_model)
    check(_L().vq_cfg_ddim_step_patch(_p(eps_c), _p(eps_u), _p(x), _p(rows), _p(step), _p(x_out), _p(x_model), n, Cc, Co, T,
                                      H, W, pt, ph, pw, ld, int(guided), int(row), rows.shape[0],
                                      int(eps_c.dtype == torch.float16), xm16, copies, _stream()), "vq_cfg_ddim_step_patch")
    return x_out


def dpmpp_advance(step: torch.Tensor, coef: torch.Tensor, t_out: torch.Tensor) -> None:
    """t_out[:] = the counter's row's next model-input time, then the counter moves on (saturating at the last row):
    vq_dpmpp_advance, enqueued after a table-driven step(step=counter) (T_NEXT is the same column in every row layout)."""
    _req(step, torch.int32, "step")
    _req(coef, torch.float32, "coef")
    _req(t_out, torch.float32, "t_out")
    assert coef.dim() == 2 and coef.shape[1] == _lib.DPMPP_ROW
    check(_L().vq_dpmpp_advance(_p(step), _p(coef), coef.shape[0], _p(t_out), t_out.numel(), _stream()), "vq_dpmpp_advance")


def cfg_ddpm_step_ok(eps, x) -> bool:
    """Whether vq_cfg_ddpm_step takes a model output ``eps`` [2n, 2C, ...] and a latent ``x`` [n, C, ...] (_step_ok)."""
    return _step_ok(eps, x, 2)


def cfg_ddpm_step(eps: torch.Tensor, x: torch.Tensor, noise: torch.Tensor, coef: torch.Tensor, row: int,
                  step: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None,
                  x0_out: Optional[torch.Tensor] = None, x_model: Optional[torch.Tensor] = None,
                  guided: int = 3) -> torch.Tensor:
    """One call of the fused guidance + learned-range variance + posterior step (vq_cfg_ddpm_step): ``eps`` [2n, 2C, ...]
    the (cond | uncond) model output (fp16 / fp32, batch pitch free), ``x`` and ``noise`` [n, C, ...] fp32, ``coef``
    [n_rows, DDPM_ROW] fp32 on the device; the row is ``row`` plus the device counter ``step`` (int32, one element) when
    given.  Returns x_out (may be ``x`` itself); ``x0_out`` receives pred_xstart, ``x_model`` [2n, C, ...] (fp16 / fp32)
    the sample twice."""
    bad = noise.shape != x.shape or coef.dim() != 2 or coef.shape[1] != _lib.DDPM_ROW
    n, Cc, inner, ld, x_out, xm16 = _step_front(
        eps, x, noise, "noise", coef, 2, "[2n, 2C, ...]",
        (bad, "noise must have x's shape and coef rows of %d floats" % _lib.DDPM_ROW), step, x_out, x_model)
    if x0_out is not None:
        _req(x0_out, torch.float32, "x0_out")
        assert x0_out.shape == x.shape
    check(_L().vq_cfg_ddpm_step(_p(eps), _p(x), _p(noise), _p(coef), _p(step), _p(x_out), _p(x0_out), _p(x_model), n, Cc,
                                inner, ld, int(guided), int(row), coef.shape[0], int(eps.dtype == torch.float16), xm16,
                                _stream()), "vq_cfg_ddpm_step")
    return x_out



def cfg_sa_step_ok(eps, x) -> bool:
    """Whether vq_cfg_sa_step takes a model output ``eps`` [2n, C, ...] and a latent ``x`` [n, C, ...] (_step_ok)."""
    return _step_ok(eps, x, 1)


def cfg_sa_step(eps: torch.Tensor, x: torch.Tensor, xp: torch.Tensor, hist: torch.Tensor, noise: torch.Tensor,
                coef: torch.Tensor, row: int, step: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None,
                xp_out: Optional[torch.Tensor] = None, x_model: Optional[torch.Tensor] = None):
    """One call of the fused guidance + x0 + SA-Solver corrector + next predictor (vq_cfg_sa_step): ``eps`` [2n, C, ...] the
    (uncond | cond) model output (fp16 / fp32, batch pitch free), ``x`` (the corrected sample of the previous step) and
    ``xp`` (the predicted sample the model saw) [n, C, ...] fp32, ``hist`` [2, n*C*inner] fp32, ``noise`` the ring
    [2, n*C*inner] fp32, ``coef`` [n_rows, SA_ROW] fp32 on the device; the row is ``row`` plus the device counter ``step``
    (int32, one element) when given.  Returns (x_out, xp_out) (may be ``x`` / ``xp`` themselves); ``x_model`` [2n, C, ...]
    (fp16 / fp32) receives xp_out twice."""
    bad = (hist.numel() != 2 * x.numel() or noise.numel() != 2 * x.numel() or xp.shape != x.shape or not xp.is_cuda
           or xp.dtype != torch.float32 or not xp.is_contiguous() or not noise.is_cuda or noise.dtype != torch.float32
           or not noise.is_contiguous() or coef.dim() != 2 or coef.shape[1] != _lib.SA_ROW)
    n, Cc, inner, ld, x_out, xm16 = _step_front(
        eps, x, hist, "hist", coef, 1, "[2n, C, ...]",
        (bad, "xp must be an fp32 GPU tensor of x's shape, hist and the noise ring must hold 2 x %d fp32 and coef rows of "
              "%d floats" % (x.numel(), _lib.SA_ROW)), step, x_out, x_model)
    if xp_out is None:
        xp_out = torch.empty_like(x)
    else:
        _req(xp_out, torch.float32, "xp_out")
        assert xp_out.shape == x.shape
    check(_L().vq_cfg_sa_step(_p(eps), _p(x), _p(xp), _p(hist), _p(noise), _p(coef), _p(step), _p(x_out), _p(xp_out),
                              _p(x_model), n, Cc, inner, ld, int(row), coef.shape[0], int(eps.dtype == torch.float16), xm16,
                              _stream()), "vq_cfg_sa_step")
    return x_out, xp_out

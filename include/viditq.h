/*
 * viditq.h - C ABI of libviditq_hip.so: the MI355X (gfx950) kernels of the
 * quantized-DiT denoising path.
 *
 * The reference (thu-nics/ViDiT-Q) has no FFI layer: its operator API is the
 * Python class surface of qdiff.  Each entry point below
 * replaces the torch ops executed by the cited reference lines; the Python
 * host package (vidit-q_amd) binds them with ctypes and keeps the reference's
 * class/method names on top.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; no hidden
 *     allocation, no host synchronisation; work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream);
 *   - return value: VQ_OK (0) or a negative VQ_E* code; nothing throws;
 *   - activations are fp16 (`uint16_t` bit patterns, IEEE binary16), row-major,
 *     rows contiguous; quantized activations are int8 `code - cx` with row
 *     stride `Kp` (a multiple of 128 bytes, the tail beyond K is zero);
 *   - "row" r of an activation [B, n_tok, C] is r = b*n_tok + tok; per-token
 *     quant parameters are shared over b (reference quirk) and
 *     are stored replicated per row so the GEMM never needs n_tok.
 *
 * Integer form computed by the GEMMs:
 *   out[m,n] = sx[m]*sw[n] * ( acc[m,n] - zw[n]*R[m] - zx[m]*cs[n] ) + bias[n]
 *   acc = sum_k xs[m,k]*ws[n,k];  xs = code_x - cx, ws = code_w - cw
 *   zx = zp_x - cx, zw = zp_w - cw, cs[n] = sum_k ws[n,k],
 *   R[m] = sum_k xs[m,k] - K*zx[m]
 */
#ifndef VIDITQ_H
#define VIDITQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQ_OK 0
#define VQ_EINVAL (-1)   /* bad argument (null pointer, non-positive size) */
#define VQ_ESHAPE (-2)   /* unsupported shape / alignment */
#define VQ_ELAUNCH (-3)  /* hip launch error (see vq_last_hip_error) */
#define VQ_EUNSUP (-4)   /* unsupported bit-width / mode */

/* status-word bits written by the quantizing kernels (device int32) */
#define VQ_ST_EPSFILL 1  /* some token had delta < 1e-6: the reference would fill
                            EVERY delta with 1e-6 (base_quantizer.py:220-222) */

/* GEMM kernel choice: VQ_GEMM_DEFAULT lets the library choose per shape; an explicit number pins one kernel
 * (11 = full-line LDS-DMA ring, one 256 x 288 tile per 8-wave workgroup).  Retired generations and profiling
 * ablations are not part of this library (tools/lab). */
#define VQ_GEMM_DEFAULT (-1)

/* GEMM epilogues */
#define VQ_EPI_NONE 0        /* out = y                                        */
#define VQ_EPI_GELU 1        /* out = gelu_tanh(y)      (mlp.fc1 -> act)       */
#define VQ_EPI_GATE_RESID 2  /* out = resid + gate[b,n]*y   (x = x + gate*f(x)) */
#define VQ_EPI_RESID 3       /* out = resid + y             (x = x + cross(x)) */

int vq_version(void);
const char* vq_strerror(int code);
int vq_last_hip_error(void);

/* ---- per-token dynamic activation quantizer ------------------------------
 * Replaces DynamicActQuantizer.forward (qdiff/quantizer/dynamic_quantizer.py:
 * 16-45) + init_quant_params token branch (base_quantizer.py:177-228) as used
 * by every QuantLayer subclass (quant_layer.py:157-165, stdit_quant_layer.py:
 * 68-73,159-164,270-281), optionally preceded by the smooth-quant division
 * x / s (quant_layer.py:140) and the temporal pos-embed add (stdit.py:113-114).
 *
 * x        [B*n_tok, C] fp16
 * add_rows nullable [n_add, C] fp16 added to row r as add_rows[(r % n_tok) / add_div]
 * s        nullable [C] fp32 smooth-quant channel scale; x is DIVIDED by s in-kernel
 *          (correctly rounded division, bit-exact with the reference's x / s)
 * s_rcp    nullable [C] fp32 RN(1 / s) from vq_smooth_reciprocal (only when it reported 0 bad channels): the
 *          same quotient in 3 instead of ~12 instructions per element; without it the kernels divide the IEEE way
 * xq       [B*n_tok, Kp] int8 (code - cx, cx = 128 when n_bits==8 else 0)
 * sx       [B*n_tok] fp32 delta      zx [B*n_tok] int32 (zp - cx)
 * R        [B*n_tok] int32           zpf nullable [B*n_tok] fp32 (raw zero point)
 * delta_in/zp_in nullable: a static, calibrated grid (ActQuantizer after init_done,
 *          base_quantizer.py:129-144) of n_param = 1 (tensor-wise) or n_tok entries;
 *          when given, no min/max is taken
 * status   nullable device int32 (bit VQ_ST_EPSFILL or-ed in)
 */
int vq_rowquant(const void* x, const void* add_rows, int n_add, int add_div, const float* s, const float* s_rcp,
                int8_t* xq, float* sx, int32_t* zx, int32_t* R, float* zpf,
                const float* delta_in, const float* zp_in, int n_param,
                int B, int n_tok, int C, int Kp, int n_bits, int32_t* status, void* stream);

/* GELU(tanh) + x / s + per-token dynamic quantizer in ONE pass over x [1, n_tok, C] fp16.
 * Replaces, for the second MLP Linear: Mlp.act (nn.GELU(approximate="tanh"), t2v/opensora/models/layers/blocks.py:27,
 * applied to the fc1 output) followed by the fc2 activation quantizer (qdiff/models/quant_layer.py:136-160 +
 * qdiff/quantizer/dynamic_quantizer.py:16-45).  The fc1 GEMM is then launched with VQ_EPI_NONE: the activation's
 * exp/rcp run under this HBM-bound kernel instead of the MFMA-bound GEMM epilogue.  GELU output is rounded to fp16
 * before quantization (the activation dtype of the reference pipeline).  B = 1, or B = 2 with x [2, n_tok, C] and the
 * grid of a token shared by its two samples (base_quantizer.py:185: the t2i loop's uncond | cond forward; outputs
 * indexed by row = sample * n_tok + token with the shared step replicated, as vq_rowquant writes them; with a smoothing
 * vector only rows longer than 1536 channels).  Larger batches: VQ_EUNSUP (use the GEMM's GELU epilogue + vq_rowquant).
 * Outputs as vq_rowquant. */
int vq_gelu_rowquant(const void* x, const float* s, const float* s_rcp, int8_t* xq, float* sx, int32_t* zx, int32_t* R,
                     int B, int n_tok, int C, int Kp, int n_bits, int32_t* status, void* stream);

/* Same, fused with LayerNorm(eps, no affine) + AdaLN modulate:
 *   x_m = LN(x) * (1 + scale[b]) + shift[b]       (stdit.py:100-103,124)
 * shift/scale: fp32 [B, C] (already scale_shift_table + t0 chunk).
 * Up to three smoothing vectors s0..s2 produce up to three quantized copies
 * (q/k/v each balance against their own weight, quant_layer.py:136); n_out>=1.
 * xm_out nullable [B*n_tok, C] fp16: the modulated activation itself.
 */
int vq_ln_modulate_rowquant(const void* x, const float* shift, const float* scale, float ln_eps,
                            int n_out, const float* const* s, const float* const* s_rcp, int8_t* const* xq, float* const* sx,
                            int32_t* const* zx, int32_t* const* R, void* xm_out,
                            int B, int n_tok, int C, int Kp, int n_bits, int32_t* status, void* stream);

/* n_out (1..3) smoothed per-token quantizers of the SAME input x [n_tok, C] (B == 1) in one launch: output j is
 * vq_rowquant(x, s[j], s_rcp[j]).  The q / k / v activation quantizers of a plan that balances each Linear against
 * its own weight (quant_layer.py:136-160), where no LayerNorm precedes them (temporal attention, stdit.py:112-118).
 * Arrays are HOST arrays of device pointers, reciprocals mandatory.  Shapes outside the reciprocal-form kernel
 * (C % 128, 768 <= C <= 1280, Kp == C, n_tok >= 2) return VQ_EUNSUP - call vq_rowquant per output instead. */
int vq_rowquant_smooth_multi(const void* x, int n_out, const float* const* s, const float* const* s_rcp,
                             int8_t* const* xq, float* const* sx, int32_t* const* zx, int32_t* const* R,
                             int n_tok, int C, int Kp, int n_bits, int32_t* status, void* stream);

/* The same for a JOINT forward over cat([x, x]) (cfg_split: False; iddpm/__init__.py:141-163): x [2, n_tok, C] fp16 and
 * n_out (1..3) smoothed per-token dynamic quantizers from ONE pass over the rows, the grid of a token shared by its rows
 * of both samples (base_quantizer.py:177-189, line 185), outputs indexed by row = sample * n_tok + token with the shared
 * step replicated, as vq_rowquant(B = 2) writes them.  Input arm, one of:
 *   plain (shift = scale = NULL): output j is vq_rowquant(x, s[j], s_rcp[j], B = 2), bit for bit - the q / k / v
 *   quantizers of temporal attention (stdit.py:112-118; quant_layer.py:136-160; dynamic_quantizer.py:16-45);
 *   LayerNorm(ln_eps, no affine) + (1 + scale[b]) * y + shift[b] (shift / scale fp32 [2, C], both set; stdit.py:100-103,
 *   124; layers/blocks.py:51): output j is vq_ln_modulate_rowquant(n_out = 1, s[j], B = 2), bit for bit.
 * s, s_rcp, xq, sx, zx, R are HOST arrays of n_out device pointers, reciprocals (vq_smooth_reciprocal) mandatory.
 * There is no xm_out and there are no added rows.
 * Errors, each before any device call or dereference of a device pointer, checked in this order: VQ_EINVAL for a null
 * required pointer or array entry below n_out, exactly one of shift / scale, n_out outside 1..3, a non-positive B, n_tok
 * or C; VQ_ESHAPE for C % 8, Kp % 128 or Kp < C and VQ_EUNSUP for n_bits outside 2..8; VQ_ESHAPE for x, shift, scale, s[j],
 * s_rcp[j] or xq[j] off 16 bytes; VQ_EUNSUP for B != 2, a width other than 768, 1024, 1152 or 1280, or Kp != C - the
 * caller then runs one launch per output. */
int vq_rowquant_smooth_multi_shared(const void* x, const float* shift, const float* scale, float ln_eps, int n_out,
                                    const float* const* s, const float* const* s_rcp, int8_t* const* xq, float* const* sx,
                                    int32_t* const* zx, int32_t* const* R, int B, int n_tok, int C, int Kp, int n_bits,
                                    int32_t* status, void* stream);

/* One pass over x [B, n_tok, C] fp16 -> n_out (1..3) quantized copies on STATIC calibrated grids: ActQuantizer.forward
 * after init_done (qdiff/quantizer/base_quantizer.py:129-144) for Linears that share an input (q / k / v), with what
 * precedes them in a block in the same pass.  Input arm, one of:
 *   plain;
 *   + add_rows[(r % n_tok) / add_div] (fp16 [n_add, C]: the temporal position embedding, stdit.py:112-114);
 *   LayerNorm(ln_eps, no affine) + (1 + scale[b]) * y + shift[b] (shift / scale fp32 [B, C], both set; stdit.py:103,124,
 *   layers/blocks.py:51), rounded to fp16 - the activation the reference stores - before it is quantized; xm_out
 *   (nullable, [B*n_tok, C] fp16) receives it, bit-identical to vq_ln_modulate_rowquant(n_out = 1, s = NULL, xm_out).
 * Output j: u = v / s[j][c] when s[j] is set (quant_layer.py:140; the reciprocal form only when s_rcp[j] is given too),
 *   code = clamp(rint(u / delta_j) + zp_j, 0, 2^n_bits - 1)   (base_quantizer.py:134-140),
 * with the grid (delta[j], zp[j]) of n_param entries (1 = tensor-wise, or n_tok: entry tok serves every b) read on the
 * device - no host synchronisation.  xq / sx / zx / R as vq_rowquant writes them (sx[r] = delta, zx[r] = (int)zp - cx,
 * R[r] = sum(xq) - C * zx[r], pad columns [C, Kp) zero).  There is no status word: a static grid has no eps fill.
 * s, s_rcp, delta, zp, xq, sx, zx, R are HOST arrays of n_out device pointers (s / s_rcp nullable, as may be their
 * entries).  Precondition: zp integer-valued and delta > 0, as every calibrated grid is.
 * Errors, all before anything is dereferenced or launched: VQ_EINVAL for a null pointer, a non-positive extent, n_out
 * outside 1..3, n_param not in {1, n_tok}; VQ_ESHAPE for C % 8, Kp % 128, Kp < C or a pointer off 16 bytes (x, add_rows,
 * shift, scale, xm_out, s[j], s_rcp[j], xq[j]); VQ_EUNSUP for add_rows together with LayerNorm, n_bits outside 2..8 or
 * Kp > 4608. */
int vq_rowquant_static(const void* x, const void* add_rows, int n_add, int add_div,
                       const float* shift, const float* scale, float ln_eps,
                       int n_out, const float* const* s, const float* const* s_rcp,
                       const float* const* delta, const float* const* zp, int n_param,
                       int8_t* const* xq, float* const* sx, int32_t* const* zx, int32_t* const* R,
                       void* xm_out, int B, int n_tok, int C, int Kp, int n_bits, void* stream);

/* Reciprocal of a smooth-quant channel scale for the s_rcp arguments above: r[c] = RN(1 / s[c]); *n_bad (device int32,
 * zeroed by the caller) counts the channels for which the reciprocal form of x / s is not guaranteed bit-exact
 * (s not a positive normal number, significand all ones, reciprocal not normal): pass s_rcp only when it stays 0.
 * Replaces nothing in the reference - it is how `x / s` (quant_layer.py:140) is evaluated here. */
int vq_smooth_reciprocal(const float* s, float* r, int n, int32_t* n_bad, void* stream);
/* Test hook: fast[i] = a[i] / b[i] through the reciprocal form, exact[i] = the IEEE quotient. */
int vq_smooth_div_check(const float* a, const float* b, float* fast, float* exact, long n, void* stream);

/* Quantize->dequantize (the reference's fake-quant result), exact incl. the
 * global eps-fill rule; the operator behind BaseQuantizer.forward for
 * activations (base_quantizer.py:112-144, dynamic_quantizer.py:16-45).
 * mode 0: per-token dynamic (delta/zp computed, written to delta_out/zp_out [n_tok])
 * mode 1: static (delta_in/zp_in given: 1 element tensor-wise or n_tok per-token)
 * codes nullable [B*n_tok, C] uint8 raw codes.  `scratch` = 1 device float (mode 0).
 */
int vq_fakequant_act(const void* x, void* out, uint8_t* codes, float* delta_out, float* zp_out,
                     const float* delta_in, const float* zp_in, int n_param,
                     int B, int n_tok, int C, int n_bits, int mode, float* scratch,
                     int32_t* status, void* stream);

/* Global eps-fill fix-up behind the integer route of a few-row Linear whose input is not normalised (the prompt
 * tokens into cross_attn.kv_linear).  base_quantizer.py:219-223 sets EVERY token's step to 1e-6 as soon as one token's
 * step is below 1e-6; vq_rowquant raises VQ_ST_EPSFILL in `flag` for that case instead.  When the flag is clear the
 * kernel returns at once; when it is set, out[g, row, :] is overwritten with the reference's fp16-mode result:
 * (x / s rounded to fp16) -> exact quantize / dequantize on the step-1e-6 grid -> fp32 contraction with the
 * dequantized fp16 weight wdq [n_batch, N, C] (+ bias [n_batch, N] fp16, nullable) -> fp16.
 * x [L, C] fp16 (shared by the batch), s nullable [C] fp32, out [n_batch, L, N] fp16. */
int vq_epsfill_fixup(const int32_t* flag, const void* x, const float* s, const void* wdq, const void* bias,
                     void* out, int n_batch, int L, int C, int N, int n_bits, void* stream);

/* ---- running smooth-quant act-scale statistic, device-resident ---------------
 * Replaces QuantLayer's momentum statistic where a script leaves it running at inference (quant_txt2img.py:297-300):
 * the update of qdiff/models/quant_layer.py:118-126 and :147-154,
 *   cur = input.abs().amax(dim=-2).mean(dim=0);  act_scale = cur if act_scale.abs().mean() == 0
 *                                                else act_scale * momentum + cur * (1 - momentum),
 * followed by the zero patch of the channel-wise scale (:128-133: entries that are exactly zero become 1e-5) - with the
 * two host-visible tests of the reference evaluated on the device: no synchronisation, capturable in a graph.
 * x          [B, n_tok, C] fp16, rows contiguous, finite values
 * act_scale  [C] fp32 device state, updated in place (one time range's slice of act_quantizer.act_scale)
 * cur_out    nullable [C] fp32: this call's cur
 * scratch    [B*C] uint32 owned by the caller; zeroed by this call on `stream` (a small kernel) - callers do not pre-zero
 * Contract:
 *   m[b][c] = max over tok of |x[b, tok, c]| as fp16, taken as the integer maximum of `bits & 0x7fff` (independent of the
 *     order of rows and workgroups: the integer atomic between workgroups is bit-reproducible);
 *   cur[c] = (float(m[0][c]) + float(m[1][c]) + ... in order b = 0 .. B-1) / B;
 *   every entry of act_scale zero: act_scale = cur; otherwise
 *   act_scale[c] = RN(RN(act_scale[c] * momentum) + RN(cur[c] * one_minus_momentum)) - three fp32 roundings, no fma; the
 *     host passes one_minus_momentum = (float)(1.0 - momentum) evaluated in double, as torch does for a Python scalar;
 *   then entries of act_scale that are exactly zero become 1.0e-5f.
 * Bit-exact against the reference lines on the CPU (for B > 2 up to the reference's own summation order).
 * Errors, all before any HIP call or dereference, null pointers first: VQ_EINVAL for a null x, act_scale or scratch, a
 * non-positive extent, B > 65535, B*C beyond int32, a momentum outside [0, 1]; VQ_ESHAPE for C % 8 or x off 16 bytes. */
int vq_act_scale_momentum(const void* x, float* act_scale, float* cur_out, uint32_t* scratch,
                          float momentum, float one_minus_momentum,
                          int B, int n_tok, int C, void* stream);

/* ---- weight packer ---------------------------------------------------------
 * Replaces WeightQuantizer.forward on W*s (base_quantizer.py:129-144 via
 * quant_layer.py:174-185): codes = clamp(round(W*s/delta)+zp, 0, 2^b-1) on the
 * grid (delta, zp) given per out-channel; emits ws = code - cw as int8 [N, Kp]
 * (n_bits > 4) or packed nibbles [N, Kp/2] (n_bits <= 4; per group of 8 k, byte j
 * holds code[k0+j] in the low and code[k0+4+j] in the high nibble - pack.hip),
 * zw[n] = zp - cw, sw[n] = delta, cs[n] = sum_k ws.  cw = 128 iff n_bits == 8.
 * W [N,K] fp16; s nullable [K] fp32; delta, zp [N] fp32.
 */
int vq_pack_weight(const void* W, const float* s, const float* delta, const float* zp,
                   void* wq, float* sw, int32_t* zw, int32_t* cs,
                   int N, int K, int Kp, int n_bits, void* stream);

/* Per-out-channel min-max grid of W*s (base_quantizer.py:168-172,191-228):
 * delta[n], zp[n] for one bit-width; status gets VQ_ST_EPSFILL like above and
 * a second call with force_eps=1 reproduces the fill. */
int vq_weight_minmax(const void* W, const float* s, float* delta, float* zp,
                     int N, int K, int n_bits, int force_eps, int32_t* status, void* stream);

/* ---- int8 MFMA GEMM with fused dequant epilogue ----------------------------
 * Replaces F.linear(x_hat, W_hat, bias) of quant_layer.py:211 /
 * stdit_quant_layer.py:96,187,304 / dit_quant_layer.py:29,76 (and, by
 * epilogue, nn.GELU(tanh) of modules.py:57 and the gate/residual adds of
 * stdit.py:109,118,121,128).
 * xq [M,Kp] int8, wq [N,Kp] int8 (w_bits>4) or [N,Kp/2] nibbles (w_bits<=4)
 * bias nullable [N] fp32; out [M, ldo] fp16 written at columns [0,N)
 * resid nullable [M, ldo] fp16; gate nullable fp32 [M/rows_per_gate, N]
 * variant: VQ_GEMM_DEFAULT (form chosen by shape), or a pinned form of the same kernel -
 *   11: 256 x 288 tile, 8 waves, general form (any M, N);  16: 128 x 288 tile, general form;
 *   19: 256 x 288 tile, interior form (scalar-addressed stage pieces, one wave per SIMD issues them) - what
 *       VQ_GEMM_DEFAULT picks for launches made of interior tiles;
 *   19 returns VQ_ESHAPE unless M % 256 == 0, N % 288 == 0, ldo % 8 == 0 and - VQ_EPI_GATE_RESID - rows_per_gate % 256
 *   == 0 (VQ_GEMM_DEFAULT falls back to the general form instead).  All forms give bit-identical results.
 */
int vq_gemm_i8(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R,
               const void* wq, const float* sw, const int32_t* zw, const int32_t* cs,
               const float* bias, void* out, int ldo, const void* resid, const float* gate,
               int rows_per_gate, int M, int N, int K, int Kp, int w_bits, int epilogue,
               int variant, void* stream);

/* Diagnostics (bench telemetry, no reference counterpart): ONE launch of the default 8-bit kernel (256 x 288 tile,
 * plain epilogue) whose waves also stamp the shader cycle counter and the chip's 100 MHz wall clock - what clock the
 * GEMM actually ran at on THIS box (bench.py reports it beside every rate; a power-bound part runs 1.8-2.1 of its
 * nominal 2.4 GHz).  stamps [tiles][8 waves][10] int64, tiles = ceil(M/256) * ceil(N/288): 0-6 shader cycles at entry /
 * first stage landed / main loop end / parameters staged / slabs written / stores issued / stores drained, 7 and 8 the
 * wall clock at entry and exit (10 ns ticks), 9 the shader cycle at which the wave arrived at the stage barrier of k-tile 1 (0 when
 * the problem has fewer than three k-tiles).  n_stamps = capacity of `stamps` in int64 (VQ_ESHAPE when
 * too small).  Outputs equal vq_gemm_i8(..., w_bits 8, VQ_EPI_NONE). */
int vq_gemm_i8_stamped(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R,
                       const void* wq, const float* sw, const int32_t* zw, const int32_t* cs,
                       const float* bias, void* out, int ldo, int M, int N, int K, int Kp,
                       void* stamps, long n_stamps, void* stream);

/* Batched form of vq_gemm_i8 for ONE activation and nbatch stacked weight sets:
 *   out[b] [M, N] fp16 = dequant(xq . wq[b]^T) + bias[b],   b = 0 .. nbatch-1
 * wq [nbatch, N, Kp] int8, sw / zw / cs / bias [nbatch, N], out [nbatch, M, N] contiguous.  Used for the kv_linear of
 * all transformer blocks: MultiHeadCrossAttention.kv_linear (t2v/opensora/models/layers/blocks.py:297) is applied by
 * every block to the same prompt tokens, so one launch of nbatch x ceil(N/288) workgroups replaces nbatch launches
 * of ceil(N/288) workgroups each.  8-bit weights, no fused epilogue. */
int vq_gemm_i8_batched(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R, const void* wq,
                       const float* sw, const int32_t* zw, const int32_t* cs, const float* bias, void* out,
                       int nbatch, int M, int N, int K, int Kp, int w_bits, void* stream);

/* ngroups (1..3) independent Linears of ONE shape in one grid: out_g [M, N] = dequant(xq_g . wq_g^T) + bias_g at
 * out + g * N, row pitch ldo >= ngroups * N (the q | k | v column blocks of one buffer).  For the plans that balance
 * q / k / v each against its own weight (quant_layer.py:136-160: three smoothing vectors, hence three quantized copies
 * of the shared input, stdit_quant_layer.py:96,187,304 applied per layer): what the reference runs as three F.linear
 * calls.  Arrays are HOST arrays of device pointers; bias nullable (and each entry nullable).  No fused epilogue. */
int vq_gemm_i8_grouped(int ngroups, const int8_t* const* xq, const float* const* sx, const int32_t* const* zx,
                       const int32_t* const* R, const void* const* wq, const float* const* sw,
                       const int32_t* const* zw, const int32_t* const* cs, const float* const* bias, void* out,
                       int ldo, int M, int N, int K, int Kp, int w_bits, void* stream);

/* mlp.fc1 with GELU(tanh) AND the STATIC (calibrated, tensor-wise) activation quantizer of mlp.fc2 in the GEMM's epilogue:
 * replaces F.linear(x_hat, W_hat, bias) (qdiff/models/quant_layer.py:211) + nn.GELU(approximate="tanh")
 * (t2v/opensora/models/layers/blocks.py:27; modules.py:57) + ActQuantizer.forward after init_done
 * (qdiff/quantizer/base_quantizer.py:129-144) behind the smooth-quant division of the consuming Linear
 * (quant_layer.py:136-140).  The fp16 activation [M, N] is never written: every output element is rounded to fp16 as
 * vq_gemm_i8(VQ_EPI_GELU) would store it and quantized where it sits.
 * xq .. bias, M, N, K, Kp, w_bits, variant: as vq_gemm_i8 (8-bit weight storage only: 4 < w_bits <= 8).
 * s / s_rcp: both null, or the consuming Linear's smooth-quant channel scale per OUTPUT column [N] and its reciprocal from
 *   vq_smooth_reciprocal (the division exists in reciprocal form only here; s_rcp without s is ignored).
 * delta, zp: ONE fp32 value each in device memory, read by the kernel (no host synchronisation: graph-capturable); zp
 *   integer-valued, delta > 0.  n_bits 2..8.  No status word (no eps fill on a calibrated grid).
 * Contract: xq_out [M, Kp_out] (codes - 128 at 8 bits, raw codes below; pad columns [N, Kp_out) zero), sx_out[r] = delta,
 *   zx_out[r] = (int)zp - cx and R_out[r] = sum(raw codes) - N * (int)zp are bit-identical to
 *   vq_rowquant(..., s, s_rcp, delta_in = delta, zp_in = zp, n_param = 1) of the fp16 matrix vq_gemm_i8(..., VQ_EPI_GELU,
 *   variant) writes, for every variant.  R_out is zeroed by this call on `stream` before the launch (a small kernel; every
 *   wave adds its columns' part of a row's term with one relaxed integer atomic per row): callers do not pre-zero, and
 *   R_out is bit-reproducible.
 * variant: VQ_GEMM_DEFAULT, 11, 16 or 19 with the meaning (and 19's conditions: M % 256 == 0, N % 288 == 0) of vq_gemm_i8.
 * Errors, all before any HIP call or dereference, null pointers first: VQ_EINVAL for a null required pointer (all but
 *   bias, s, s_rcp) or a non-positive extent; VQ_ESHAPE for what vq_gemm_i8 refuses (Kp % 128, Kp < K, K > 16384, an
 *   operand image of 2^32 bytes or more), N % 8, Kp_out % 128, Kp_out < N, xq_out / s / s_rcp off 16 bytes, variant 19's
 *   conditions; VQ_EUNSUP for w_bits <= 4 or > 8, n_bits outside 2..8, s without s_rcp, an unknown variant. */
int vq_gemm_i8_rowquant_static(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R,
                               const void* wq, const float* sw, const int32_t* zw, const int32_t* cs,
                               const float* bias, const float* s, const float* s_rcp,
                               const float* delta, const float* zp,
                               int8_t* xq_out, float* sx_out, int32_t* zx_out, int32_t* R_out,
                               int M, int N, int K, int Kp, int Kp_out, int w_bits, int n_bits,
                               int variant, void* stream);

/* cross_attn.q_linear AND cross attention against the prompt's keys in ONE launch: the GEMM's 256 x 288 tile is 256 queries
 * x 4 heads of 72, the keys are <= 128 prompt tokens, so a workgroup holds everything its (query, head) pairs need and the
 * attention runs in the GEMM's epilogue.  Replaces F.linear(x_hat, W_hat, bias) (qdiff/models/quant_layer.py:211) +
 * xformers memory_efficient_attention with a block-diagonal mask (opensora/models/layers/blocks.py:302-304).  q [M, N] is
 * never written.
 * xq .. bias, M, N, K, Kp, w_bits: as vq_gemm_i8 (VQ_EPI_NONE; 8-bit and nibble weight storage).
 * k, v, o, n_seq, Lq, Lk, H, D, kv_*_stride, o_*_stride, kv_off, scale: as vq_attn_fwd, q being the GEMM's output: row
 *   i * Lq + t of the GEMM is token t of sequence i, its columns h * D .. h * D + D - 1 head h.
 * Contract: o is bit-identical to vq_gemm_i8(..., VQ_EPI_NONE, VQ_GEMM_DEFAULT) into a dense [M, N] buffer followed by
 *   vq_attn_fwd on it.
 * Shapes (VQ_ESHAPE otherwise, nothing launched): M % 256 == 0, N == H * D with N % 288 == 0, M == n_seq * Lq with
 *   Lq % 256 == 0 (every 256-row tile inside one sequence), Kp % 128 == 0, Kp >= K, K <= 16384, operand images below
 *   2^32 bytes, 0 < Lk <= 128 (with kv_off: the caller's bound on every sequence's key count), Lk * kv_tok_stride below
 *   2^30, strides multiples of 8 with kv_tok_stride >= D and o_tok_stride >= N, xq, wq, k, v, o 16-byte aligned.
 *   VQ_EUNSUP: D != 72, w_bits outside 2..8.  VQ_EINVAL: a null required pointer (all but bias, kv_off), a non-positive
 *   extent.  All checks come before any HIP call or dereference. */
int vq_gemm_i8_cross_attn(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R, const void* wq,
                          const float* sw, const int32_t* zw, const int32_t* cs, const float* bias,
                          const void* k, const void* v, void* o,
                          int M, int N, int K, int Kp, int w_bits, int n_seq, int Lq, int Lk, int H, int D,
                          long kv_seq_stride, long kv_tok_stride, long o_seq_stride, long o_tok_stride,
                          const int32_t* kv_off, float scale, void* stream);

/* ---- fp16 attention (fp32 online softmax) -----------------------------------
 * Replaces flash_attn_func / the softmax branch of Attention.forward
 * (opensora/models/layers/blocks.py:169-187), xformers block-diagonal
 * memory_efficient_attention (blocks.py:302-304) and PixArt self-attention
 * (t2i/diffusion/model/nets/PixArt_blocks.py:151-155).
 * Element (sequence i, token t, head h, dim d) of q is at
 *   q + i*q_seq_stride + t*q_tok_stride + h*D + d      (strides in elements,
 * multiples of 8); k, v use kv_*_stride, o uses o_*_stride.  With kv_off
 * (device int32 [n_seq+1], nullable) sequence i attends to kv rows
 * [kv_off[i], kv_off[i+1]) at kv_tok_stride (block-diagonal / varlen cross
 * attention), kv_seq_stride is ignored and Lk is an upper bound on every sequence's
 * kv length if the caller knows one (0 = unknown): D = 72 with a bound <= 128 (the
 * <= 120 prompt tokens of STDiT) runs a kernel that keeps K and V^T of a head in
 * registers.  D in {16, 32, 64, 72}.  q, k, v and o are 16-byte aligned (VQ_ESHAPE
 * otherwise): the kernels move 16 bytes per access.
 */
int vq_attn_fwd(const void* q, const void* k, const void* v, void* o,
                int n_seq, int Lq, int Lk, int H, int D,
                long q_seq_stride, long q_tok_stride, long kv_seq_stride, long kv_tok_stride,
                long o_seq_stride, long o_tok_stride, const int32_t* kv_off,
                float scale, void* stream);

/* Kernels behind vq_attn_fwd (ids returned by vq_attn_fwd_route). */
#define VQ_ATTN_K_FWD 0         /* attn_fwd_kernel: the general kernel (kv_off with an unknown bound, short queries)   */
#define VQ_ATTN_K_FWD8_NW4 1    /* attn_fwd8_kernel, 4 waves: no kv_off, Lk > 128, 96 <= Lq < 192                      */
#define VQ_ATTN_K_FWD8_NW8 2    /* attn_fwd8_kernel, 8 waves: Lq >= 192 with a K / V byte extent of 2^31 or more       */
#define VQ_ATTN_K_FWD32D 3      /* attn_fwd32d_kernel: no kv_off, Lk > 128, Lq >= 192                                  */
/* (value 4 is retired, never reused: the four-wave arm of attn_fwd32d_kernel, a lab kernel in tools/lab/attn_lab.hip) */
#define VQ_ATTN_K_FWD64D 5      /* attn_fwd64d_kernel: Lq >= 2048 and Lk >= 2048                                       */
#define VQ_ATTN_K_CROSS32_2 6   /* attn_cross32_kernel, 2 tile images: known Lk <= 128, Lq >= 256                      */
#define VQ_ATTN_K_CROSS32_3 7   /* attn_cross32_kernel, 3 / 4 / 5 tile images: kv_off, Lk bound 129-192 / 193-256 /    */
#define VQ_ATTN_K_CROSS32_4 8   /*   257-320, Lq >= 256, D >= 64                                                       */
#define VQ_ATTN_K_CROSS32_5 9
#define VQ_ATTN_K_CROSS_REG 10  /* attn_cross_reg_kernel: D = 72, known Lk <= 128, H % 8 == 0, 64 <= Lq < 256          */

/* Test hook: the VQ_ATTN_K_* kernel vq_attn_fwd would launch for exactly these arguments (same checks, same
 * negative code on a bad argument).  Launches nothing and makes no HIP call; pointers are not dereferenced. */
int vq_attn_fwd_route(const void* q, const void* k, const void* v, void* o,
                      int n_seq, int Lq, int Lk, int H, int D,
                      long q_seq_stride, long q_tok_stride, long kv_seq_stride, long kv_tok_stride,
                      long o_seq_stride, long o_tok_stride, const int32_t* kv_off,
                      float scale, void* stream);

/* Temporal attention of STDiTBlock (stdit.py:112-118): rows are laid out
 * [B][T][S] (row = (b*T + t)*S + s, row strides ld_in / ld_out elements) and
 * attention runs over t for every (b, s, head).  T <= 16.  q, k, v and o are
 * 16-byte aligned (VQ_ESHAPE otherwise). */
int vq_attn_temporal(const void* q, const void* k, const void* v, void* o,
                     int B, int T, int S, int H, int D, long ld_in, long ld_out,
                     float scale, void* stream);

/* Temporal attention fused with the per-token 8-bit dynamic quantizer of the Linear that consumes its output
 * (attn_temp.proj: stdit.py:116 -> QuantTemporalAttnLinear.forward, stdit_quant_layer.py:161-166 ->
 * DynamicActQuantizer, dynamic_quantizer.py:16-45) for B == 1 per forward: the fp16 attention output is
 * rounded as vq_attn_temporal would store it but never written; outputs are what vq_rowquant(n_bits = 8, s, s_rcp)
 * would produce from it (xq [B*T*S, Kp] codes - 128 with zeroed pad columns, sx, zx, R; status as there).
 * s / s_rcp: both null, or the consuming Linear's smooth-quant channel scale [H*D] and its reciprocal from
 * vq_smooth_reciprocal (the division x / s of quant_layer.py:140 exists in reciprocal form only in this kernel).
 * o: nullable, dense [B*T*S, H*D] fp16 copy of the attention output for callers that need both.
 * H <= 16, T <= 16, H*D % 16 == 0, Kp % 128 == 0.  q, k, v, xq and, when set, s, s_rcp and o are 16-byte
 * aligned (VQ_ESHAPE otherwise).  With B > 1 its grids are per row; grids shared by the samples of a joint forward are
 * vq_attn_temporal_rowquant_shared. */
int vq_attn_temporal_rowquant(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                              int8_t* xq, float* sx, int32_t* zx, int32_t* R, int32_t* status, void* o, int B, int T,
                              int S, int H, int D, long ld_in, int Kp, float scale, void* stream);

/* Temporal attention fused with the per-token dynamic quantizer of attn_temp.proj for a JOINT cond | uncond forward, at
 * 2..8 bits (stdit.py:112-118 -> QuantTemporalAttnLinear.forward, stdit_quant_layer.py:161-166 -> DynamicActQuantizer,
 * dynamic_quantizer.py:16-45; the joint forward over cat([x, x]) of iddpm/__init__.py:141-163): a token's grid is shared by
 * the rows of all B samples (base_quantizer.py:177-189: [B, n, C] -> [n, B*C]).  B is 1 or 2, T <= 16: the shared-grid
 * forms of the two kernels behind vq_attn_temporal_rowquant, one workgroup per spatial position of every sample.
 * Rows are r = (b*T + t)*S + s.  Contract: xq [B*T*S, Kp] (codes - 128 at 8 bits, raw codes below; pad columns
 * [H*D, Kp) zero), sx, zx (one grid per token, replicated per row), R (per row) and the VQ_ST_EPSFILL bit of status are
 * bit-identical to vq_rowquant(x = o viewed [B, T*S, H*D], s, s_rcp, n_bits) of the kernel's own fp16 output o, and o of
 * sample b is what vq_attn_temporal_rowquant writes for that sample alone.
 * s / s_rcp: both null, or proj's smooth-quant channel scale [H*D] and its reciprocal from vq_smooth_reciprocal.
 * o: nullable, dense [B*T*S, H*D] fp16 copy of the attention output.  status: nullable.
 * VQ_EINVAL: a null q / k / v / xq / sx / zx / R, s without s_rcp or the reverse, a non-positive B, T, S, H, D or Kp.
 * VQ_ESHAPE: T > 16, H > 16, ld_in % 8 != 0, H*D % 16 != 0, Kp % 128 != 0, Kp < H*D, 16 * (H*D / 8) > 192 * H (the V
 * staging registers), q / k / v / xq / s / s_rcp / o not 16-byte aligned, D outside {16, 32, 64, 72}, B > 2.
 * VQ_EUNSUP: n_bits outside 2..8.  In this order, all before any HIP call or dereference. */
int vq_attn_temporal_rowquant_shared(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                                     int8_t* xq, float* sx, int32_t* zx, int32_t* R, int32_t* status, void* o,
                                     int B, int T, int S, int H, int D, long ld_in, int Kp, int n_bits,
                                     float scale, void* stream);

/* Temporal attention for up to 64 frames (OpenSORA 64x512x512; STDiTBlock's temporal branch, stdit.py:112-118), with
 * the per-token 8-bit dynamic quantizer of attn_temp.proj (QuantTemporalAttnLinear.forward, stdit_quant_layer.py:161-166)
 * optionally fused.  Rows [B][T][S] as in vq_attn_temporal; 1 <= T <= 64, H <= 16 (one workgroup per spatial position
 * and all heads), D in {16, 32, 64, 72}, H*D % 16 == 0, q / k / v 16-byte aligned, ld_in % 8 == 0.
 * o: nullable fp16 output [B*T*S] rows of stride ld_out (% 8 == 0), rounded as vq_attn_temporal stores it.
 * xq: nullable; when set, sx, zx and R are required, B == 1 (per-token grids are shared over the batch) and
 * Kp % 128 == 0, and xq / sx / zx / R / status are what vq_rowquant(n_bits = 8, s, s_rcp) produces from the fp16
 * output (see vq_attn_temporal_rowquant).  At least one of o and xq.  s / s_rcp: both null or both set, 16-byte
 * aligned. */
int vq_attn_temporal_long(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                          int8_t* xq, float* sx, int32_t* zx, int32_t* R, int32_t* status, void* o, int B, int T,
                          int S, int H, int D, long ld_in, long ld_out, int Kp, float scale, void* stream);

/* Temporal attention fused with the STATIC (calibrated, tensor-wise) quantizer of attn_temp.proj (stdit.py:112-118 ->
 * QuantTemporalAttnLinear.forward, stdit_quant_layer.py:161-166 -> ActQuantizer.forward after init_done,
 * base_quantizer.py:129-144): the static-grid forms of the kernels behind vq_attn_temporal_rowquant (T <= 16, same
 * trimmed / generic choice) and vq_attn_temporal_long (17 <= T <= 64).  delta, zp: ONE fp32 value each in device
 * memory, read by the kernel (no host synchronisation: graph-capturable); zp integer-valued.  n_bits 2..8.  Any B >= 1
 * (a static grid is not shared over the batch) and no status word (no eps fill on a calibrated grid).
 * Contract: xq [B*T*S, Kp] (codes - 128 at 8 bits, raw codes below; pad columns [H*D, Kp) zero), sx = delta,
 * zx = (int)zp - cx and R = sum(xq) - H*D*zx are bit-identical to vq_rowquant(..., s, s_rcp, delta_in = delta,
 * zp_in = zp, n_param = 1) of the kernel's own fp16 attention output.
 * s / s_rcp: both null, or proj's smooth-quant channel scale [H*D] and its reciprocal from vq_smooth_reciprocal.
 * o: nullable fp16 copy of the attention output, dense for T <= 16 (ld_out == H*D), rows of stride ld_out
 * (% 8 == 0, >= H*D) for T > 16.
 * VQ_EINVAL: a null required pointer (q, k, v, delta, zp, xq, sx, zx, R; s without s_rcp or the reverse), a non-positive
 * extent, T outside 1..64.  VQ_ESHAPE: H > 16, H*D % 16 != 0, D outside {16, 32, 64, 72}, Kp % 128 != 0, Kp < H*D,
 * ld_in % 8 != 0, the rules of o above, q / k / v / xq / s / s_rcp / o not 16-byte aligned, B > 65535, and for T > 16 a
 * position whose rows span 2^31 bytes or more.  VQ_EUNSUP: n_bits outside 2..8.  All before any HIP call or dereference. */
int vq_attn_temporal_rowquant_static(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                                     const float* delta, const float* zp, int8_t* xq, float* sx, int32_t* zx, int32_t* R,
                                     void* o, int B, int T, int S, int H, int D, long ld_in, long ld_out, int Kp,
                                     int n_bits, float scale, void* stream);

/* Spatial / cross / image attention (vq_attn_fwd) fused with the STATIC (calibrated, tensor-wise) quantizer of the Linear
 * that consumes its output - attn.proj and cross_attn.proj of STDiTBlock (opensora/models/layers/blocks.py:151-195,292-310;
 * stdit.py:104-109,121), PixArt's self-attention proj (PixArt_blocks.py:151-155) -> ActQuantizer.forward after init_done
 * (base_quantizer.py:129-144) behind the smooth-quant division of quant_layer.py:136-140.  The arguments are those of
 * vq_attn_fwd plus the quantizer's; the kernel is the static-grid form of the one vq_attn_fwd_route names for the same
 * arguments: attn_fwd_kernel, attn_fwd32d_kernel, attn_fwd64d_kernel, attn_cross32_kernel (VQ_ATTN_K_FWD, FWD32D, FWD64D,
 * CROSS32_2..5).  The quantizer is one more epilogue step of that kernel: attention arithmetic and fp16 rounding are its own.
 * delta, zp: ONE fp32 value each in device memory, read by the kernel (no host synchronisation: graph-capturable); zp
 * integer-valued.  n_bits 2..8.  No status word (no eps fill on a calibrated grid).  Quantized rows are dense:
 * row = sequence * Lq + query.  R is zeroed by this call on `stream` before the launch (a small kernel; every head adds
 * its part of a row's term with an integer atomic): callers do not pre-zero, and R is bit-reproducible.
 * Contract: o, when set, is bit-identical to vq_attn_fwd with the same arguments; xq [n_seq*Lq, Kp] (codes - 128 at 8
 * bits, raw codes below; pad columns [H*D, Kp) zero), sx = delta, zx = (int)zp - cx and R = sum(xq) - H*D*zx are
 * bit-identical to vq_rowquant(..., s, s_rcp, delta_in = delta, zp_in = zp, n_param = 1) of that output.
 * s / s_rcp: both null, or the consuming Linear's smooth-quant channel scale [H*D] and its reciprocal from
 * vq_smooth_reciprocal (the division exists in reciprocal form only here).  o: nullable.
 * VQ_EINVAL: a null required pointer (q, k, v, delta, zp, xq, sx, zx, R); s without s_rcp or the reverse; a non-positive
 * extent (n_seq, Lq, H, D, Kp; Lk without kv_off).  VQ_ESHAPE: the rules of vq_attn_fwd (strides % 8, q / k / v / o 16-byte
 * aligned, n_seq, H <= 65535); Kp % 128 != 0, Kp < H*D, D % 4 != 0; xq / s / s_rcp not 16-byte aligned; n_seq*Lq beyond
 * int32.  VQ_EUNSUP: n_bits outside 2..8; D outside {16, 32, 64, 72}; a route without a static-grid form
 * (VQ_ATTN_K_FWD8_NW4, VQ_ATTN_K_FWD8_NW8, VQ_ATTN_K_CROSS_REG): the caller keeps vq_attn_fwd + vq_rowquant.  All before
 * any HIP call or dereference. */
int vq_attn_fwd_rowquant_static(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                                const float* delta, const float* zp, int8_t* xq, float* sx, int32_t* zx, int32_t* R,
                                void* o, int n_seq, int Lq, int Lk, int H, int D,
                                long q_seq_stride, long q_tok_stride, long kv_seq_stride, long kv_tok_stride,
                                long o_seq_stride, long o_tok_stride, const int32_t* kv_off,
                                int Kp, int n_bits, float scale, void* stream);

/* ---- small fused elementwise helpers ---------------------------------------
 * mod[j, b, c] = table[j, c] + t0[b, j*C + c]  (stdit.py:100-102), fp32 out, chunk-major. */
int vq_adaln_table(const void* table, const void* t0, float* mod, int B, int J, int C, void* stream);

/* Fused CFG + DDIM(eta=0) update of the kept half of the batch: replaces the tail of
 * forward_with_cfg (t2v/opensora/schedulers/iddpm/__init__.py:168-184; PTQD division by
 * 1+k, guidance on eps[:, :3] only) and p_mean_variance + ddim_sample
 * (iddpm/gaussian_diffusion.py:252-335,514-552).  cond/uncond fp32 [n,2C,inner] model
 * outputs, x / x_out fp32 [n,C,inner]; A = sqrt_recip_alphas_cumprod[t],
 * Bc = sqrt_recipm1_alphas_cumprod[t], abar_prev = alphas_cumprod_prev[t]. */
int vq_cfg_ddim_step(const float* cond, const float* uncond, const float* x, float* x_out,
                     int n, int C, int inner, float cfg, float one_plus_k,
                     float A, float Bc, float abar_prev, void* stream);

/* Fused CFG + data-prediction DPM-Solver++ multistep update: ONE launch per model call of the PixArt sampling loop.
 * Replaces model_wrapper's guidance (t2i/diffusion/model/dpm_solver_sigma.py:318-332: noise_uncond + scale * (noise -
 * noise_uncond)), data_prediction_fn (:435-444: x0 = (x - sigma_t * noise) / alpha_t) and the update that follows the
 * call: dpm_solver_first_update (:551-596), multistep_dpm_solver_second_update (:805-862, solver_type 'dpmsolver' and
 * 'taylor') or multistep_dpm_solver_third_update (:864-915), algorithm_type 'dpmsolver++'.
 * For call number k (0-based) = clamp(row + (step ? *step : 0), 0, n_rows - 1), per element of [n, C, inner]:
 *   u = eps[b], c = eps[n + b]       eps: the model's output for the (uncond | cond) batch, [2n] x [C*inner], batch pitch
 *                                    ld_eps elements (2*C*inner for the chunk(2, dim=1)[0] view of forward_with_dpmsolver:
 *                                    the learned-sigma channels are never read); fp32 (eps_f16 = 0) or fp16 (1)
 *   e   = u + cfg * (c - u)
 *   m_k = (x - sigma_t * e) * inv_alpha_t            -> hist[k % 3]         hist: [3, n*C*inner] fp32
 *   order 1: x_out = a*x - b*m_k
 *   order 2: D1_0 = inv_r0 * (m_k - m_{k-1});  x_out = a*x - b*m_k - c1*D1_0 ('dpmsolver') / + c1*D1_0 ('taylor')
 *   order 3: D1_0 as above, D1_1 = inv_r1 * (m_{k-1} - m_{k-2}), dd = D1_0 - D1_1, D1 = D1_0 + r0_frac * dd,
 *            D2 = inv_r01 * dd;  x_out = a*x - b*m_k + c1*D1 - c2*D2
 *   with m_{k-1} = hist[(k - 1) % 3], m_{k-2} = hist[(k - 2) % 3], each expression evaluated left to right.
 * x_out fp32 [n, C, inner], may alias x.  x_model: NULL, or the next forward's input [2n, C, inner] in fp32 (xm_f16 = 0) or
 * fp16 (1): both halves receive x_out (torch.cat([x, x]) and the model's cast).
 * Coefficient row (VQ_DPMPP_ROW floats, device memory, n_rows rows): the indices below.  step: NULL (an eager launch of
 * row `row`) or a device counter: the same captured launch then serves every timestep (vq_dpmpp_advance moves it).
 * Numerics: bit-identical to the eager torch expressions on the same device.  Every operation is one fp32 rounding and
 * nothing is contracted into an fma; with fp16 eps, c - u, cfg * (.), u + (.) and sigma_t * e are each rounded to fp16 (the
 * eager path's fp16 tensors).  The division by alpha_t is the product with VQ_DPMPP_INV_ALPHA = RN_fp32(1 / alpha_t): torch
 * divides a GPU tensor by a host scalar that way (on the CPU it divides; VQ_DPMPP_ALPHA is kept in the row for that form).
 * VQ_EINVAL: a null eps / x / hist / coef / x_out, n / C / inner / n_rows <= 0, row outside [0, n_rows).  Then VQ_ESHAPE:
 * ld_eps < C*inner; the kernel moves 4 elements per access when inner % 4 == 0 (else 1): ld_eps not a multiple of that, or
 * eps / x / hist / x_out / x_model not aligned to that many elements; coef / step off 4 bytes.  Then VQ_EUNSUP: eps_f16 or
 * xm_f16 outside {0, 1}.  All before any HIP call or dereference. */
#define VQ_DPMPP_ROW 16        /* floats per row */
#define VQ_DPMPP_ORDER 0       /* 1, 2 or 3 */
#define VQ_DPMPP_TAYLOR 1      /* 0 'dpmsolver', 1 'taylor' (order 2) */
#define VQ_DPMPP_CFG 2         /* guidance scale */
#define VQ_DPMPP_SIGMA 3       /* sigma_t of this call's time (data_prediction_fn) */
#define VQ_DPMPP_ALPHA 4       /* alpha_t of this call's time (not read by the kernel) */
#define VQ_DPMPP_INV_ALPHA 5   /* RN_fp32(1 / alpha_t) */
#define VQ_DPMPP_X 6           /* a  = sigma_next / sigma_t */
#define VQ_DPMPP_M0 7          /* b  = alpha_next * phi_1 */
#define VQ_DPMPP_D1 8          /* c1 = 0.5 * (alpha_next * phi_1) | alpha_next * (phi_1 / h + 1) | alpha_next * phi_2 */
#define VQ_DPMPP_D2 9          /* c2 = alpha_next * phi_3 */
#define VQ_DPMPP_INV_R0 10     /* 1 / r0 */
#define VQ_DPMPP_INV_R1 11     /* 1 / r1 */
#define VQ_DPMPP_R0_FRAC 12    /* r0 / (r0 + r1) */
#define VQ_DPMPP_INV_R01 13    /* 1 / (r0 + r1) */
#define VQ_DPMPP_T_NEXT 14     /* model-input time of the NEXT forward: (t_next - 1/N) * 1000 */
                               /* 15: zero */
int vq_cfg_dpmpp_step(const void* eps, const float* x, float* hist, const float* coef, const int32_t* step,
                      float* x_out, void* x_model, int n, int C, int inner, long ld_eps, int row, int n_rows,
                      int eps_f16, int xm_f16, void* stream);

/* The same step for the STDiT sampling loop (t2v/opensora/schedulers/dpms/__init__.py: DMP_SOLVER.sample,
 * forward_with_dpmsolver), reading the model output where final_layer left it instead of an unpatchified fp32 copy.
 *   eps_u, eps_c: the uncond and the cond output, each [n, N_t*N_h*N_w, p_t*p_h*p_w*C_out] with N_t = T/p_t, N_h = H/p_h,
 *                 N_w = W/p_w, sample pitch ld_eps elements, fp32 (eps_f16 = 0) or fp16 (1).  Two pointers: the two
 *                 forwards of a cfg_split step write two buffers; a joint forward passes eps_c = eps_u + n*ld_eps.
 *   latent element (b, c, t, h, w), c < C, is read from token ((t/p_t)*N_h + h/p_h)*N_w + w/p_w at column
 *                 (((t%p_t)*p_h + h%p_h)*p_w + w%p_w)*C_out + c: the index map of STDiT.unpatchify.  Channels C .. C_out-1
 *                 (the learned sigma that chunk(2, dim=1)[0] drops) are never read.
 * Every value is widened to fp32 on load and ALL arithmetic is fp32, one rounding per operation, nothing contracted: what
 * unpatchify, .to(float32) and the eager expressions compute (the fp16-typed guidance of vq_cfg_dpmpp_step is the PixArt
 * loop's).  The formulas, hist (3 slots), the VQ_DPMPP_* row, row / n_rows / step are those of vq_cfg_dpmpp_step; x, hist
 * slots and x_out are dense fp32 [n, C, T, H, W], x_out may alias x.  x_model: NULL, or [xm_copies, n, C, T, H, W] in fp32
 * (xm_f16 = 0) or fp16 (1): xm_copies = 1 for the cfg_split forwards (both read the same n samples), 2 for a joint one.
 * Access: C == 4, C_out % 4 == 0 and W % 2 == 0 read 4 channels per eps access and move 2 elements along w per fp32 /
 * x_model access; every other shape moves one element per access.
 * VQ_EINVAL: a null eps_u / eps_c / x / hist / coef / x_out, an extent, a patch extent or n_rows <= 0, row outside
 * [0, n_rows).  Then VQ_ESHAPE: C > C_out, T % p_t, H % p_h or W % p_w != 0, ld_eps < T*H*W*C_out; ld_eps not a multiple of
 * the channels per eps access, eps_u / eps_c not aligned to that many elements, x / hist / x_out / x_model not aligned to
 * the elements per access along w; coef / step off 4 bytes.  Then VQ_EUNSUP: a patch extent outside {1, 2}, eps_f16 or
 * xm_f16 outside {0, 1}, xm_copies outside {1, 2}.  All before any HIP call or dereference. */
int vq_cfg_dpmpp_step_patch(const void* eps_u, const void* eps_c, const float* x, float* hist, const float* coef,
                            const int32_t* step, float* x_out, void* x_model, int n, int C, int C_out, int T, int H, int W,
                            int p_t, int p_h, int p_w, long ld_eps, int row, int n_rows, int eps_f16, int xm_f16,
                            int xm_copies, void* stream);

/* One workgroup, enqueued after vq_cfg_dpmpp_step: t_out[0 .. n_t) (fp32) = VQ_DPMPP_T_NEXT of row clamp(*step, 0,
 * n_rows - 1), then *step = min(*step + 1, n_rows - 1).  A launch of its own, so that no workgroup of the step kernel can
 * read a counter another one has already moved.  VQ_EINVAL: a null pointer, n_rows or n_t <= 0; VQ_ESHAPE: a pointer off
 * 4 bytes. */
int vq_dpmpp_advance(int32_t* step, const float* coef, int n_rows, float* t_out, int n_t, void* stream);

/* The DDIM(eta = 0) step of vq_cfg_ddim_step for the STDiT loop in the table-driven, patch-major form: it reads the model
 * output where final_layer left it (no unpatchify copy, no fp32 cast) and its five scalars from a coefficient row.
 *   eps_c, eps_u: the cond and the uncond output, each [n, N_t*N_h*N_w, p_t*p_h*p_w*C_out], sample pitch ld_eps elements,
 *                 fp32 (eps_f16 = 0) or fp16 (1).  Two pointers: the two forwards of a cfg_split step write two buffers; a
 *                 joint forward of this loop (text = cat([cond, null])) passes eps_u = eps_c + n*ld_eps.
 *   The index map, patch extents, x_model / xm_copies, the access widths and their choice, and the grid are those of
 *   vq_cfg_dpmpp_step_patch.  Channels C .. C_out-1 (the learned sigma, unused at eta = 0) and the pitch padding are never read.
 * For row k = clamp(row + (step ? *step : 0), 0, n_rows - 1), per latent element (b, c, t, h, w), every value widened to
 * fp32 on load, with fl() one fp32 rounding and fma() one rounding of the exact a*b + c:
 *   cv = fl(cond / (1 + k)),  uv = fl(uncond / (1 + k))                         (IEEE division)
 *   e  = c < guided ? fma(cfg, fl(cv - uv), uv) : cv                            (guided > C behaves as C)
 *   be = fl(Bc * e);   x0 = fma(A, x, -be)
 *   r  = fl(fl(A * x) - x0)               [paired: fma(A, x, -x0)]
 *   e2 = fl(r / Bc)                                                             (IEEE division)
 *   sa = sqrt(abar_prev),  sb = sqrt(fl(1 - abar_prev))                          (__fsqrt_rn)
 *   x_next = fl(fl(sa * x0) + fl(sb * e2))  [paired: fma(sa, x0, fl(sb * e2))]
 * This is, operation for operation, what the compiled cfg_ddim_kernel of vq_cfg_ddim_step performs (that kernel leaves
 * contraction to the compiler; here every fma is written out and nothing else is contracted), so the result is bit for
 * bit vq_cfg_ddim_step applied to unpatchify(out).to(float32).  That kernel has TWO compiled bodies: its grid-stride loop
 * (4096 x 256 = 2^20 elements per pass) is unrolled by two, and the unrolled body contracts r and x_next (the bracketed
 * 'paired' forms) where the remainder body does not.  A latent of n*C*T*H*W <= 2^20 elements - a 16 x 64 x 64 one has
 * 2^18 per sample - is one pass, remainder body throughout.  Above that, the dense index i of an element decides: with
 * first = i mod 2^20 and passes = floor((total - 1 - first) / 2^20) + 1, the element is 'paired' iff
 * floor(i / 2^20) < passes - passes % 2.  This entry point evaluates the same rule per element (shifts, no division).
 * Coefficient row: VQ_DDIM_ROW floats, the indices below; unused slots are zero.  The row has the size of the DPM-Solver++
 * row and keeps the next model-input time in the same slot (VQ_DDIM_T_NEXT == VQ_DPMPP_T_NEXT), so vq_dpmpp_advance serves
 * as this step's counter kernel.  PTQD's 1 + k is per row.
 * x dense fp32 [n, C, T, H, W]; x_out the same, may alias x.
 * Refusals: those of vq_cfg_dpmpp_step_patch in its order (there is no hist), and guided < 0 is VQ_EINVAL.  All before any
 * HIP call or dereference. */
#define VQ_DDIM_ROW 16         /* floats per row (== VQ_DPMPP_ROW) */
#define VQ_DDIM_CFG 0          /* guidance scale */
#define VQ_DDIM_ONE_PLUS_K 1   /* 1 + k (PTQD), 1 without */
#define VQ_DDIM_A 2            /* sqrt_recip_alphas_cumprod[t] */
#define VQ_DDIM_BC 3           /* sqrt_recipm1_alphas_cumprod[t] */
#define VQ_DDIM_ABAR_PREV 4    /* alphas_cumprod_prev[t] */
#define VQ_DDIM_T_NEXT 14      /* model-input time of the NEXT forward */
int vq_cfg_ddim_step_patch(const void* eps_c, const void* eps_u, const float* x, const float* coef, const int32_t* step,
                           float* x_out, void* x_model, int n, int C, int C_out, int T, int H, int W, int p_t, int p_h,
                           int p_w, long ld_eps, int guided, int row, int n_rows, int eps_f16, int xm_f16, int xm_copies,
                           void* stream);

/* Fused CFG + learned-range variance + ancestral posterior step: ONE launch per model call of the PixArt IDDPM loop
 * (p_sample_loop(model.forward_with_cfg, ...), quant_txt2img.py:154-166).  Replaces, for the kept first half of the
 * duplicated batch, the tail of forward_with_cfg (t2i/diffusion/model/nets/PixArtMS.py:221-234), p_mean_variance
 * (t2i/diffusion/model/gaussian_diffusion.py:303-318), _predict_xstart_from_eps (:363-368), q_posterior_mean_variance
 * (:264-267) and p_sample (:439-445).  For row k = clamp(row + (step ? *step : 0), 0, n_rows - 1), per element of
 * [n, C, inner]:
 *   c = eps[b, ch], u = eps[n + b, ch]   eps: the model's output for the (cond | uncond) batch - the OPPOSITE order of
 *                                        vq_cfg_dpmpp_step -, [2n] x [2C * inner], batch pitch ld_eps elements; fp32
 *                                        (eps_f16 = 0) or fp16 (1)
 *   e    = ch < guided ? u + cfg * (c - u) : c          (guided = 3 in the reference)
 *   v    = eps[b, C + ch]                               cond's variance channel; uncond's channels >= guided and its
 *                                                       variance channels are never read
 *   frac = (v + 1) * 0.5
 *   lv   = frac * max_log + (1 - frac) * min_log
 *   x0   = A * x - B * e;  clamped into [-1, 1] when CLIP   -> x0_out (NULL or fp32 [n, C, inner]: 'pred_xstart')
 *   mean = c1 * x0 + c2 * x
 *   out  = mean + ((nonzero * exp(0.5 * lv)) * noise)   -> x_out fp32 [n, C, inner], may alias x
 * noise: fp32 [n, C, inner], required on every row (the reference draws it on the last one too, where nonzero = 0).
 * x_model: NULL, or the next forward's input [2n, C, inner] in fp32 (xm_f16 = 0) or fp16 (1): both halves receive out.
 * Coefficient row: VQ_DDPM_ROW floats, the indices below; unused slots are zero.  The row has the size of the DPM-Solver++
 * row and keeps the next model-input time in the same slot (VQ_DDPM_T_NEXT == VQ_DPMPP_T_NEXT), so vq_dpmpp_advance serves
 * as the counter and time kernel of this step unchanged.  step: as for vq_cfg_dpmpp_step.
 * Numerics: every operation is rounded on its own, nothing is contracted; with fp16 eps, c - u, cfg * (.), u + (.), v + 1,
 * (.) * 0.5 and 1 - frac are each rounded to fp16 (the eager path's fp16 tensors) and everything that meets a coefficient
 * is fp32; exp is expf.
 * Refusals, in this order, before any HIP call or dereference.  VQ_EINVAL: a null eps / x / noise / coef / x_out; n / C /
 * inner / n_rows <= 0; row outside [0, n_rows); guided < 0.  VQ_ESHAPE: ld_eps < 2*C*inner; guided > C; the kernel moves 4
 * elements per access when inner % 4 == 0 (else 1): ld_eps not a multiple of that, or eps / x / noise / x_out / x0_out /
 * x_model not aligned to that many elements; coef / step off 4 bytes.  VQ_EUNSUP: eps_f16 or xm_f16 outside {0, 1}. */
#define VQ_DDPM_ROW 16         /* floats per row (== VQ_DPMPP_ROW) */
#define VQ_DDPM_CFG 0          /* guidance scale */
#define VQ_DDPM_A 1            /* sqrt_recip_alphas_cumprod[i] */
#define VQ_DDPM_B 2            /* sqrt_recipm1_alphas_cumprod[i] */
#define VQ_DDPM_C1 3           /* posterior_mean_coef1[i] */
#define VQ_DDPM_C2 4           /* posterior_mean_coef2[i] */
#define VQ_DDPM_MIN_LOG 5      /* posterior_log_variance_clipped[i] */
#define VQ_DDPM_MAX_LOG 6      /* log(betas[i]) */
#define VQ_DDPM_NONZERO 7      /* 1, on the row of i == 0: 0 */
#define VQ_DDPM_CLIP 8         /* clip_denoised: 0 or 1 */
#define VQ_DDPM_T_NEXT 14      /* model-input time of the NEXT forward (== VQ_DPMPP_T_NEXT) */
                               /* 9 - 13, 15: zero */
int vq_cfg_ddpm_step(const void* eps, const float* x, const float* noise, const float* coef, const int32_t* step,
                     float* x_out, float* x0_out, void* x_model, int n, int C, int inner, long ld_eps, int guided,
                     int row, int n_rows, int eps_f16, int xm_f16, void* stream);

/* Fused CFG + x0 + SA-Solver corrector + next predictor: ONE launch per model call of the PixArt SA-Solver loop
 * (SASolverSampler.sample, t2i/diffusion/sa_sampler.py:75-92: 'few_steps', PEC, predictor 2, corrector 2).  Replaces
 * model_wrapper's guidance (t2i/diffusion/model/sa_solver.py:297-322), data_prediction_fn (:377-386), the corrector
 * adams_moulton_update_few_steps (:700-753) of loop step k and the predictor adams_bashforth_update_few_steps (:644-698) of
 * loop step k + 1 (sample_few_steps :755-909); the final, predictor-only step (tau = 0, order 1, no model call) is the
 * predictor half of the last call, so S launches serve S model calls and the last launch's xp_out is the result.
 * For call number k (0-based) = clamp(row + (step ? *step : 0), 0, n_rows - 1), per element of [n, C, inner]:
 *   u = eps[b], c = eps[n + b]           eps: the model's output for the (uncond | cond) batch, [2n] x [C*inner], batch
 *                                        pitch ld_eps elements; fp32 (eps_f16 = 0) or fp16 (1)
 *   e   = u + cfg * (c - u)
 *   m_k = (xp - sigma * e) / alpha                                          -> hist[k % 2]     hist: [2, n*C*inner] fp32
 *   OC == 0 (call 0):  xc = x
 *   OC >= 1:           g  = CG0 * m_k;  if OC == 2: g = g + CG1 * m_{k-1}
 *                      xc = (CX * x + g) + CN * noise[k % 2]                -> x_out
 *   OP >= 1:           q  = PG0 * m_k;  if OP == 2: q = q + PG1 * m_{k-1}
 *                      xq = (PX * xc + q) + PN * noise[(k + 1) % 2]         -> xp_out, x_model   (OP == 0: xq = xc)
 *   with m_{k-1} = hist[(k - 1) % 2], each expression evaluated left to right.
 * x: the corrected sample of the previous loop step, xp: the predicted sample the model just saw, both fp32 [n, C, inner];
 * x_out may alias x and xp_out may alias xp.  noise: fp32 [2, n*C*inner], a ring: slot (k + 1) % 2 holds the draw of loop
 * step k + 1, written by the host before call k.  m_{k-1} is read only when an order is 2, noise[k % 2] only when OC >= 1.
 * x_model: NULL, or the next forward's input [2n, C, inner] in fp32 (xm_f16 = 0) or fp16 (1): both halves receive xq.
 * Coefficient row: VQ_SA_ROW floats, the indices below; unused slots are zero.  The row has the size of the DPM-Solver++ row
 * and keeps the next model-input time in the same slot (VQ_SA_T_NEXT == VQ_DPMPP_T_NEXT), so vq_dpmpp_advance serves as
 * the counter and time kernel of this step unchanged - which is why the orders stop at 2 (the released configuration);
 * an order outside {0, 1, 2} in the table is the host's to avoid.  step: as for vq_cfg_dpmpp_step.
 * Numerics: bit-identical to the eager torch expressions on the same device and to an fp32 model that rounds every
 * operation on its own.  Nothing is contracted; with fp16 eps, c - u, cfg * (.) and u + (.) are each rounded to fp16,
 * sigma * e is an fp32 product (sigma_t is a one-element fp32 tensor in the eager path: it promotes) and the division by
 * alpha is the correctly rounded fp32 division.  No transcendental.
 * Refusals, in this order, before any HIP call or dereference.  VQ_EINVAL: a null eps / x / xp / hist / noise / coef /
 * x_out / xp_out; n / C / inner / n_rows <= 0; row outside [0, n_rows).  VQ_ESHAPE: ld_eps < C*inner; the kernel moves 4
 * elements per access when inner % 4 == 0 (else 1): ld_eps not a multiple of that, or eps / x / xp / hist / noise / x_out /
 * xp_out / x_model not aligned to that many elements; coef / step off 4 bytes.  VQ_EUNSUP: eps_f16 or xm_f16 outside
 * {0, 1}. */
#define VQ_SA_ROW 16           /* floats per row (== VQ_DPMPP_ROW) */
#define VQ_SA_CFG 0            /* guidance scale */
#define VQ_SA_SIGMA 1          /* sigma_t of this call's time (data_prediction_fn) */
#define VQ_SA_ALPHA 2          /* alpha_t of this call's time */
#define VQ_SA_OC 3             /* corrector order of loop step k: 0 (call 0: none), 1 or 2 */
#define VQ_SA_CX 4             /* exp(-tau^2 h) * (sigma_t / sigma_prev), step k-1 -> k */
#define VQ_SA_CG0 5            /* ((1 + tau^2) * sigma_t) * exp(-tau^2 lambda_t) * gc[0] */
#define VQ_SA_CG1 6            /* ... * gc[1] (OC == 2) */
#define VQ_SA_CN 7             /* sigma_t * sqrt(1 - exp(-2 tau^2 h)) */
#define VQ_SA_OP 8             /* predictor order of loop step k + 1: 1 or 2 */
#define VQ_SA_PX 9             /* as CX, for the step k -> k+1 with that step's tau (last row: tau = 0) */
#define VQ_SA_PG0 10           /* as CG0 */
#define VQ_SA_PG1 11           /* as CG1 (OP == 2) */
#define VQ_SA_PN 12            /* as CN */
#define VQ_SA_T_NEXT 14        /* model-input time of the NEXT forward (== VQ_DPMPP_T_NEXT) */
                               /* 13, 15: zero */
int vq_cfg_sa_step(const void* eps, const float* x, const float* xp, float* hist, const float* noise, const float* coef,
                   const int32_t* step, float* x_out, float* xp_out, void* x_model, int n, int C, int inner, long ld_eps,
                   int row, int n_rows, int eps_f16, int xm_f16, void* stream);

/* ---- floating-point Linears at the edges of a forward -------------------------------------
 * out[m, n] = act_out( sum_k act_in(x[m, k]) * w[n, k] + bias[n] ): fp16 operands and result, fp32 accumulation (MFMA),
 * act: 0 none, 1 SiLU, 2 GELU(tanh).  Replaces F.linear of the layers the reference's FP lists keep out of quantization
 * (t2v/remain_fp.txt; quant_txt2img.py:294): TimestepEmbedder.mlp = Linear, SiLU, Linear
 * (t2v/opensora/models/layers/blocks.py:405-460; act_out = 1 on the first), t_block = SiLU, Linear
 * (t2v/opensora/models/stdit/stdit.py:193-196; act_in = 1), CaptionEmbedder.y_proj = Linear, GELU(tanh), Linear
 * (blocks.py:511-548; act_out = 2 on the first), T2IFinalLayer.linear (blocks.py:393-397), and the patch embedding
 * PatchEmbed3D.proj, a Conv3d whose kernel equals its stride, as a [tokens, C_in pt ph pw] matmul (blocks.py:66-105).
 * x [M, K] row pitch ldx, w [N, K] row pitch ldw, bias [N] fp16 or NULL, out [M, N] row pitch ldo (elements).
 * K % 8 == 0, N % 4 == 0, pitches multiples of 8 / 8 / 4.  Supported (act_in, act_out): (0,0) (0,1) (0,2) (1,0). */
int vq_linear_f16(const void* x, const void* w, const void* bias, void* out, int M, int N, int K, long ldx, long ldw,
                  long ldo, int act_in, int act_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDITQ_H */

// attn_rowquant.h - what the temporal attention kernels with the fused per-token quantizer share
// (attn_temporal_quant_kernel, attn_temporal_quant2_kernel, attn_temporal_long_kernel of attention.hip).
//
// The layout all of them use: one wave per head, 16x16 MFMA tiles, lane = (query row tq = lane & 15, row group
// g4 = lane >> 4).  S^T = K Q^T leaves lane (tq, g4) with keys 16 kt + 4 g4 .. + 3 of query tq; O^T = V^T P^T leaves it
// with dims 16 dt + 4 g4 .. + 3 of token tq.  A token's quantizer needs its whole row (all heads): every wave reduces its
// head's part over its four 16-lane rows, the parts meet in LDS (ex_min / ex_max / ex_sum: [wave][16] each, between two
// s_waitcnt lgkmcnt(0) + s_barrier pairs), and every wave derives the same grid from them.  The contract: codes, scale,
// zero point and row sum are bit-identical to vq_rowquant of the kernel's own fp16 output (vq_row_grid / rq_round_group).
//
// Only the row reductions live here.  The softmax / x / s / min-max / encode / record steps are still written out in
// each kernel: behind __forceinline__ helpers hipcc selects other instructions and allocates other registers for the
// same arithmetic (the callee is simplified on its own before it is inlined), up to +12 VGPRs and +4 bytes of scratch -
// profiles/refactor_attn_isa.md has the figures per helper.  A fourth kernel of this kind should start from there.
//
// The static-grid forms (the three kernels instantiated on TempQSArgs; vq_attn_temporal_rowquant_static) quantize every row
// on ONE calibrated grid (delta, zp: one fp32 value each, read on the device) at a code width of 2..8 bits: no row
// min / max, hence no ex_min / ex_max exchange, no vq_row_grid, no eps fill and no status word; only the row sum still
// crosses the heads (ex_sum).  Their codes are rqs_grid / rqs_quant of rowquant_shared.h - rq_round_group's bound needs
// the row's own grid - and bit-identical to vq_rowquant(delta_in, zp_in, n_param = 1) of the kernel's own fp16 output.
// Everything the static arm adds sits in the helpers at the end of this file: the arm is an ``if constexpr`` of each
// kernel, so the dynamic instantiations compile to what they were (profiles/static_quant/attn_resources.md).
#pragma once
#include "vq_common.h"
#include "rowquant_shared.h"

// ---- reductions over the four 16-lane rows of a wave (all 64 lanes receive the result) -------------------------------
// (the swap builtins return a 2-vector: its elements are copied into scalars before any __builtin_bit_cast - written on the
//  vector elements directly, hipcc of ROCm 7.2 reads element 0 for both)
__device__ __forceinline__ float tq_xor16(float x, bool is_max) {     // combine rows (0,1) and (2,3) of the wave
    const unsigned b = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    const unsigned r0 = r[0], r1 = r[1];
    float m;      // (asm: fmaxf / fminf would canonicalise both operands first - two more instructions per reduction step)
    if (is_max) asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(r0), "v"(r1));
    else asm("v_min_f32 %0, %1, %2" : "=v"(m) : "v"(r0), "v"(r1));
    return m;
}
__device__ __forceinline__ float tq_xor32(float x, bool is_max) {     // combine the two halves of the wave
    const unsigned b = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    const unsigned r0 = r[0], r1 = r[1];
    float m;      // (asm: fmaxf / fminf would canonicalise both operands first - two more instructions per reduction step)
    if (is_max) asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(r0), "v"(r1));
    else asm("v_min_f32 %0, %1, %2" : "=v"(m) : "v"(r0), "v"(r1));
    return m;
}
__device__ __forceinline__ float tq_sum4rows(float x) {
    unsigned b = __builtin_bit_cast(unsigned, x);
    auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    unsigned r0 = r[0], r1 = r[1];
    x = __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
    b = __builtin_bit_cast(unsigned, x);
    r = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    r0 = r[0], r1 = r[1];
    return __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
}
__device__ __forceinline__ int tq_isum4rows(int x) {
    auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
    x = (int)r[0] + (int)r[1];
    r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
    return (int)r[0] + (int)r[1];
}

// ---- the static-grid arm ----------------------------------------------------------------------------------------------
struct TqStatic {
    RqWidth wd;        // last level, int8 offset (128 at 8 bits only) and its packed form
    RqsGrid g;         // the calibrated grid and the tie guard of its product form
};
// (kernel-uniform values computed by the VALU: handed to scalar registers, they are live for the whole position loop)
__device__ __forceinline__ float tq_uniform(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}
__device__ __forceinline__ TqStatic tq_static(const float* delta, const float* zp, int n_bits) {
    TqStatic q;
    q.wd = rq_width(n_bits);
    q.g = rqs_grid(delta, zp, 0, q.wd.qmax);
    q.g.delta = tq_uniform(q.g.delta), q.g.zp = tq_uniform(q.g.zp), q.g.inv = tq_uniform(q.g.inv), q.g.thr = tq_uniform(q.g.thr);
    return q;
}
// four values of one lane -> their dword of codes as stored (offset applied); csum += the raw codes
template <bool SAT8>
__device__ __forceinline__ uint32_t tq_static_codes(const float (&x4)[4], const TqStatic& q, uint32_t& csum) {
    uint32_t pk[1];
    rqs_quant<4, SAT8>(x4, q.g, q.wd.qmax, pk);
    csum = __builtin_amdgcn_sad_u8(pk[0], 0u, csum);
    return pk[0] ^ q.wd.flip;
}

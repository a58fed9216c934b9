// attn_rowquant.h - what the temporal attention kernels with the fused per-token quantizer share
// (attn_temporal_quant_kernel, attn_temporal_quant2_kernel, attn_temporal_long_kernel of attention.hip).
//
// The layout all of them use: one wave per head, 16x16 MFMA tiles, lane = (query row tq = lane & 15, row group
// g4 = lane >> 4).  S^T = K Q^T leaves lane (tq, g4) with keys 16 kt + 4 g4 .. + 3 of query tq; O^T = V^T P^T leaves it
// with dims 16 dt + 4 g4 .. + 3 of token tq.  A token's quantizer needs its whole row (all heads): every wave reduces its
// head's part over its four 16-lane rows, the parts meet in LDS (ex_min / ex_max / ex_sum: [wave][16] each, between two
// tq_lds_barrier()s), and every wave derives the same grid from them.  The contract: codes, scale, zero point and row
// sum are bit-identical to vq_rowquant of the kernel's own fp16 output.
//
// Every step of a position that does not depend on a kernel's load schedule or LDS map is written ONCE here and used by
// all three kernels in both of their forms (one exception, measured: the long kernel keeps its softmax written out, see
// there): the masked 16-key softmax (tq_softmax16), the V^T operand (tq_vt_frag), the
// optional fp16 copy (tq_store_o), x / s (tq_div_s), the row statistics of the dynamic grid (tq_minmax4 /
// tq_publish_minmax / tq_row_grid), the encode (tq_codes), the code-sum exchange (tq_publish_sum / tq_collect_sum), the
// record (rq_write_row of rowquant_shared.h) and the LDS barrier.  The kernels keep their load schedules, LDS maps, the
// place of their barriers, the O^T accumulation and the way codes leave.
// NOT shared: the reciprocal of the softmax row sum.  tq_softmax16 returns the sum and the caller inverts it - IEEE
// __fdiv_rn in the first-generation kernel, v_rcp_f32 (1 ulp) in the other two - because the fp16 output of each kernel
// is pinned bit for bit and the two differ in that ulp.
// (hipcc simplifies a forced-inline callee on its own before it inlines it, so these kernels do not compile to the
//  instruction streams of their written-out forms: profiles/refactor_attn_isa.md has what moved at the first attempt,
//  profiles/refactor_temporal_steps.md the resources and the timing on the MI355X that this form was accepted on.)
//
// One grid type, TqGrid, serves all forms.  The dynamic form (TempQArgs) derives it per row from the row's min / max
// (vq_row_grid, 8 bits) and encodes with rq_quant; the static form (TempQSArgs; vq_attn_temporal_rowquant_static) reads
// ONE calibrated grid (delta, zp: one fp32 value each, read on the device) at a code width of 2..8 bits: no row
// min / max, hence no ex_min / ex_max exchange, no vq_row_grid, no eps fill and no status word; only the row sum still
// crosses the heads.  Its codes are rqs_grid / rqs_quant of rowquant_shared.h - rq_round_group's bound needs the row's
// own grid - and bit-identical to vq_rowquant(delta_in, zp_in, n_param = 1) of the kernel's own fp16 output.
// The shared-grid form (TempQPArgs; vq_attn_temporal_rowquant_shared; the two T <= 16 kernels) is the dynamic form for a joint
// cond | uncond forward (B <= 2) at 2..8 bits: a token's grid comes from its min / max over all heads AND both samples
// (base_quantizer.py:177-189), so one workgroup owns a spatial position of every sample.  It runs the attention steps per
// sample, carries the lane's min / max from one sample to the next, keeps every sample's fp16 output in LDS (tq_park /
// tq_unpark: each lane reads back what it wrote, no barrier) and encodes the samples' rows on the one grid; the division
// by s is redone at the encode (deterministic, so the statistics and the codes see the same values).
#pragma once
#include "vq_common.h"
#include "rowquant_shared.h"

typedef __fp16 h4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));   // operand type of the LDS transpose read

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

// ---- the LDS barrier of the position loops ----------------------------------------------------------------------------
// (raw: __syncthreads() also waits for vmcnt(0), i.e. for the global loads in flight for the next positions - that
//  serialised every iteration behind one HBM round trip)
__device__ __forceinline__ void tq_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

// ---- softmax of one query over NKT tiles of 16 keys ---------------------------------------------------------------------
// sc[kt][r]: the score of key 16 kt + 4 g4 + r (keys >= T are masked here); pf: exp2((s - m) c) as the fp16 B operand
// of O^T = V^T P^T.  Returns the sum of the fp32 exponentials over all keys of the query (every lane of the query's
// column has it); a fully masked query (no row tq < T feeds it) gets m = 0, p = 0 and the sum 0.
template <int NKT>
__device__ __forceinline__ float tq_softmax16(float4v (&sc)[NKT], int g4, int T, float c, half4 (&pf)[NKT]) {
    float mloc = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (16 * kt + 4 * g4 + r >= T) sc[kt][r] = -INFINITY;
            mloc = fmaxf(mloc, sc[kt][r]);
        }
    mloc = tq_xor32(tq_xor16(mloc, true), true);
    const float m_use = (mloc == -INFINITY) ? 0.f : mloc;
    float psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f((sc[kt][r] - m_use) * c);
            psum += p;
            pf[kt][r] = (half_t)p;
        }
    return tq_sum4rows(psum);
}

// ---- the V^T operand of O^T = V^T P^T ------------------------------------------------------------------------------------
// (dim tq, keys 4 g4 .. + 3) by ONE LDS transpose read of a row-major tile: lane i of a 16-lane group points at
// [key 4 g4 + i / 4][dims 16 dt + 4 (i % 4) .. + 3] - p, the caller's LDS map - and receives column i of the 4 x 16 block
// (four 2-byte reads and their packing before).  Dims >= D of the last tile read whatever lies behind the head's
// columns: finite values in output rows nobody stores.
__device__ __forceinline__ half4 tq_vt_frag(const uint8_t* p) {
    const h4_t vt = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4_t*)p);
    return half4{(half_t)vt[0], (half_t)vt[1], (half_t)vt[2], (half_t)vt[3]};
}

// ---- the optional fp16 copy of a 16-query tile: this lane's dims 16 dt + 4 g4 .. + 3 of its token's head ---------------
// (ov: the fp16-rounded output, held as fp32 or as half4)
template <int D, class V>
__device__ __forceinline__ void tq_store_o(half_t* orow, const V (&ov)[(D + 15) / 16], int g4) {
#pragma unroll
    for (int dt = 0; dt < (D + 15) / 16; ++dt) {
        const int d0 = dt * 16 + 4 * g4;
        if (d0 < D) {
            half4 o4;
#pragma unroll
            for (int r = 0; r < 4; ++r) o4[r] = (half_t)ov[dt][r];
            *reinterpret_cast<half4*>(orow + d0) = o4;
        }
    }
}

// ---- the shared-grid form: a dim tile's O^T * (1 / sum p) rounded to fp16, and its parking place ----------------------------
// The fp16 output of the shared-grid form is pinned, bit for bit, to the dynamic form of the same kernel, and that form's
// rounding is hipcc's choice (profiles/refactor_temporal_steps.md, "A rounding the compiler chooses"): v_mul_f32 +
// v_cvt_pk_f16_f32 (the product rounded to fp32, then to fp16) everywhere in attn_temporal_quant2_kernel; in
// attn_temporal_quant_kernel the ONE rounding of v_fma_mixlo_f16 for the first two values of every dim tile but the first,
// two roundings for the rest.  MIXED spells that selection out, each rounding behind an asm so that it stays what is written
// (the instantiation alone, with the park as one more consumer, was compiled to two roundings everywhere); the other
// kernel's expression is the dynamic form's own, and its assembly is checked to hold no v_fma_mix* (profiles/temporal_shared).
// (the asm reads an MFMA result, and the wait states between the two are the compiler's to insert for instructions it knows:
//  an asm block is not one of them, so it brings its own - 12, where hipcc puts 8 at the most (s_nop 7) between such an MFMA
//  and the first VALU read of its result in these kernels)
template <bool MIXED>
__device__ __forceinline__ half4 tq_round_o(const float4v& o4, float inv_p, int dt) {
    half4 h;
    if constexpr (MIXED) {
        if (dt >= 1) {
            uint32_t lo0, lo1;
            asm("s_nop 7\n\ts_nop 3\n\tv_fma_mixlo_f16 %0, %2, %3, 0\n\tv_fma_mixlo_f16 %1, %2, %4, 0"
                : "=&v"(lo0), "=&v"(lo1)
                : "v"(inv_p), "v"(o4[0]), "v"(o4[1]));
            h[0] = __builtin_bit_cast(half_t, (uint16_t)lo0);
            h[1] = __builtin_bit_cast(half_t, (uint16_t)lo1);
        }
#pragma unroll
        for (int r = dt >= 1 ? 2 : 0; r < 4; ++r) {
            float p = o4[r] * inv_p;
            asm("" : "+v"(p));
            h[r] = (half_t)p;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = (half_t)(o4[r] * inv_p);
    }
    return h;
}
// this lane's four fp16 outputs of dim tile dt, [dt][thread] 8 bytes each: each lane reads back what it wrote, no barrier
__device__ __forceinline__ void tq_park(uint8_t* park, int nthr, int tid, int dt, const half4& h) {
    *reinterpret_cast<half4*>(park + ((size_t)dt * nthr + tid) * 8) = h;
}
__device__ __forceinline__ void tq_unpark(const uint8_t* park, int nthr, int tid, int dt, float (&x4)[4]) {
    const half4 h = *reinterpret_cast<const half4*>(park + ((size_t)dt * nthr + tid) * 8);
#pragma unroll
    for (int r = 0; r < 4; ++r) x4[r] = (float)h[r];
}

// ---- the quantizer's input: x / s of the consuming Linear's smoothing vector when it has one ----------------------------
// (quant_layer.py:140; reciprocal form, bit-identical to the IEEE quotient - vq_common.h.)  ch: the channel of x4[0].
template <class V>                                 // V: float[4] or float4v
__device__ __forceinline__ void tq_div_s(V& x4, const float* s, const float* s_rcp, int ch) {
    if (s) {                                       // kernel-uniform
        const float4v s4 = *reinterpret_cast<const float4v*>(s + ch);
        const float4v r4 = *reinterpret_cast<const float4v*>(s_rcp + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) x4[r] = rq_div_rcp(x4[r], s4[r], r4[r]);
    }
}

// ---- one grid for both forms ---------------------------------------------------------------------------------------------
struct TqGrid {
    RqWidth wd;        // last level, int8 offset (128 at 8 bits only) and its packed form
    RqsGrid g;         // step, zero point, reciprocal; thr: the tie guard of the static product form (unused by the dynamic one)
};
// (kernel-uniform values computed by the VALU: handed to scalar registers, they are live for the whole position loop)
__device__ __forceinline__ float tq_uniform(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}
// the static form's grid: once per kernel
__device__ __forceinline__ TqGrid tq_static(const float* delta, const float* zp, int n_bits) {
    TqGrid q;
    q.wd = rq_width(n_bits);
    q.g = rqs_grid(delta, zp, 0, q.wd.qmax);
    q.g.delta = tq_uniform(q.g.delta), q.g.zp = tq_uniform(q.g.zp), q.g.inv = tq_uniform(q.g.inv), q.g.thr = tq_uniform(q.g.thr);
    return q;
}

// ---- row statistics of the dynamic form ----------------------------------------------------------------------------------
template <class V>
__device__ __forceinline__ void tq_minmax4(const V& x4, float& vmin, float& vmax) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        vmin = fminf(vmin, x4[r]);
        vmax = fmaxf(vmax, x4[r]);
    }
}
// this head's min / max of token tq: reduced over the wave's four rows, published for the other heads
__device__ __forceinline__ void tq_publish_minmax(float vmin, float vmax, float* ex_min, float* ex_max, int wave, int lane) {
    vmin = tq_xor32(tq_xor16(vmin, false), false);
    vmax = tq_xor32(tq_xor16(vmax, true), true);
    if (lane < 16) {
        ex_min[wave * 16 + lane] = vmin;
        ex_max[wave * 16 + lane] = vmax;
    }
}
// (behind the barrier) token tq's min / max over the H heads -> its grid at n_bits (8 in the dynamic form), as vq_rowquant
// derives it; ``flag``: this lane reports the row's eps fill (one lane per stored row)
__device__ __forceinline__ TqGrid tq_row_grid(const float* ex_min, const float* ex_max, int H, int tq, bool flag, int32_t* status,
                                              int n_bits = 8) {
    float vmin = INFINITY, vmax = -INFINITY;
    for (int w = 0; w < H; ++w) {
        vmin = fminf(vmin, ex_min[w * 16 + tq]);
        vmax = fmaxf(vmax, ex_max[w * 16 + tq]);
    }
    TqGrid q;
    q.wd = rq_width(n_bits);
    q.g.thr = 0.f;
    bool small;
    vq_row_grid(vmin, vmax, q.wd.qmax, q.g.delta, q.g.zp, small, q.g.inv);
    if (small && flag && status) atomicOr(status, VQ_ST_EPSFILL);
    return q;
}

// ---- encode: four values of one lane -> their dword of codes as stored (offset applied); csum += the raw codes ----------
// (SAT8: inside RQ_BY_WIDTH(q.wd.qmax, ...), once around the caller's loop; the dynamic form's width is a constant, so
//  its other arm folds away)
template <bool SAT8>
__device__ __forceinline__ uint32_t tq_static_codes(const float (&x4)[4], const TqGrid& q, uint32_t& csum) {
    uint32_t pk[1];
    rqs_quant<4, SAT8>(x4, q.g, q.wd.qmax, pk);
    csum = __builtin_amdgcn_sad_u8(pk[0], 0u, csum);
    return pk[0] ^ q.wd.flip;
}
template <bool ST, bool SAT8>
__device__ __forceinline__ uint32_t tq_codes(const float (&x4)[4], const TqGrid& q, uint32_t& csum) {
    if constexpr (ST) {
        return tq_static_codes<SAT8>(x4, q, csum);
    } else {
        uint32_t pk[1];
        rq_quant<4, SAT8>(x4, q.g.inv, q.g.delta, q.g.zp, q.wd.qmax, pk);   // one tie test per four codes, packed fp32 math
        csum = __builtin_amdgcn_sad_u8(pk[0], 0u, csum);
        return pk[0] ^ q.wd.flip;
    }
}

// ---- code-sum exchange: this head's part of token tq's row sum into exs[wave][16]; (behind the barrier) the row's sum ----
__device__ __forceinline__ void tq_publish_sum(uint32_t csum, int* exs, int wave, int lane) {
    const int cs = tq_isum4rows((int)csum);
    if (lane < 16) exs[wave * 16 + lane] = cs;
}
__device__ __forceinline__ int tq_collect_sum(const int* exs, int H, int tq) {
    int rs = 0;
    for (int w = 0; w < H; ++w) rs += exs[w * 16 + tq];
    return rs;
}

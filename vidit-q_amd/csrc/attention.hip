// attention.hip - fp16 attention (fp32 online softmax) for gfx950.
//
// Replaces flash_attn_func / the fp32-softmax branch of Attention.forward
// (opensora/models/layers/blocks.py:169-187), xformers block-diagonal
// memory_efficient_attention of MultiHeadCrossAttention (blocks.py:292-310) and PixArt's
// xformers self-attention (t2i/diffusion/model/nets/PixArt_blocks.py:151-155).
// No activation quantization happens inside attention in the reference
// (quant_block.py:617-632 is commented out), so q, k, v, P stay fp16 / fp32.
//
// attn_fwd_kernel (spatial, cross, image): flash-style, one 256-thread workgroup per
// (128-query tile, head, sequence); K and V tiles [64 keys][D] staged row-major in LDS, double
// buffered (V^T fragments are gathered by conflict-free column reads); v_mfma_f32_32x32x16_f16 computes S^T = K Q^T (so one lane owns one
// query column: softmax statistics are lane-local plus one lane^32 exchange) and
// O^T = V^T P^T (the P^T accumulator quads are already the B operand once the key order
// inside each 16-key step is permuted identically on the V^T side).
// head_dim 72 is contracted as 5 k-steps of 16 (zero tail) and produced as 3 row tiles of 32.
//
// attn_temporal_kernel: T <= 16 tokens per sequence, 1024*B sequences: HBM-bound; one
// workgroup = 2 spatial positions x 4 heads, rows staged once through LDS with full-width
// coalesced loads, one wave per head, 32x32 MFMA over the 2x16 token rows with a
// block-diagonal mask.
//
// attn_temporal_quant_kernel / attn_temporal_quant2_kernel (T <= 16) and attn_temporal_long_kernel (T <= 64): temporal
// attention with the consuming Linear's per-token quantizer fused in; one argument struct (TempQArgs), and the lane layout,
// LDS exchange contract and every step of a position that does not depend on a kernel's load schedule or LDS map - softmax,
// V^T operand, fp16 copy, x / s, row statistics, grid, encode, code-sum exchange, record, LDS barrier - once in
// attn_rowquant.h: a kernel body here is its load schedule, LDS map, barrier placement, O^T accumulation and the way its codes
// leave.  Each has a static-grid form (instantiated on the argument struct TempQSArgs, vq_attn_temporal_rowquant_static):
// attn_temp.proj's calibrated tensor-wise quantizer at 2..8 bits, on the same steps through the one grid type TqGrid.
//
// The five flash-style kernels behind vq_attn_fwd are written on the shared steps of attn_tile.h (geometry, operand reads,
// LDS-DMA delivery, softmax, epilogue): a kernel body here is its schedule.  Two blocks are written out where the helper cost
// a measured register bound or timing band: attn_fwd8_kernel's lazy rescale, attn_fwd64d_kernel's softmax block.
//
// Host side: every launcher goes through vq_prepare_kernel (dynamic-LDS limit and CU count once per device, vq_common.h)
// and every entry point picks the head dim with vq_dispatch_head_dim.  Nothing here reads the environment or depends on a
// build flag, and no kernel has a profiling or ablation arm: the retired kernels and A/B arms are the lab's attn_lab.hip,
// which includes this file.
#include "vq_common.h"
#include "attn_rowquant.h"
#include "attn_tile.h"

template <int D>
struct AttCfg {
    static constexpr int KS = (D + 15) / 16;       // QK^T k-steps (16 dims each)
    static constexpr int DT = (D + 32) / 32;       // O^T row tiles: D dims + 1 spare row for the row sums
    static constexpr int CHD = D / 8;              // 16-byte chunks per head row
    static constexpr int KROW = (CHD | 1) * 16;    // K tile row stride (odd # of 16 B slots)
    // V tile: KEY-PAIR interleaved [key/2][D | ones | pad] dwords, each dword = {V[2j][d], V[2j+1][d]}: one
    // ds_read_b32 per lane fetches the fp16 pair an MFMA A-operand register needs (lane = output dim d), the
    // interleave is done in registers while staging (lanes l, l^1 hold the two keys of a pair).  Column D holds
    // {1,1} so that the P.V MFMA also yields the softmax row sums (row D of O^T).
    static constexpr int VROW = ((D + 1 + 3) / 4 * 4) * 4 + 16;   // bytes per key pair row (16 B aligned)
    static constexpr int KTILE = 64 * KROW;
    static constexpr int VTILE = 32 * VROW;
    static constexpr int LDS = 2 * (KTILE + VTILE);
    static constexpr int KCH = 64 * CHD;           // K (and V) chunks per tile
    static constexpr int KPT = (KCH + 255) / 256;
    static_assert(DT * 32 > D, "needs a spare O^T row for the row sums");
};

// (AttnArgs, the argument block of every vq_attn_fwd kernel, is declared in attn_tile.h: the shared steps take it)
// A = AttnQSArgs: the static-grid form ST (attn_tile.h: attn_quant_rows) - the consuming Linear's calibrated quantizer as one
// more epilogue step, `o` optional.  The same holds for attn_fwd32d_kernel, attn_fwd64d_kernel and attn_cross32_kernel.
template <int D, class A = AttnArgs>
__global__ __launch_bounds__(256) void attn_fwd_kernel(A a) {
    constexpr bool ST = std::is_same<A, AttnQSArgs>::value;
    using C = AttCfg<D>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int qt = blockIdx.x, h = blockIdx.y, seq = blockIdx.z;
    [[maybe_unused]] TqGrid sq;
    if constexpr (ST) sq = tq_static(a.delta, a.zp, a.n_bits);

    const half_t* kbase;
    const half_t* vbase;
    const int kv_len = attn_kv_base<D>(a, seq, h, kbase, vbase);
    const int qi = qt * 128 + wave * 32 + l31;
    const bool q_ok = qi < a.Lq;
    const int qc = q_ok ? qi : a.Lq - 1;

    half8 qf[C::KS];                                    // Q fragments (B operand): lane = query, 8 dims at ks*16 + 8g
    attn_q_frags<D>(a.q + (long)seq * a.q_seq_stride + (long)qc * a.q_tok_stride + h * D, g, qf);
    float16v oacc[C::DT];
    attn_zero(oacc);
    float m_run = -INFINITY;

    const int nkt = (kv_len + 63) / 64;
    int4v kr[C::KPT], vr[C::KPT];
    auto load_tile = [&](int kt) {
#pragma unroll
        for (int i = 0; i < C::KPT; ++i) {
            const int c = tid + i * 256;
            if (C::KCH % 256 == 0 || c < C::KCH) {
                int key = kt * 64 + c / C::CHD;
                key = key < kv_len ? key : kv_len - 1;
                kr[i] = *reinterpret_cast<const int4v*>(kbase + (long)key * a.kv_tok_stride + (c % C::CHD) * 8);
                // V: lanes c, c^1 hold the same 8-dim chunk of the two keys of pair (c>>1)/CHD
                int vkey = kt * 64 + 2 * ((c >> 1) / C::CHD) + (c & 1);
                vkey = vkey < kv_len ? vkey : kv_len - 1;
                vr[i] = *reinterpret_cast<const int4v*>(vbase + (long)vkey * a.kv_tok_stride + ((c >> 1) % C::CHD) * 8);
            }
        }
    };
    auto store_tile = [&](int buf) {
        uint8_t* kt_ = smem + buf * C::KTILE;
        uint8_t* vt_ = smem + 2 * C::KTILE + buf * C::VTILE;
#pragma unroll
        for (int i = 0; i < C::KPT; ++i) {
            const int c = tid + i * 256;
            if (C::KCH % 256 == 0 || c < C::KCH) {
                *reinterpret_cast<int4v*>(kt_ + (c / C::CHD) * C::KROW + (c % C::CHD) * 16) = kr[i];
                const int odd = c & 1;
                // exchange with the pair partner: the even lane assembles dims 0-3 of the chunk, the odd one 4-7
                const int r0 = __shfl_xor(odd ? vr[i][0] : vr[i][2], 1);
                const int r1 = __shfl_xor(odd ? vr[i][1] : vr[i][3], 1);
                const uint32_t lo0 = odd ? (uint32_t)r0 : (uint32_t)vr[i][0], lo1 = odd ? (uint32_t)r1 : (uint32_t)vr[i][1];
                const uint32_t hi0 = odd ? (uint32_t)vr[i][2] : (uint32_t)r0, hi1 = odd ? (uint32_t)vr[i][3] : (uint32_t)r1;
                int4v pv;
                pv[0] = (int)((lo0 & 0xffffu) | (hi0 << 16));
                pv[1] = (int)((lo0 >> 16) | (hi0 & 0xffff0000u));
                pv[2] = (int)((lo1 & 0xffffu) | (hi1 << 16));
                pv[3] = (int)((lo1 >> 16) | (hi1 & 0xffff0000u));
                *reinterpret_cast<int4v*>(vt_ + ((c >> 1) / C::CHD) * C::VROW + (((c >> 1) % C::CHD) * 8 + 4 * odd) * 4) = pv;
            }
        }
    };

    // column D of both V buffers := {1.0, 1.0} (never overwritten by the staging stores)
    if (tid < 64)
        *reinterpret_cast<uint32_t*>(smem + 2 * C::KTILE + (tid >> 5) * C::VTILE + (tid & 31) * C::VROW + D * 4) = 0x3c003c00u;
    if (nkt > 0) {
        load_tile(0);
        store_tile(0);
    }
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) load_tile(kt + 1);
        const uint8_t* kt_ = smem + cur * C::KTILE;
        const uint8_t* vt_ = smem + 2 * C::KTILE + cur * C::VTILE;

        // ---- S^T = K Q^T for two 32-key sub-tiles ----
        float16v s[2];
#pragma unroll
        for (int sc = 0; sc < 2; ++sc) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[sc][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks)
                s[sc] = __builtin_amdgcn_mfma_f32_32x32x16_f16(attn_frag<D>(kt_ + (sc * 32 + l31) * C::KROW, ks, g), qf[ks], s[sc], 0, 0, 0);
        }
        // ---- online softmax (lane = query; its 64 keys sit in 32 registers here and 32 in lane^32) ----
        // VALU is the bound of this kernel (PMC: VALU busy 65 %, MFMA 18 %), so: masking only on a partial
        // last tile (wave-uniform branch), exponent as one fma + v_exp, the O rescale only when some lane's
        // running max moved, and NO row-sum adds: column D of V is 1.0, so row D of O^T is sum_k P.
        if (kt * 64 + 64 > kv_len) {
#pragma unroll
            for (int sc = 0; sc < 2; ++sc) attn_mask(s[sc], kt * 64 + sc * 32, g, kv_len);
        }
        const float mloc = attn_rowmax_shfl(s);
        const float m_new = fmaxf(m_run, mloc);
        const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
        if (__any(m_new != m_run)) {
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * a.c);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
            m_run = m_new;
        }
        const float mc = m_use * a.c;
#pragma unroll
        for (int sc = 0; sc < 2; ++sc)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[sc][r] = __builtin_amdgcn_exp2f(fmaf(s[sc][r], a.c, -mc));

        // ---- O^T += V^T P^T : 4 k-steps of 16 keys ----
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int sc = kk >> 1, rq = 2 * (kk & 1);
            half8 pf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pf[e] = (half_t)s[sc][4 * rq + e];
                pf[4 + e] = (half_t)s[sc][4 * rq + 4 + e];
            }
            // V^T fragment (A operand: lane = output dim d, 8 keys) = 4 dwords of the key-pair image,
            // 32 lanes read 32 consecutive dwords -> conflict-free.
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) {
                const int d = dt * 32 + l31;          // d == D: the ones column; d > D: clamped, result unused
                const uint8_t* vp = vt_ + (8 * kk + 2 * g) * C::VROW + (d <= D ? d : D) * 4;
                int4v vw;                             // key pairs (4g+0,1) (4g+2,3) (8+4g+0,1) (8+4g+2,3) of step kk
                vw[0] = *reinterpret_cast<const int*>(vp);
                vw[1] = *reinterpret_cast<const int*>(vp + C::VROW);
                vw[2] = *reinterpret_cast<const int*>(vp + 4 * C::VROW);
                vw[3] = *reinterpret_cast<const int*>(vp + 5 * C::VROW);
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, vw), pf, oacc[dt], 0, 0, 0);
            }
        }
        if (kt + 1 < nkt) store_tile(cur ^ 1);
        __syncthreads();
    }

    // ---- normalise and store: lane = query, accumulator quads = 4 consecutive dims ----
    const float inv = attn_inv_row_sum<D>(oacc, l31);
    if constexpr (ST) {
        if (a.o && q_ok) attn_store_rows_h4<D>(oacc, inv, a.o + (long)seq * a.o_seq_stride + (long)qi * a.o_tok_stride + h * D, g);
        attn_quant_rows<D>(oacc, inv, a, sq, seq * a.Lq + qc, h, g, q_ok);
    } else {
        if (q_ok) attn_store_rows_h4<D>(oacc, inv, a.o + (long)seq * a.o_seq_stride + (long)qi * a.o_tok_stride + h * D, g);
    }
}

// ---------------------------------------------------------------------------
// temporal attention, T <= 16
// ---------------------------------------------------------------------------
struct TempArgs {
    const half_t* q;
    const half_t* k;
    const half_t* v;
    half_t* o;
    long ld_in, ld_out;  // row strides in elements; row(b,t,s) = (b*T + t)*S + s
    int B, T, S, H;
    float c;
};

template <int D>
__global__ __launch_bounds__(256) void attn_temporal_kernel(TempArgs a) {
    constexpr int KS = (D + 15) / 16, DT = (D + 31) / 32, CHD = D / 8;
    constexpr int SEGCH = 4 * CHD;                 // chunks per (row, 4 heads)
    constexpr int RS = 4 * D * 2 + 16;             // LDS row stride (bytes), +16 de-conflicts b128 reads
    constexpr int TILE = 32 * RS;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int s0 = blockIdx.x * 2, h0 = blockIdx.y * 4, b = blockIdx.z;
    const int nh = (a.H - h0) < 4 ? (a.H - h0) : 4;  // heads present in this quad

    // ---- stage Q, K, V rows [2 s][16 t] x [4 heads * D] through LDS (coalesced 16 B chunks) ----
    // ALL loads of a thread are issued before its first LDS write (constant trip count, registers): with one
    // load -> wait -> store per iteration the kernel serialised 14 HBM round trips per workgroup
    constexpr int NCHK = 3 * 32 * SEGCH, NIT = (NCHK + 255) / 256;
    int4v vals[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int c = tid + i * 256;
        const int ten = c / (32 * SEGCH), rem = c % (32 * SEGCH);
        const int row = rem / SEGCH, ch = rem % SEGCH;
        const int sl = row >> 4, t = row & 15;
        vals[i] = int4v{0, 0, 0, 0};
        if (c < NCHK && t < a.T && s0 + sl < a.S && ch < nh * CHD) {
            const half_t* base = ten == 0 ? a.q : (ten == 1 ? a.k : a.v);
            const long grow = ((long)b * a.T + t) * a.S + s0 + sl;
            vals[i] = *reinterpret_cast<const int4v*>(base + grow * a.ld_in + h0 * D + ch * 8);
        }
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int c = tid + i * 256;
        const int ten = c / (32 * SEGCH), rem = c % (32 * SEGCH);
        const int row = rem / SEGCH, ch = rem % SEGCH;
        if (c < NCHK) *reinterpret_cast<int4v*>(smem + ten * TILE + row * RS + ch * 16) = vals[i];
    }
    __syncthreads();
    if (wave >= nh) return;
    const uint8_t* qs = smem + wave * D * 2;
    const uint8_t* ksm = qs + TILE;
    const uint8_t* vs = qs + 2 * TILE;

    float16v s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int d0 = ks * 16 + 8 * g;
        half8 kf = *reinterpret_cast<const half8*>(ksm + l31 * RS + (d0 < D ? d0 : 0) * 2);
        half8 qf = *reinterpret_cast<const half8*>(qs + l31 * RS + (d0 < D ? d0 : 0) * 2);
        if (d0 >= D)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                kf[e] = (half_t)0.f;
                qf[e] = (half_t)0.f;
            }
        s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf, s, 0, 0, 0);
    }
    const int sq = l31 >> 4, tq = l31 & 15;
    float mloc = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int krow = (r & 3) + 8 * (r >> 2) + 4 * g;
        const bool ok = ((krow >> 4) == sq) && ((krow & 15) < a.T);
        if (!ok) s[r] = -INFINITY;
        mloc = fmaxf(mloc, s[r]);
    }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
    const float m_use = (mloc == -INFINITY) ? 0.f : mloc;
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f((s[r] - m_use) * a.c);
        s[r] = p;
        psum += p;
    }
    psum += __shfl_xor(psum, 32);
    const float inv = psum > 0.f ? __fdiv_rn(1.0f, psum) : 0.f;

    float16v oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        half8 pf;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            pf[e] = (half_t)s[8 * kk + e];
            pf[4 + e] = (half_t)s[8 * kk + 4 + e];
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d = dt * 32 + l31;
            half8 vf;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int krow = 16 * kk + 4 * g + (e & 3) + 8 * (e >> 2);
                vf[e] = d < D ? *reinterpret_cast<const half_t*>(vs + krow * RS + d * 2) : (half_t)0.f;
            }
            oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[dt], 0, 0, 0);
        }
    }
    if (tq < a.T && s0 + sq < a.S) {
        const long grow = ((long)b * a.T + tq) * a.S + s0 + sq;
        attn_store_rows_h4<D>(oacc, inv, a.o + grow * a.ld_out + (h0 + wave) * D, g);
    }
}

// ---------------------------------------------------------------------------
// attn_temporal_quant_kernel: temporal attention + the per-token quantizer of the Linear that consumes it
// (attn_temp.proj's DynamicActQuantizer, stdit.py:116 -> stdit_quant_layer.py:161-166) in one pass.
// A token's quantizer needs its whole row (all heads), so one workgroup = ONE spatial position x ALL heads
// (one wave per head, H <= 16), the T <= 16 rows of q | k | v staged once through LDS.  Each wave computes its
// head with 16x16x16 MFMAs (S^T = K Q^T leaves the matrix core in the layout P^T needs as the B operand of
// O^T = V^T P^T), rounds the output to fp16 as the unfused path stores it, and the row min / max / code sum are
// combined over the waves through LDS.  The fp16 attention output (37.7 MB per block-sample) never goes to HBM and the separate
// quantizer pass (read 37.7 MB, write 18.9 MB) disappears; codes leave through LDS as whole 16-byte chunks.
// ---------------------------------------------------------------------------
struct TempQArgs {
    const half_t* q;
    const half_t* k;
    const half_t* v;
    int8_t* xq;                                    // nullable in attn_temporal_long_kernel: no quantizer (plain fp16 output)
    float* sx;
    int32_t* zx;
    int32_t* R;
    int32_t* status;
    half_t* o;                                     // nullable (not when xq is null): also store the fp16 attention output [B*T*S, ld_out]
    const float* s;                                // nullable [H*D]: smooth-quant channel scale of the consuming Linear
    const float* s_rcp;                            //                 and its reciprocal (vq_smooth_reciprocal)
    long ld_in, ld_out;                            // row strides in elements (the T <= 16 kernels store o densely: ld_out = H*D)
    int B, T, S, H, Kp;
    float c;
};
// the static-grid forms (ST) add the calibrated grid of the consuming Linear - one fp32 value each, read by the kernel -
// and the code width; the dynamic forms keep their argument block as it was
struct TempQSArgs : TempQArgs {
    const float* delta;
    const float* zp;
    int n_bits;                                    // 2 .. 8
};

// the shared-grid form (SH; vq_attn_temporal_rowquant_shared): the dynamic form for B <= 2 samples whose tokens share ONE grid
// per (t, s) at a code width of 2..8 bits - a joint cond | uncond forward (iddpm/__init__.py:141-163, base_quantizer.py:177-189)
struct TempQPArgs : TempQArgs {
    int n_bits;                                    // 2 .. 8
};
// The walk of a persistent workgroup over its positions.  Dynamic / static forms: position = (b, s), pos = b * S + s, one
// after the other in steps of the grid.  SH: a workgroup owns the spatial position s of ALL samples, pos = s * B + b with b
// fastest (B is 1 or 2), and moves on by the grid only behind the last sample.
template <bool SH>
__device__ __forceinline__ int tq_next_pos(int pos, int G, int B) {
    if constexpr (SH) return (pos & (B - 1)) == B - 1 ? pos + (G - 1) * B + 1 : pos + 1;
    else return pos + G;
}

// The head count is a.H (the chunk -> (tensor, row, piece) divisions of the staging loops are by H * D / 8 and cost ~45
// VALU instructions each with a run-time divisor: the H = 16 kernel is attn_temporal_quant2_kernel below).
// A = TempQSArgs: the static-grid form ST (attn_rowquant.h): a.delta / a.zp / a.n_bits instead of the row's own 8-bit
// grid, any B.  A = TempQPArgs: the shared-grid form SH (attn_rowquant.h): one grid per token over both samples at a.n_bits;
// LDS: a code area and a sum area per sample, and the parked fp16 output of every sample behind them
template <int D, class A = TempQArgs>
__global__ __launch_bounds__(1024) void attn_temporal_quant_kernel(A a) {
    constexpr bool ST = std::is_same<A, TempQSArgs>::value;
    constexpr bool SH = std::is_same<A, TempQPArgs>::value;
    constexpr int NCB = SH ? 2 : 1;                // code / sum areas (one per sample of a shared grid)
    constexpr int KS = (D + 15) / 16;              // 16-dim k-steps of QK^T = 16-dim row tiles of O^T
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // = head
    const int tq = lane & 15, g4 = lane >> 4;      // MFMA 16x16x16: lane = (row or column tq, k / row group g4)
    const int H = a.H, C = H * D, nthr = 64 * H;
    const int RS = C * 2 + 16;                     // LDS row stride (odd number of 16-byte slots)
    const int TILE = 16 * RS;
    const int RCH = C / 8;                         // 16-byte chunks per tensor row
    const int CROW = C + 16;                       // code row stride in LDS (rows land 4 banks apart)
    // [V tile | codes | row statistics]; SH: [V tile | row statistics | codes | parked output] - with two code areas in
    // front of them the statistics would lie beyond the 64 KB that a DS instruction's offset reaches, and every one of the
    // 2 * H addresses of tq_row_grid's reads became a register of its own
    uint8_t* codes = smem + TILE + (SH ? 4 * 1024 : 0);
    float* ex_min = reinterpret_cast<float*>(SH ? smem + TILE : codes + 16 * CROW);
    float* ex_max = ex_min + 256;
    int* ex_sum = reinterpret_cast<int*>(ex_max + 256);
    [[maybe_unused]] uint8_t* park = codes + NCB * 16 * CROW;
    const int npos = a.S * a.B, G = (int)gridDim.x;
    // pos -> (s, b)
    auto pos_s = [&](int pos) { if constexpr (SH) return pos >> (a.B - 1); else return pos % a.S; };
    auto pos_b = [&](int pos) { if constexpr (SH) return pos & (a.B - 1); else return pos / a.S; };

    // One workgroup walks positions p, p + G, ...: while position p is computed, the rows of the next one are in flight
    // into registers (a one-position-per-workgroup version ran load -> compute -> store in lockstep on every CU:
    // 2.8 TB/s).  Only V goes through LDS (its MFMA operand is the transpose of the stored rows); the K and Q
    // operands of S^T = K Q^T are the stored rows themselves - lane (tq, g4) needs 4 dims of row tq per k-step - and
    // come straight from global memory in operand form: staging all of q | k | v (111 KB per position) through
    // ds_write_b128 at ~79 B/clk was 1400 of the ~1600 cycles a position took.
    constexpr int NITMAX = 3;                      // 16 * 144 V chunks / 1024 threads (H = 16, D = 72)
    const int nchk = 16 * RCH;
    int4v vals[NITMAX];
    constexpr int KS2 = (D + 31) / 32;             // 32-dim k-steps of the 16x16x32 form of QK^T
    half8 kfn[KS2], qfn[KS2];                      // next position's operands (in flight), copied over after use
    // (tx: an opaque per-position copy of the thread id, so that the chunk -> address arithmetic is recomputed per
    //  position instead of being hoisted out of the loop and kept in registers)
    auto load_qkv = [&](int pos, int tx) {
        const int s = pos_s(pos), b = pos_b(pos);
#pragma unroll
        for (int i = 0; i < NITMAX; ++i) {
            const int c = tx + i * nthr;
            const int t = c / RCH, ch = c - t * RCH;
            vals[i] = int4v{0, 0, 0, 0};
            if (c < nchk && t < a.T) {
                const long grow = ((long)b * a.T + t) * a.S + s;
                vals[i] = *reinterpret_cast<const int4v*>(a.v + grow * a.ld_in + ch * 8);
            }
        }
        // 16x16x32 operand form: lane (row tq, k-group g4) holds dims 32 * step + 8 * g4 .. + 7 of row tq - one 16-byte
        // load, and the four k-groups of a row read 64 contiguous bytes (whole cache lines, like the GEMM's DMA pieces)
        const int ln = tx & 63, tq_ = ln & 15, g4_ = ln >> 4;
        const long grow = ((long)b * a.T + (tq_ < a.T ? tq_ : 0)) * a.S + s;
        const half_t* krow = a.k + grow * a.ld_in + wave * D;
        const half_t* qrow = a.q + grow * a.ld_in + wave * D;
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) {
            const int d0 = ks * 32 + 8 * g4_;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                kfn[ks][e] = (half_t)0.f;
                qfn[ks][e] = (half_t)0.f;
            }
            if (d0 < D && tq_ < a.T) {
                kfn[ks] = *reinterpret_cast<const half8*>(krow + d0);
                qfn[ks] = *reinterpret_cast<const half8*>(qrow + d0);
            }
        }
    };
    auto store_qkv = [&](int tx) {
#pragma unroll
        for (int i = 0; i < NITMAX; ++i) {
            const int c = tx + i * nthr;
            const int t = c / RCH, ch = c - t * RCH;
            if (c < nchk) *reinterpret_cast<int4v*>(smem + t * RS + ch * 16) = vals[i];
        }
    };
    const uint8_t* vs = smem + wave * D * 2;
    TqGrid gq;                                     // ST: the calibrated grid; else every row's own, behind its statistics
    if constexpr (ST) gq = tq_static(a.delta, a.zp, a.n_bits);

    int pos = SH ? blockIdx.x * a.B : blockIdx.x;
    if (pos >= npos) return;
    load_qkv(pos, tid);
    store_qkv(tid);
    half8 kfc[KS2], qfc[KS2];
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks) {
        kfc[ks] = kfn[ks];
        qfc[ks] = qfn[ks];
    }
    __syncthreads();
    if (tq_next_pos<SH>(pos, G, a.B) < npos) load_qkv(tq_next_pos<SH>(pos, G, a.B), tid);
    [[maybe_unused]] float shmin = INFINITY, shmax = -INFINITY;   // SH: a token's extremes, carried from one sample to the next
    for (int npos_next; pos < npos; pos = npos_next) {
        const int s = pos_s(pos), b = pos_b(pos);
        npos_next = tq_next_pos<SH>(pos, G, a.B);
        const bool has_next = npos_next < npos;    // workgroup-uniform; its rows are already in flight
        [[maybe_unused]] const bool last = !SH || b == a.B - 1;   // SH: the position's statistics are complete
        int tx = tid;
        asm volatile("" : "+v"(tx));

        // ---- S^T[key 4*g4 + r][query tq] = K Q^T, 16 x 16 per head: lane holds 8 dims of key row tq and of query row tq
        float4v sc[1] = {{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) sc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kfc[ks], qfc[ks], sc[0], 0, 0, 0);
        half4 pf[1];
        const float psum = tq_softmax16<1>(sc, g4, a.T, a.c, pf);
        const float inv_p = psum > 0.f ? __fdiv_rn(1.0f, psum) : 0.f;    // (IEEE here, v_rcp_f32 in the other two: attn_rowquant.h)

        if constexpr (SH) {
            // the shared-grid form: a dim tile at a time - round (as the dynamic form of this kernel does: tq_round_o), store,
            // park, and this head's part of the token's extremes over the samples so far
            half_t* orow = a.o + (((long)b * a.T + tq) * a.S + s) * C + wave * D;
#pragma unroll
            for (int dt = 0; dt < KS; ++dt) {
                const half4 vf = tq_vt_frag(vs + (4 * g4 + (tq >> 2)) * RS + (dt * 16 + 4 * (tq & 3)) * 2);
                const float4v o4 = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[0], float4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                const half4 oh = tq_round_o<true>(o4, inv_p, dt);
                const int d0 = dt * 16 + 4 * g4;
                if (d0 < D) {
                    if (a.o && tq < a.T) *reinterpret_cast<half4*>(orow + d0) = oh;
                    tq_park(park + b * KS * nthr * 8, nthr, tid, dt, oh);
                    float x4[4] = {(float)oh[0], (float)oh[1], (float)oh[2], (float)oh[3]};
                    tq_div_s(x4, a.s, a.s_rcp, wave * D + d0);
                    tq_minmax4(x4, shmin, shmax);
                }
            }
            if (last) {
                tq_publish_minmax(shmin, shmax, ex_min, ex_max, wave, lane);
                shmin = INFINITY, shmax = -INFINITY;
            }
            tq_lds_barrier();                      // row statistics visible; every wave is done with the q | k | v tiles
            if (has_next) {                        // (as below)
                store_qkv(tx);
#pragma unroll
                for (int ks = 0; ks < KS2; ++ks) {
                    kfc[ks] = kfn[ks];
                    qfc[ks] = qfn[ks];
                }
                if (tq_next_pos<SH>(npos_next, G, a.B) < npos) load_qkv(tq_next_pos<SH>(npos_next, G, a.B), tx);
            }
            if (last) {                            // one grid for the token's rows of all samples, each from where it was parked
                gq = tq_row_grid(ex_min, ex_max, H, tq, tid < 16 && tq < a.T, a.status, a.n_bits);
                for (int bb = 0; bb < a.B; ++bb) {
                    uint32_t csum = 0;
                    RQ_BY_WIDTH(gq.wd.qmax, _Pragma("unroll") for (int dt = 0; dt < KS; ++dt) {
                        const int d0 = dt * 16 + 4 * g4;
                        if (d0 < D) {
                            float x4[4];
                            tq_unpark(park + bb * KS * nthr * 8, nthr, tid, dt, x4);
                            tq_div_s(x4, a.s, a.s_rcp, wave * D + d0);
                            *reinterpret_cast<uint32_t*>(codes + (bb * 16 + tq) * CROW + wave * D + d0) = tq_codes<false, SAT8_>(x4, gq, csum);
                        }
                    })
                    tq_publish_sum(csum, ex_sum + bb * 256, wave, lane);
                }
            }
            tq_lds_barrier();                      // (not last: only the next sample's V rows become visible)
            if (!last) continue;
            const int kch = a.Kp / 16, cch = C / 16;
            for (int bb = 0; bb < a.B; ++bb) {
                for (int c = tid; c < 16 * kch; c += nthr) {
                    const int t = c / kch, ch = c - t * kch;
                    if (t < a.T) {
                        const long grow = ((long)bb * a.T + t) * a.S + s;
                        const int4v val = ch < cch ? *reinterpret_cast<const int4v*>(codes + (bb * 16 + t) * CROW + ch * 16) : int4v{0, 0, 0, 0};
                        *reinterpret_cast<int4v*>(a.xq + grow * a.Kp + ch * 16) = val;
                    }
                }
                if (tid < 16 && tq < a.T)
                    rq_write_row(a.sx, a.zx, a.R, nullptr, (size_t)(((long)bb * a.T + tq) * a.S + s), gq.g.delta, gq.g.zp,
                                 tq_collect_sum(ex_sum + bb * 256, H, tq), C, gq.wd.cx);
            }
            continue;
        }
        // ---- O^T[dim 16*dt + 4*g4 + r][query tq] = V^T P^T: P^T is the accumulator layout of S^T already.
        // this lane: token tq, dims 16*dt + 4*g4 + r, rounded to fp16 like the stored tensor
        // (float4v, and x4 copies at the encode: in this shape hipcc selects v_fma_mixlo_f16 - ONE rounding of o4 * inv_p to
        //  fp16 - for the same 2 / 6 / 8 of the lane's values at D = 32 / 64 / 72 of the dynamic form as in the written-out
        //  kernel, and the two-rounding v_mul + v_cvt_pk_f16_f32 for all others; as float[KS][4] every value rounds twice and
        //  ~1e-5 of the fp16 outputs move by an ulp: profiles/refactor_temporal_steps.md)
        float4v ov[KS];
#pragma unroll
        for (int dt = 0; dt < KS; ++dt) {
            const half4 vf = tq_vt_frag(vs + (4 * g4 + (tq >> 2)) * RS + (dt * 16 + 4 * (tq & 3)) * 2);
            const float4v o4 = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[0], float4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[dt][r] = (float)(half_t)(o4[r] * inv_p);
        }
        if (a.o && tq < a.T)                       // optional fp16 copy (tests, callers that need both)
            tq_store_o<D>(a.o + (((long)b * a.T + tq) * a.S + s) * C + wave * D, ov, g4);
        // the quantizer's input, and this head's part of the row statistics
        [[maybe_unused]] float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
        for (int dt = 0; dt < KS; ++dt) {
            const int d0 = dt * 16 + 4 * g4;
            if (d0 < D) {
                tq_div_s(ov[dt], a.s, a.s_rcp, wave * D + d0);
                if constexpr (!ST) tq_minmax4(ov[dt], vmin, vmax);
            }
        }
        if constexpr (!ST) tq_publish_minmax(vmin, vmax, ex_min, ex_max, wave, lane);
        tq_lds_barrier();                          // row statistics visible; every wave is done with the q | k | v tiles
                                                   // (ST: nothing to publish, but store_qkv below reuses the V tile)
        if (has_next) {
            store_qkv(tx);                         // next position's V rows (visible after the barrier below) ...
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {     // ... its K / Q operands move into the current set ...
                kfc[ks] = kfn[ks];
                qfc[ks] = qfn[ks];
            }
            if (tq_next_pos<SH>(npos_next, G, a.B) < npos) load_qkv(tq_next_pos<SH>(npos_next, G, a.B), tx);   // ... and the position after it is requested
        }
        if constexpr (!ST) gq = tq_row_grid(ex_min, ex_max, H, tq, tid < 16 && tq < a.T, a.status);
        uint32_t csum = 0;
        RQ_BY_WIDTH(gq.wd.qmax, _Pragma("unroll") for (int dt = 0; dt < KS; ++dt) {
            const int d0 = dt * 16 + 4 * g4;
            if (d0 < D) {
                const float x4[4] = {ov[dt][0], ov[dt][1], ov[dt][2], ov[dt][3]};
                *reinterpret_cast<uint32_t*>(codes + tq * CROW + wave * D + d0) = tq_codes<ST, SAT8_>(x4, gq, csum);
            }
        })
        tq_publish_sum(csum, ex_sum, wave, lane);
        tq_lds_barrier();
        // ---- codes out as whole 16-byte chunks (pad columns [C, Kp) zeroed like the row quantizers do); the next
        //      iteration touches codes / ex_sum only after its own first barrier, which every thread reaches after this
        const int kch = a.Kp / 16, cch = C / 16;
        for (int c = tid; c < 16 * kch; c += nthr) {
            const int t = c / kch, ch = c - t * kch;
            if (t < a.T) {
                const long grow = ((long)b * a.T + t) * a.S + s;
                const int4v val = ch < cch ? *reinterpret_cast<const int4v*>(codes + t * CROW + ch * 16) : int4v{0, 0, 0, 0};
                *reinterpret_cast<int4v*>(a.xq + grow * a.Kp + ch * 16) = val;
            }
        }
        if (tid < 16 && tq < a.T)
            rq_write_row(a.sx, a.zx, a.R, nullptr, (size_t)(((long)b * a.T + tq) * a.S + s), gq.g.delta, gq.g.zp,
                         tq_collect_sum(ex_sum, H, tq), C, gq.wd.cx);
    }
}

// ---------------------------------------------------------------------------
// attn_temporal_quant2_kernel (round 6): the kernel above for H = 16 heads with its per-position INSTRUCTION count cut.
// Ablations of the kernel above (profiles/r06_experiments.md 6: 38.8 us; loads only 11.7 us; compute + stores only 27.9 us)
// showed it bound by its own instruction stream - ~1300 static instructions per position and wave, 16 waves in lockstep
// between two barriers - not by the 132 MB it moves.  Here:
//   * every global access is SGPR base (per position, scalar arithmetic) + a 32-bit per-lane offset computed ONCE (the kernel
//     above recomputed five 64-bit addresses per position with v_mad_u64_u32 / v_mul_lo_u32 chains to save registers);
//   * the K / Q operand registers are requested again right behind the QK^T MFMAs that consume them - one set, no copy of
//     a "next" set into a "current" one (24 registers and 24 moves per position less: the spill of the kernel above is gone);
//   * 1 / sum(p) is v_rcp_f32 (1 ulp; the fp16 rounding that follows is 2^13 times coarser) instead of an IEEE division;
//   (the cross-row reductions over the four 16-lane rows of a wave as v_permlane16_swap / v_permlane32_swap + one VALU
//    instruction each instead of ds_bpermute round trips - ten dependent LDS latencies per position - came with this kernel
//    too; they are the shared steps' reductions now, so the kernel above has them as well)
//   * the chunk -> (row, column) decomposition of the code stores is per-lane state, not a division per chunk.
// Codes / grids / row sums remain exact functions of the kernel's own fp16 output (bit-identical to vq_rowquant of it: the
// shared steps of attn_rowquant.h, tested).
// ---------------------------------------------------------------------------
template <int D, class A = TempQArgs>
__global__ __launch_bounds__(1024) void attn_temporal_quant2_kernel(A a) {
    constexpr bool ST = std::is_same<A, TempQSArgs>::value;   // the static-grid form (attn_rowquant.h)
    constexpr bool SH = std::is_same<A, TempQPArgs>::value;   // the shared-grid form: as in the kernel above
    constexpr int NCB = SH ? 2 : 1;
    constexpr int H = 16, C = H * D, NTHR = 64 * H;
    constexpr int KS = (D + 15) / 16, KS2 = (D + 31) / 32;
    constexpr int RS = C * 2 + 16, TILE = 16 * RS, RCH = C / 8, CROW = C + 16;
    constexpr int NIT = (16 * RCH + NTHR - 1) / NTHR;      // V chunks per thread (3 at D = 72)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // = head
    const int tq = lane & 15, g4 = lane >> 4;
    uint8_t* codes = smem + TILE + (SH ? 4 * 1024 : 0);   // (the LDS maps of the kernel above)
    float* ex_min = reinterpret_cast<float*>(SH ? smem + TILE : codes + 16 * CROW);
    float* ex_max = ex_min + 256;
    int* ex_sum = reinterpret_cast<int*>(ex_max + 256);
    [[maybe_unused]] uint8_t* park = codes + NCB * 16 * CROW;
    const int npos = a.S * a.B, G = (int)gridDim.x;
    const unsigned tstride = (unsigned)a.S * (unsigned)a.ld_in * 2u;          // bytes between the rows t, t + 1 of a position

    // ---- per-lane state, computed once -----------------------------------------------------------------------------
    unsigned vgo[NIT], vlo[NIT];                           // V chunk: global byte offset from the position's base, LDS offset
    bool vok[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int c = tid + i * NTHR;
        const int t = c / RCH, ch = c - t * RCH;
        vok[i] = c < 16 * RCH && t < a.T;
        vgo[i] = (unsigned)t * tstride + (unsigned)ch * 16u;
        vlo[i] = (unsigned)(t * RS + ch * 16);
    }
    const bool kq_row = tq < a.T;
    const unsigned kqo = (unsigned)(kq_row ? tq : 0) * tstride + (unsigned)(wave * D + 8 * g4) * 2u;   // + 64 bytes per k-step
    const int kch = a.Kp / 16, cch = C / 16;
    constexpr int NCI = 2;                                 // code chunks per thread: 16 rows x Kp / 16 <= 2048 (Kp <= 2048)
    unsigned cgo[NCI], clo[NCI];
    bool cok[NCI], cpad[NCI];
#pragma unroll
    for (int j = 0; j < NCI; ++j) {
        const int c = tid + j * NTHR;
        const int t = c / kch, ch = c - t * kch;
        cok[j] = c < 16 * kch && t < a.T;
        cpad[j] = ch >= cch;
        cgo[j] = (unsigned)t * (unsigned)a.S * (unsigned)a.Kp + (unsigned)ch * 16u;
        clo[j] = (unsigned)(t * CROW + ch * 16);
    }
    const uint8_t* vs = smem + wave * D * 2;
    const unsigned vtro = (unsigned)((4 * g4 + (tq >> 2)) * RS + 4 * (tq & 3) * 2);   // transpose-read lane offset (+ 32 bytes per dim tile)

    int4v vals[NIT];
    half8 kf[KS2], qf[KS2];
    auto row_of = [&](int b, int s) -> size_t { return ((size_t)b * a.T * a.S + s); };
    auto base_of = [&](int pos) -> size_t {                // first row (t = 0) of the position, in ELEMENTS of ld_in rows
        if constexpr (SH) return row_of(pos & (a.B - 1), pos >> (a.B - 1));
        else return row_of(pos / a.S, pos % a.S);
    };
    auto load_v = [&](int pos) {
        const uint8_t* vb = reinterpret_cast<const uint8_t*>(a.v) + base_of(pos) * (size_t)a.ld_in * 2;
#pragma unroll
        for (int i = 0; i < NIT; ++i)
            if (vok[i]) vals[i] = *reinterpret_cast<const int4v*>(vb + vgo[i]);   // (lanes without a chunk keep their zeros)
    };
    auto load_kq = [&](int pos) {
        const size_t bo = base_of(pos) * (size_t)a.ld_in * 2;
        const uint8_t* kb = reinterpret_cast<const uint8_t*>(a.k) + bo;
        const uint8_t* qb = reinterpret_cast<const uint8_t*>(a.q) + bo;
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks)
            if (ks * 32 + 8 * g4 < D && kq_row) {          // (dims >= D / rows >= T: the registers keep the zeros set below)
                kf[ks] = *reinterpret_cast<const half8*>(kb + kqo + ks * 64);
                qf[ks] = *reinterpret_cast<const half8*>(qb + kqo + ks * 64);
            }
    };
#pragma unroll
    for (int i = 0; i < NIT; ++i) vals[i] = int4v{0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < KS2; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            kf[ks][e] = (half_t)0.f;
            qf[ks][e] = (half_t)0.f;
        }
    auto store_v = [&]() {
#pragma unroll
        for (int i = 0; i < NIT; ++i)
            if (tid + i * NTHR < 16 * RCH) *reinterpret_cast<int4v*>(smem + vlo[i]) = vals[i];
    };

    TqGrid gq;                                             // ST: the calibrated grid; else every row's own, behind its statistics
    if constexpr (ST) gq = tq_static(a.delta, a.zp, a.n_bits);

    int pos = SH ? blockIdx.x * a.B : blockIdx.x;
    if (pos >= npos) return;
    load_v(pos);
    load_kq(pos);
    store_v();
    __syncthreads();
    if (tq_next_pos<SH>(pos, G, a.B) < npos) load_v(tq_next_pos<SH>(pos, G, a.B));
    [[maybe_unused]] float shmin = INFINITY, shmax = -INFINITY;   // SH: a token's extremes, carried from one sample to the next
    for (int pos_n; pos < npos; pos = pos_n) {
        pos_n = tq_next_pos<SH>(pos, G, a.B);
        const bool has_next = pos_n < npos;                // workgroup-uniform
        const size_t row0 = base_of(pos);
        [[maybe_unused]] const int b = SH ? pos & (a.B - 1) : 0;
        [[maybe_unused]] const bool last = !SH || b == a.B - 1;   // SH: the position's statistics are complete

        // ---- S^T = K Q^T (16 x 16 per head), then the operand registers are requested again for the next position
        float4v sc[1] = {{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) sc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[ks], qf[ks], sc[0], 0, 0, 0);
        if (has_next) load_kq(pos_n);
        half4 pf[1];
        const float psum = tq_softmax16<1>(sc, g4, a.T, a.c, pf);
        const float inv_p = psum > 0.f ? __builtin_amdgcn_rcpf(psum) : 0.f;

        if constexpr (SH) {
            // the shared-grid form: a dim tile at a time - round, store, park, and this head's part of the token's extremes
            // over the samples so far (the 20 output registers of the dynamic form are not held across the barrier)
            half_t* orow = a.o + (row0 + (size_t)tq * a.S) * C + wave * D;
#pragma unroll
            for (int dt = 0; dt < KS; ++dt) {
                const half4 vf = tq_vt_frag(vs + vtro + dt * 32);
                const float4v o4 = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[0], float4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                const half4 oh = tq_round_o<false>(o4, inv_p, dt);
                const int d0 = dt * 16 + 4 * g4;
                if (d0 < D) {
                    if (a.o && tq < a.T) *reinterpret_cast<half4*>(orow + d0) = oh;
                    tq_park(park + b * KS * NTHR * 8, NTHR, tid, dt, oh);
                    float x4[4] = {(float)oh[0], (float)oh[1], (float)oh[2], (float)oh[3]};
                    tq_div_s(x4, a.s, a.s_rcp, wave * D + d0);
                    tq_minmax4(x4, shmin, shmax);
                }
            }
            if (last) {
                tq_publish_minmax(shmin, shmax, ex_min, ex_max, wave, lane);
                shmin = INFINITY, shmax = -INFINITY;
            }
            tq_lds_barrier();                                // row statistics visible; every wave is done with the V tile
            if (has_next) {
                store_v();                                   // the next sample's or position's V rows (visible after the barrier below)
                if (tq_next_pos<SH>(pos_n, G, a.B) < npos) load_v(tq_next_pos<SH>(pos_n, G, a.B));
            }
            if (last) {                                      // one grid for the token's rows of all samples, each from where it was parked
                gq = tq_row_grid(ex_min, ex_max, H, tq, tid < 16 && tq < a.T, a.status, a.n_bits);
                for (int bb = 0; bb < a.B; ++bb) {
                    uint32_t csum = 0;
                    RQ_BY_WIDTH(gq.wd.qmax, _Pragma("unroll") for (int dt = 0; dt < KS; ++dt) {
                        const int d0 = dt * 16 + 4 * g4;
                        if (d0 < D) {
                            float x4[4];
                            tq_unpark(park + bb * KS * NTHR * 8, NTHR, tid, dt, x4);
                            tq_div_s(x4, a.s, a.s_rcp, wave * D + d0);
                            *reinterpret_cast<uint32_t*>(codes + (bb * 16 + tq) * CROW + wave * D + d0) = tq_codes<false, SAT8_>(x4, gq, csum);
                        }
                    })
                    tq_publish_sum(csum, ex_sum + bb * 256, wave, lane);
                }
            }
            tq_lds_barrier();                                // (not last: only the next sample's V rows become visible)
            if (!last) continue;
            for (int bb = 0; bb < a.B; ++bb) {
                const size_t rowb = row_of(bb, pos >> (a.B - 1));
                uint8_t* xb = reinterpret_cast<uint8_t*>(a.xq) + rowb * (size_t)a.Kp;
#pragma unroll
                for (int j = 0; j < NCI; ++j)
                    if (cok[j]) {
                        const int4v val = cpad[j] ? int4v{0, 0, 0, 0} : *reinterpret_cast<const int4v*>(codes + bb * 16 * CROW + clo[j]);
                        *reinterpret_cast<int4v*>(xb + cgo[j]) = val;
                    }
                if (tid < 16 && tq < a.T)
                    rq_write_row(a.sx, a.zx, a.R, nullptr, rowb + (size_t)tq * a.S, gq.g.delta, gq.g.zp,
                                 tq_collect_sum(ex_sum + bb * 256, H, tq), C, gq.wd.cx);
            }
            continue;
        }
        // ---- O^T = V^T P^T, rounded to fp16 as the stored tensor is
        float ov[KS][4];
#pragma unroll
        for (int dt = 0; dt < KS; ++dt) {
            const half4 vf = tq_vt_frag(vs + vtro + dt * 32);
            const float4v o4 = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[0], float4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[dt][r] = (float)(half_t)(o4[r] * inv_p);
        }
        if (a.o && tq < a.T)                               // optional fp16 copy (tests, callers that need both)
            tq_store_o<D>(a.o + (row0 + (size_t)tq * a.S) * C + wave * D, ov, g4);
        // the quantizer's input, and this head's part of the row statistics
        [[maybe_unused]] float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
        for (int dt = 0; dt < KS; ++dt) {
            const int d0 = dt * 16 + 4 * g4;
            if (d0 < D) {
                tq_div_s(ov[dt], a.s, a.s_rcp, wave * D + d0);
                if constexpr (!ST) tq_minmax4(ov[dt], vmin, vmax);
            }
        }
        if constexpr (!ST) tq_publish_minmax(vmin, vmax, ex_min, ex_max, wave, lane);
        tq_lds_barrier();                                    // row statistics visible; every wave is done with the V tile
                                                             // (ST: nothing to publish, but store_v below reuses the tile)
        if (has_next) {
            store_v();                                       // the next position's V rows (visible after the barrier below)
            if (tq_next_pos<SH>(pos_n, G, a.B) < npos) load_v(tq_next_pos<SH>(pos_n, G, a.B));
        }
        if constexpr (!ST) gq = tq_row_grid(ex_min, ex_max, H, tq, tid < 16 && tq < a.T, a.status);
        uint32_t csum = 0;
        RQ_BY_WIDTH(gq.wd.qmax, _Pragma("unroll") for (int dt = 0; dt < KS; ++dt) {
            const int d0 = dt * 16 + 4 * g4;
            if (d0 < D) *reinterpret_cast<uint32_t*>(codes + tq * CROW + wave * D + d0) = tq_codes<ST, SAT8_>(ov[dt], gq, csum);
        })
        tq_publish_sum(csum, ex_sum, wave, lane);
        tq_lds_barrier();
        // ---- codes out as whole 16-byte chunks (pad columns [C, Kp) zeroed like the row quantizers do)
        {
            uint8_t* xb = reinterpret_cast<uint8_t*>(a.xq) + row0 * (size_t)a.Kp;
#pragma unroll
            for (int j = 0; j < NCI; ++j)
                if (cok[j]) {
                    const int4v val = cpad[j] ? int4v{0, 0, 0, 0} : *reinterpret_cast<const int4v*>(codes + clo[j]);
                    *reinterpret_cast<int4v*>(xb + cgo[j]) = val;
                }
        }
        if (tid < 16 && tq < a.T)
            rq_write_row(a.sx, a.zx, a.R, nullptr, row0 + (size_t)tq * a.S, gq.g.delta, gq.g.zp, tq_collect_sum(ex_sum, H, tq), C,
                         gq.wd.cx);
    }
}

// ---------------------------------------------------------------------------
// attn_temporal_long_kernel: temporal attention for 17 <= T <= 64 frames (OpenSORA 64x512x512: stdit.py:112-118), with the
// optional per-token 8-bit quantizer of attn_temp.proj (stdit_quant_layer.py:161-166) fused as in the kernels above.
// One persistent workgroup walks spatial positions (b, s); one wave per head (H <= 16), 64 * H threads.
//   * LDS: at T = 64 one position's q | k | v is 442 KB, so nothing is staged for the whole workgroup.  Each wave stages its
//     OWN head's V rows [64 t][D] (row stride 2 D bytes, rows t >= T zeroed) for the ds_read_b64_tr_b16 transpose read of
//     the V^T operand; no other wave reads them, so no barrier guards the tile.  H * 64 * 2 D bytes (147 456 B at H = 16,
//     D = 72) + 64 B of zeroed tail (the dims 72..79 of the last transpose read at D = 72, which land in O^T rows >= D that
//     are discarded) + 3 KB of cross-wave row statistics = 150 592 B:
//     one workgroup per CU.
//   * Q and K operands of S^T = K Q^T come straight from global memory in 16x16x32 operand form (16-byte loads of the
//     head's 2 D-byte row slice), both per 16-query tile: K of the 4 key tiles is 48 VGPRs at D = 72 and is read again
//     for every query tile (from L2 after the first) - kept for the whole position it made the kernel spill.
//   * queries in tiles of 16 (registers: a full 64 x 64 score tile plus O^T for 64 queries does not fit 128 VGPRs):
//     S^T [64 keys][16 queries] in 4 accumulators, keys >= T masked, softmax lane-local over 16 keys + the permlane row
//     reductions, O^T = V^T P^T over 4 key steps, rounded to fp16 as the stored tensor.  Query tiles wholly past T are
//     skipped, so are key tiles.
//   * with codes (B == 1): the tile's row min / max and code sums are combined over the waves through LDS (two barriers
//     per tile), grid and codes are the vq_row_grid / rq_round_group arithmetic of vq_rowquant (bit-identical to it on
//     the kernel's own fp16 output), and the codes leave straight from registers: 4 bytes per lane, 16 contiguous bytes
//     per row and 16-lane group.
// ---------------------------------------------------------------------------
// A = TempQSArgs: the static-grid form ST (attn_rowquant.h; any B).  With no row statistics to publish a tile has ONE barrier, so the
// code sums of successive tiles alternate between two [wave][16] areas (ex_sum and the idle ex_max): wave 0 may still
// read tile n's sums while the others write tile n + 1's, and tile n + 2 writes behind the barrier of tile n + 1.
template <int D, class A = TempQArgs>
__global__ __launch_bounds__(1024) void attn_temporal_long_kernel(A a) {
    constexpr bool ST = std::is_same<A, TempQSArgs>::value;
    constexpr int KS = (D + 15) / 16, KS2 = (D + 31) / 32, CHD = D / 8;
    constexpr int RSV = D * 2, VT = 64 * RSV;      // V tile of one head: row stride, bytes
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // = head
    const int tq = lane & 15, g4 = lane >> 4;
    const int H = a.H, C = H * D, T = a.T, nthr = 64 * H;
    uint8_t* vs = smem + wave * VT;
    float* ex_min = reinterpret_cast<float*>(smem + H * VT + 64);
    float* ex_max = ex_min + 256;
    int* ex_sum = reinterpret_cast<int*>(ex_max + 256);
    const int npos = a.S * a.B;
    const int nt = (T + 15) >> 4;                  // 16-row tiles holding rows < T (keys and queries)
    const unsigned tstride = (unsigned)a.S * (unsigned)a.ld_in * 2u;          // bytes between the rows t, t + 1 of a position
    const bool quant = ST || a.xq != nullptr;
    TqGrid gq;                                     // ST: the calibrated grid; else every row's own, behind its statistics
    [[maybe_unused]] int par = 0;                  // ST: which of the two code-sum areas this tile uses
    if constexpr (ST) gq = tq_static(a.delta, a.zp, a.n_bits);
    const int npad = a.Kp / 16 - C / 16;           // 16-byte pad chunks [C, Kp) of a code row
    const unsigned vtro = (unsigned)((4 * g4 + (tq >> 2)) * RSV + 4 * (tq & 3) * 2);   // transpose-read lane offset
    const unsigned kqo = (unsigned)(wave * D + 8 * g4) * 2u;                           // + 64 bytes per k-step
    // the LDS tail behind the last head's V tile: the dt = 4 transpose read at D = 72 covers dims 72..79, which for the
    // last key row of the last head lie in it.  Those values only reach O^T rows >= D (never stored, never counted);
    // zeroed once so that they are defined.
    if (tid < 4) *reinterpret_cast<int4v*>(smem + H * VT + 16 * tid) = int4v{0, 0, 0, 0};
    __syncthreads();

    for (int pos = blockIdx.x; pos < npos; pos += gridDim.x) {
        const int s = pos % a.S, b = pos / a.S;
        const size_t row0 = (size_t)b * T * a.S + s;                          // row (b, t = 0, s)
        const size_t bo = row0 * (size_t)a.ld_in * 2;
        const uint8_t* qb = reinterpret_cast<const uint8_t*>(a.q) + bo;
        const uint8_t* kb = reinterpret_cast<const uint8_t*>(a.k) + bo;
        const uint8_t* vb = reinterpret_cast<const uint8_t*>(a.v) + bo + wave * D * 2;

        // ---- this head's V rows (chunk c = row c / CHD, 16-byte piece c % CHD)
        // (lx: an opaque per-position copy of the lane id, so that the chunk offsets are recomputed per position instead
        //  of being hoisted out of the loop - nine 64-bit offsets kept live made the D = 72 kernel spill)
        int lx = lane;
        asm volatile("" : "+v"(lx));
        int4v vals[CHD];
#pragma unroll
        for (int i = 0; i < CHD; ++i) {
            const int c = lx + 64 * i, t = c / CHD, ch = c - t * CHD;
            vals[i] = int4v{0, 0, 0, 0};
            if (t < T) vals[i] = *reinterpret_cast<const int4v*>(vb + (unsigned)t * tstride + ch * 16);
        }
        // (the wave's transpose reads of the previous position were consumed by MFMAs before this point; LDS operations of
        //  one wave complete in order)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < CHD; ++i) *reinterpret_cast<int4v*>(vs + (lane + 64 * i) * 16) = vals[i];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();

        for (int qt = 0; qt < nt; ++qt) {          // workgroup-uniform
            const int tr = 16 * qt + tq;           // this lane's query row
            const bool qrow = tr < T;
            half8 qf[KS2];
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[ks][e] = (half_t)0.f;
                if (qrow && ks * 32 + 8 * g4 < D)
                    qf[ks] = *reinterpret_cast<const half8*>(qb + (unsigned)tr * tstride + kqo + ks * 64);
            }
            // ---- S^T[key 16 kt + 4 g4 + r][query tq] = K Q^T; the K operands are read per query tile (from L2 after the
            //      first): held for the whole position, 48 VGPRs at D = 72, they made the kernel spill
            float4v sc[4];
            float mloc = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                sc[kt] = float4v{0.f, 0.f, 0.f, 0.f};
                if (kt < nt) {
                    const int t = 16 * kt + tq;
                    half8 kf[KS2];
#pragma unroll
                    for (int ks = 0; ks < KS2; ++ks) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) kf[ks][e] = (half_t)0.f;
                        if (t < T && ks * 32 + 8 * g4 < D)
                            kf[ks] = *reinterpret_cast<const half8*>(kb + (unsigned)t * tstride + kqo + ks * 64);
                    }
#pragma unroll
                    for (int ks = 0; ks < KS2; ++ks)
                        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[ks], qf[ks], sc[kt], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (16 * kt + 4 * g4 + r >= T) sc[kt][r] = -INFINITY;
                    mloc = fmaxf(mloc, sc[kt][r]);
                }
            }
            // (the softmax is written out in this kernel - tq_softmax16<4> of attn_rowquant.h is the same arithmetic: with the
            //  mask and maximum of all four tiles behind the conditional MFMA blocks instead of between them, the static form
            //  at D = 72 has 2393 instructions against 2345 and its T = 64, S = 1024 time left the band of the written-out
            //  kernel: median 199.7 us against 196.4 .. 199.6 - profiles/refactor_temporal_steps.md)
            mloc = tq_xor32(tq_xor16(mloc, true), true);
            const float m_use = (mloc == -INFINITY) ? 0.f : mloc;
            float psum = 0.f;
            half4 pf[4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f((sc[kt][r] - m_use) * a.c);
                    psum += p;
                    pf[kt][r] = (half_t)p;
                }
            psum = tq_sum4rows(psum);
            const float inv_p = psum > 0.f ? __builtin_amdgcn_rcpf(psum) : 0.f;

            // ---- O^T[dim 16 dt + 4 g4 + r][query tq] = V^T P^T over the key tiles, rounded to fp16 as the stored tensor
            half4 ov[KS];                          // (fp16: the quantizer's x / s is recomputed where it is needed)
#pragma unroll
            for (int dt = 0; dt < KS; ++dt) {
                float4v o4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
                    if (kt < nt) o4 = __builtin_amdgcn_mfma_f32_16x16x16f16(tq_vt_frag(vs + kt * 16 * RSV + vtro + dt * 32), pf[kt], o4, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[dt][r] = (half_t)(o4[r] * inv_p);
            }
            const size_t grow = row0 + (size_t)tr * a.S;
            if (a.o && qrow) tq_store_o<D>(a.o + grow * a.ld_out + wave * D, ov, g4);
            if (!quant) continue;                  // kernel-uniform

            // ---- quantizer of the consuming Linear on the fp16 output (x / s first when it has a smoothing vector)
            auto qin = [&](int dt, float (&x4)[4]) {
#pragma unroll
                for (int r = 0; r < 4; ++r) x4[r] = (float)ov[dt][r];
                tq_div_s(x4, a.s, a.s_rcp, wave * D + dt * 16 + 4 * g4);
            };
            int* exs = ex_sum;                     // this tile's code sums
            if constexpr (ST) {
                exs = ex_sum - 256 * par;          // (ex_max's area: nothing else uses it here)
                par ^= 1;
            } else {
                float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
                for (int dt = 0; dt < KS; ++dt)
                    if (dt * 16 + 4 * g4 < D) {
                        float x4[4];
                        qin(dt, x4);
                        tq_minmax4(x4, vmin, vmax);
                    }
                tq_publish_minmax(vmin, vmax, ex_min, ex_max, wave, lane);
                tq_lds_barrier();                  // the tile's per-head row statistics are visible
                gq = tq_row_grid(ex_min, ex_max, H, tq, tid < 16 && qrow, a.status);
            }
            // codes leave straight from the registers
            uint8_t* xrow = reinterpret_cast<uint8_t*>(a.xq) + grow * (size_t)a.Kp + wave * D;
            uint32_t csum = 0;
            RQ_BY_WIDTH(gq.wd.qmax, _Pragma("unroll") for (int dt = 0; dt < KS; ++dt) {
                const int d0 = dt * 16 + 4 * g4;
                if (d0 < D) {
                    float x4[4];
                    qin(dt, x4);
                    const uint32_t pk = tq_codes<ST, SAT8_>(x4, gq, csum);
                    if (qrow) *reinterpret_cast<uint32_t*>(xrow + d0) = pk;
                }
            })
            tq_publish_sum(csum, exs, wave, lane);
            tq_lds_barrier();                      // code sums visible; every wave has read ex_min / ex_max of this tile
            if (tid < 16 && qrow)
                rq_write_row(a.sx, a.zx, a.R, nullptr, grow, gq.g.delta, gq.g.zp, tq_collect_sum(exs, H, tq), C, gq.wd.cx);
            for (int c = tid; c < 16 * npad; c += nthr) {       // pad columns [C, Kp) zeroed like the row quantizers do
                const int t = c / npad, ch = c - t * npad;
                if (16 * qt + t < T) {
                    int8_t* prow = a.xq + (row0 + (size_t)(16 * qt + t) * a.S) * (size_t)a.Kp + C;
                    *reinterpret_cast<int4v*>(prow + ch * 16) = int4v{0, 0, 0, 0};
                }
            }
            // (the next tile writes ex_min / ex_max only after this barrier and ex_sum only after its first one, which
            //  the lanes reading ex_sum above reach after reading it)
        }
    }
}

// ---------------------------------------------------------------------------
// attn_fwd8_kernel: second generation of the flash kernel above for long query sequences.
//   * 8 waves (256 queries) share one K/V tile: half the staging work and LDS traffic per query;
//   * V is staged DIM-major: Vt[d][32 key pairs] dwords, pair order permuted so that the four dwords an
//     MFMA A-operand lane needs (keys {4g..4g+3} and {8+4g..8+4g+3} of a 16-key step: the order in which
//     S^T leaves the first MFMA) are one 16-byte slot -> ONE ds_read_b128 with an immediate-free per-lane
//     address per MFMA (the pair-major image needed 4 ds_read_b32 + address arithmetic: 48 reads and 75
//     v_add_u32 per key tile).  Row stride 144 B (9 slots: conflict-free b128 reads across dims); the slot
//     index is rotated by d >> 4 so that the 4-byte staging writes of different 8-dim chunks spread over
//     the banks; row D is all {1.0, 1.0}: the P.V MFMA of that row yields the softmax row sums;
//   * the partner exchange of the key pair (lanes c, c^1) is a DPP quad_perm, not ds_bpermute;
//   * deferred rescale: the running max (and O) is updated only when some lane's tile max exceeds it by
//     more than 8 in the exp2 domain, so P <= 2^8 in between (fp16-safe) and the 48-register rescale of
//     O^T runs on the first tiles only.
// ---------------------------------------------------------------------------
template <int D, int NW>
struct Att8Cfg {
    static constexpr int KS = (D + 15) / 16;
    static constexpr int DT = (D + 32) / 32;
    static constexpr int CHD = D / 8;
    static constexpr int KROW = (CHD | 1) * 16;
    static constexpr int VROWB = 144;
    static constexpr int KTILE = 64 * KROW;
    static constexpr int VTILE = (D + 1) * VROWB;
    static constexpr int LDS = 2 * (KTILE + VTILE);
    static constexpr int KCH = 64 * CHD;
    static constexpr int NTH = 64 * NW;
    static constexpr int KPT = (KCH + NTH - 1) / NTH;
    static_assert(DT * 32 > D, "needs a spare O^T row for the row sums");
};

template <int D, int NW>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_fwd8_kernel(AttnArgs a) {
    using C = Att8Cfg<D, NW>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, l31 = lane & 31;
    int qt, h, seq;
    if (!attn_xcd_map(a, 32 * NW, qt, h, seq)) return;
    const half_t* kbase;
    const half_t* vbase;
    const int kv_len = attn_kv_base<D>(a, seq, h, kbase, vbase);
    const int qi = qt * (32 * NW) + wave * 32 + l31;
    const bool q_ok = qi < a.Lq;
    half8 qf[C::KS];
    float16v oacc[C::DT];
    float m_run = -INFINITY;
    attn_q_frags<D>(a.q + (long)seq * a.q_seq_stride + (long)(q_ok ? qi : a.Lq - 1) * a.q_tok_stride + h * D, g, qf);
    attn_zero(oacc);

    // V^T fragment addresses: lane = output dim d (row D = the ones row; rows above it are clamped, unused)
    int vaddr[C::DT][4];
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt) {
        const int d = dt * 32 + l31 <= D ? dt * 32 + l31 : D;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) vaddr[dt][kk] = d * C::VROWB + (((2 * kk + g + (d >> 4)) & 7) << 4);
    }

    const int nkt = (kv_len + 63) / 64;
    // two staging register sets: tile t travels in set t & 1 and is loaded TWO tiles ahead
    int4v krA[C::KPT], vrA[C::KPT], krB[C::KPT], vrB[C::KPT];
    // Per-thread staging geometry, computed ONCE (the divisions by CHD and the swizzles cost ~100 VALU per tile
    // when redone in the loop).  Chunk c of a tile: K row c / CHD, 16-byte piece c % CHD; V: lanes c, c^1 hold
    // the same 8-dim piece of keys 2p, 2p+1 (p = (c >> 1) / CHD).  The ragged last pass (KCH % NTH chunks) is
    // taken by a FIXED set of waves here (rotating it would make the geometry tile-dependent).
    bool act[C::KPT];
    int krow[C::KPT], vrow[C::KPT];                   // key row inside the tile (K: row; V: 2p + odd)
    long kgo[C::KPT], vgo[C::KPT];                    // global element offsets of the chunk inside a tile
    int kdst[C::KPT], vdst[C::KPT];                   // LDS byte offsets inside a buffer
#pragma unroll
    for (int i = 0; i < C::KPT; ++i) {
        const int c = tid + i * C::NTH;
        act[i] = c < C::KCH;
        const int cc = act[i] ? c : 0;
        krow[i] = cc / C::CHD;
        kgo[i] = (long)krow[i] * a.kv_tok_stride + (cc % C::CHD) * 8;
        kdst[i] = krow[i] * C::KROW + (cc % C::CHD) * 16;
        const int odd = cc & 1, m = cc >> 1, p = m / C::CHD, dch = m % C::CHD;
        vrow[i] = 2 * p + odd;
        vgo[i] = (long)vrow[i] * a.kv_tok_stride + dch * 8;
        const int q = 2 * (p >> 3) + ((p >> 1) & 1), idx = (p & 1) + 2 * ((p >> 2) & 1);
        vdst[i] = (8 * dch + 4 * odd) * C::VROWB + ((((q + (dch >> 1)) & 7) << 2) + idx) * 4;
    }
    const bool odd_lane = tid & 1;                     // c & 1 == tid & 1 for every pass (NTH is even)
    auto load_tile = [&](int kt, int4v (&kr)[C::KPT], int4v (&vr)[C::KPT]) {
        const long t0 = (long)kt * 64 * a.kv_tok_stride;
        const bool full = kt * 64 + 64 <= kv_len;      // wave-uniform: no clamping on full tiles
#pragma unroll
        for (int i = 0; i < C::KPT; ++i) {
            if (act[i]) {
                if (full) {
                    kr[i] = *reinterpret_cast<const int4v*>(kbase + t0 + kgo[i]);
                    vr[i] = *reinterpret_cast<const int4v*>(vbase + t0 + vgo[i]);
                } else {
                    const int kk_ = kt * 64 + krow[i] < kv_len ? krow[i] : kv_len - 1 - kt * 64;
                    const int vk_ = kt * 64 + vrow[i] < kv_len ? vrow[i] : kv_len - 1 - kt * 64;
                    kr[i] = *reinterpret_cast<const int4v*>(kbase + t0 + kgo[i] + (long)(kk_ - krow[i]) * a.kv_tok_stride);
                    vr[i] = *reinterpret_cast<const int4v*>(vbase + t0 + vgo[i] + (long)(vk_ - vrow[i]) * a.kv_tok_stride);
                }
            }
        }
    };
    auto store_tile = [&](int buf, int4v (&kr)[C::KPT], int4v (&vr)[C::KPT]) {
        uint8_t* kt_ = smem + buf * C::KTILE;
        uint8_t* vt_ = smem + 2 * C::KTILE + buf * C::VTILE;
#pragma unroll
        for (int i = 0; i < C::KPT; ++i) {
            if (act[i]) {
                *reinterpret_cast<int4v*>(kt_ + kdst[i]) = kr[i];
                // partner exchange (quad_perm [1,0,3,2]): the even lane assembles dims 0-3, the odd one 4-7
                const int s0 = odd_lane ? vr[i][0] : vr[i][2], s1 = odd_lane ? vr[i][1] : vr[i][3];
                const int r0 = __builtin_amdgcn_update_dpp(0, s0, 0xB1, 0xf, 0xf, true);
                const int r1 = __builtin_amdgcn_update_dpp(0, s1, 0xB1, 0xf, 0xf, true);
                const uint32_t lo0 = odd_lane ? (uint32_t)r0 : (uint32_t)vr[i][0], lo1 = odd_lane ? (uint32_t)r1 : (uint32_t)vr[i][1];
                const uint32_t hi0 = odd_lane ? (uint32_t)vr[i][2] : (uint32_t)r0, hi1 = odd_lane ? (uint32_t)vr[i][3] : (uint32_t)r1;
                uint8_t* vp = vt_ + vdst[i];
                *reinterpret_cast<uint32_t*>(vp) = __builtin_amdgcn_perm(hi0, lo0, 0x05040100u);
                *reinterpret_cast<uint32_t*>(vp + C::VROWB) = __builtin_amdgcn_perm(hi0, lo0, 0x07060302u);
                *reinterpret_cast<uint32_t*>(vp + 2 * C::VROWB) = __builtin_amdgcn_perm(hi1, lo1, 0x05040100u);
                *reinterpret_cast<uint32_t*>(vp + 3 * C::VROWB) = __builtin_amdgcn_perm(hi1, lo1, 0x07060302u);
            }
        }
    };

    // row D of both V images := {1.0, 1.0} in every pair slot (never overwritten by the staging stores)
    if (tid < 64)
        *reinterpret_cast<uint32_t*>(smem + 2 * C::KTILE + (tid >> 5) * C::VTILE + D * C::VROWB + (tid & 31) * 4) = 0x3c003c00u;
    if (nkt > 0) {
        load_tile(0, krA, vrA);
        if (nkt > 1) load_tile(1, krB, vrB);
        store_tile(0, krA, vrA);
    }
    __syncthreads();
    // one key tile; `cur` (LDS buffer) and the register sets are compile-time per call site: the loop below is
    // unrolled by two so that set A / set B never meet in a phi (the compiler otherwise copies them through
    // temporaries behind an s_waitcnt vmcnt(0) that exposes the whole global-load latency every tile)
    auto tile = [&](const int kt, const int cur, int4v (&krL)[C::KPT], int4v (&vrL)[C::KPT], int4v (&krS)[C::KPT],
                    int4v (&vrS)[C::KPT]) {
        if (kt + 2 < nkt) load_tile(kt + 2, krL, vrL);
        const uint8_t* kt_ = smem + cur * C::KTILE;
        const uint8_t* vt_ = smem + 2 * C::KTILE + cur * C::VTILE;

        float16v s[2];
#pragma unroll
        for (int sc = 0; sc < 2; ++sc) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[sc][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks)
                s[sc] = __builtin_amdgcn_mfma_f32_32x32x16_f16(attn_frag<D>(kt_ + (sc * 32 + l31) * C::KROW, ks, g), qf[ks], s[sc], 0, 0, 0);
        }
        // stage the NEXT tile while the QK^T MFMAs above are in flight: the other LDS buffer has had no reader
        // since the last barrier, and nothing below depends on these VALU / LDS-write instructions
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nkt) store_tile(cur ^ 1, krS, vrS);
        __builtin_amdgcn_sched_barrier(0);
        if (kt * 64 + 64 > kv_len) {
#pragma unroll
            for (int sc = 0; sc < 2; ++sc) attn_mask(s[sc], kt * 64 + sc * 32, g, kv_len);
        }
        // the lazy rescale of attn_tile.h's attn_lazy_rescale, kept inline in this one kernel: through the helper the D = 32
        // forms need 130 VGPRs instead of 128 (three resident waves per SIMD instead of four)
        const float mloc = attn_rowmax_shfl(s);
        if (__any((mloc - m_run) * a.c > 8.0f)) {
            const float m_new = fmaxf(m_run, mloc);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * a.c);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
            m_run = m_new;
        }
        const float mc = ((m_run == -INFINITY) ? 0.f : m_run) * a.c;
        // exp and P.V per 32-key sub-tile: the exponentials of the next piece run under the MFMAs of the previous one
#pragma unroll
        for (int sc = 0; sc < 2; ++sc) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[sc][r] = __builtin_amdgcn_exp2f(fmaf(s[sc][r], a.c, -mc));
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                const int kk = 2 * sc + k2, rq = 2 * k2;
                half8 pf;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    pf[e] = (half_t)s[sc][4 * rq + e];
                    pf[4 + e] = (half_t)s[sc][4 * rq + 4 + e];
                }
#pragma unroll
                for (int dt = 0; dt < C::DT; ++dt) {
                    const half8 vw = *reinterpret_cast<const half8*>(vt_ + vaddr[dt][kk]);
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vw, pf, oacc[dt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    };
    for (int kt = 0; kt < nkt; kt += 2) {
        tile(kt, 0, krA, vrA, krB, vrB);               // tile kt sits in buffer 0; loads kt+2 -> A, stages kt+1 <- B
        if (kt + 1 < nkt) tile(kt + 1, 1, krB, vrB, krA, vrA);
    }

    const float inv = attn_inv_row_sum<D>(oacc, l31);
    if (q_ok) attn_store_rows_h4<D>(oacc, inv, a.o + (long)seq * a.o_seq_stride + (long)qi * a.o_tok_stride + h * D, g);
}

// ---------------------------------------------------------------------------
// attn_fwd32d_kernel: the K / V tiles delivered by LDS-DMA (buffer_load_dwordx4 ... lds, AttnKvDma of attn_tile.h): no
// staging registers, no ds_write pass, no vmcnt coupling between the staged tile and the fragment reads.  The tile images
// are the ordinary padded row-major layout (K rows KROW bytes, V rows 192 bytes with the ones column behind the data, read
// as V^T with ds_read_b64_tr_b16).  The ~15 VGPRs this frees pay for fragment reads that run two ahead of the MFMAs
// (pinned with sched_barrier).  32 queries per wave, four waves per SIMD.
// ---------------------------------------------------------------------------
template <int D, int NW = 8, int KT = 64, class A = AttnArgs>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 4 : 3) void attn_fwd32d_kernel(A a) {
    constexpr bool ST = std::is_same<A, AttnQSArgs>::value;
    static_assert(KT % 64 == 0, "key tile in 64-row DMA units");
    using C = Att8Cfg<D, NW>;
    constexpr int KTB = (KT / 64) * C::KTILE;               // K tile bytes
    constexpr int VRB = 192, VT = KT * VRB;                 // row-major V image
    constexpr int PF = 2;
    static_assert(D * 2 + 2 <= VRB && C::DT * 64 <= VRB, "dims + ones column inside a row; every 32-dim tile readable");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, l31 = lane & 31;
    int qt, h, seq;
    if (!attn_xcd_map(a, 32 * NW, qt, h, seq)) return;
    [[maybe_unused]] TqGrid sq;
    if constexpr (ST) sq = tq_static(a.delta, a.zp, a.n_bits);
    const int kv_len = a.Lk;
    const half_t* kbase = a.k + (long)seq * a.kv_seq_stride + h * D;
    const half_t* vbase = a.v + (long)seq * a.kv_seq_stride + h * D;
    const int qi = qt * (32 * NW) + wave * 32 + l31;
    const bool q_ok = qi < a.Lq;
    half8 qf[C::KS];
    float16v oacc[C::DT];
    float m_run = -INFINITY;
    attn_q_frags<D>(a.q + (long)seq * a.q_seq_stride + (long)(q_ok ? qi : a.Lq - 1) * a.q_tok_stride + h * D, g, qf);
    attn_zero(oacc);
    const int nkt = (kv_len + KT - 1) / KT;
    const int strideB = (int)a.kv_tok_stride * 2;
    const unsigned nrec = kv_len > 0 ? (unsigned)(kv_len - 1) * (unsigned)strideB + D * 2 : 0u;
    AttnKvDma<D, NW, KT, C::KROW, VRB> dma;
    dma.init(wave, lane, strideB);
    const unsigned lds0 = attn_lds_addr(smem);
    auto issue = [&](int kt, int part = -1) __attribute__((always_inline)) {   // tile kt -> image pair kt & 1
        dma.issue(kbase, vbase, (unsigned)kt * (unsigned)KT * (unsigned)strideB, nrec, lds0 + (kt & 1) * KTB, lds0 + 2 * KTB + (kt & 1) * VT,
                  wave, part);
    };
    attn_fill_pad<D, VRB>(smem + 2 * KTB, 2 * KT, tid, 64 * NW);   // both V images (contiguous)
    if (nkt > 0) issue(0);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) asm volatile("" ::"v"(qf[ks]));   // the compiler's own wait for the Q loads goes HERE, not
                                                                          // (as vmcnt(0), stalling on the DMA) into the loop
    attn_wg_barrier();
    const int vtr0 = attn_vtr0<VRB>(lane, g);

    auto tile = [&](auto rag_tag, const int kt) __attribute__((always_inline)) {
        constexpr bool RAG = decltype(rag_tag)::value;
        const uint8_t* kt_ = smem + (kt & 1) * KTB + l31 * C::KROW;
        const uint8_t* vt_ = smem + 2 * KTB + (kt & 1) * VT + vtr0;
#pragma unroll
        for (int sc = 0; sc < KT / 32; ++sc) {
            float16v s;
            const float16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            AttnVF vf[2 * C::DT];
            half8 kf[C::KS];
            // fragment reads run PF ahead of the MFMAs in ONE sequence (K fragments 0..KS-1, then the V^T fragments: the
            // first of those fly under the softmax); sched_barrier pins the order - left alone the scheduler sinks every
            // read next to its MFMA and exposes one LDS latency per MFMA
            auto rdc = [&](int n) __attribute__((always_inline)) { attn_read_frag<D, VRB>(n, kt_ + sc * 32 * C::KROW, vt_ + sc * 32 * VRB, g, kf, vf); };
#pragma unroll
            for (int n = 0; n < PF; ++n) rdc(n);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks) {
                rdc(ks + PF);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qf[ks], ks == 0 ? zero16 : s, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // next tile's DMA into the buffers whose last readers passed the previous barrier: issued behind the QK^T
            // chains of the first two half tiles, so that the MFMAs of a tile start right after the barrier and the DMA
            // issue (~100 cycles per piece) sits in the waits for those chains' results
            // (in two instalments: A/B on one box 112.0-115.5 vs 115.3-118.0 us at 16 x 1024, 112 vs 122 us at 1 x 4096
            //  against all pieces behind the first chain; at the top of the tile, before any MFMA: 122.7 us)
            if (sc < 2 && kt + 1 < nkt) issue(kt + 1, sc);
            if constexpr (RAG) attn_mask(s, kt * KT + sc * 32, g, kv_len);
            const float mc = attn_lazy_rescale(attn_rowmax_max3(s), m_run, oacc, a.c);
            half8 pf[2];
            attn_exp_pack(s, a.c, mc, pf);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int idx = 0; idx < 2 * C::DT; ++idx) {
                rdc(C::KS + idx + PF);
                oacc[idx % C::DT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[idx].v, pf[idx / C::DT], oacc[idx % C::DT], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        attn_wg_barrier();
    };
    {
        const int nfull = kv_len / KT;
        int kt = 0;
        for (; kt < nfull; ++kt) tile(std::false_type{}, kt);
        if (kt < nkt) tile(std::true_type{}, kt);
    }
    const float inv = attn_inv_row_sum<D>(oacc, l31);
    half_t* orow = a.o + (long)seq * a.o_seq_stride + (long)(q_ok ? qi : a.Lq - 1) * a.o_tok_stride + h * D;
    if constexpr (ST) {
        if (a.o) attn_store_rows<D>(oacc, inv, orow, g, q_ok);        // kernel-uniform
        attn_quant_rows<D>(oacc, inv, a, sq, seq * a.Lq + (q_ok ? qi : a.Lq - 1), h, g, q_ok);
    } else {
        if constexpr (D % 8 == 0 && D >= 16) attn_store_rows<D>(oacc, inv, orow, g, q_ok);
        else if (q_ok) attn_store_rows_h4<D>(oacc, inv, orow, g);
    }
}

template <int D, int NW = 8, int KT = 64, class A>
static int launch_attn32d(const A& a, hipStream_t st) {
    constexpr int LDS = 2 * (KT / 64) * Att8Cfg<D, 8>::KTILE + 2 * KT * 192;
    constexpr auto k = attn_fwd32d_kernel<D, NW, KT, A>;
    const int nqt = (a.Lq + 32 * NW - 1) / (32 * NW), G = a.n_seq * a.H;
    if (const int rc = vq_prepare_kernel<k>(LDS)) return rc;
    hipLaunchKernelGGL(k, dim3(8 * ((G + 7) / 8) * nqt), dim3(64 * NW), LDS, st, a);
    return vq_check_launch();
}

// ---------------------------------------------------------------------------
// attn_fwd64d_kernel (round 6): attn_fwd32d_kernel with 64 queries per wave (two 32-row blocks A / B) and two waves per
// SIMD (<= 256 VGPRs) instead of 32 queries and four.  Every K / V^T fragment read from LDS feeds TWO MFMAs (LDS bytes per
// MFMA halved), the QK^T chains of the two blocks interleave (no 5-deep dependent chain), and block B's softmax (VALU /
// v_exp) is issued between block A's P.V MFMAs.  Same tile images, fragment layouts, lazy rescale and ones-column row sums;
// per query row the arithmetic is that of attn_fwd32d_kernel (bit-identical outputs, tested).
// ---------------------------------------------------------------------------
template <int D, int NW = 8, int KT = 64, class A = AttnArgs>
__global__ __launch_bounds__(64 * NW, 2) void attn_fwd64d_kernel(A a) {
    constexpr bool ST = std::is_same<A, AttnQSArgs>::value;
    static_assert(KT % 64 == 0, "key tile in 64-row DMA units");
    constexpr int NQ = 2;
    using C = Att8Cfg<D, NW>;
    constexpr int KTB = (KT / 64) * C::KTILE;
    constexpr int VRB = 192, VT = KT * VRB;
    constexpr int PF = 2;
    static_assert(D * 2 + 2 <= VRB && C::DT * 64 <= VRB, "dims + ones column inside a row; every 32-dim tile readable");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, l31 = lane & 31;
    int qt, h, seq;
    if (!attn_xcd_map(a, 32 * NQ * NW, qt, h, seq)) return;
    [[maybe_unused]] TqGrid sq;
    if constexpr (ST) sq = tq_static(a.delta, a.zp, a.n_bits);
    const int kv_len = a.Lk;
    const half_t* kbase = a.k + (long)seq * a.kv_seq_stride + h * D;
    const half_t* vbase = a.v + (long)seq * a.kv_seq_stride + h * D;
    int qi[NQ];
    bool q_ok[NQ];
    half8 qf[NQ][C::KS];
    float16v oacc[NQ][C::DT];
    float m_run[NQ];
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
        qi[nq] = qt * (32 * NQ * NW) + wave * (32 * NQ) + nq * 32 + l31;
        q_ok[nq] = qi[nq] < a.Lq;
        m_run[nq] = -INFINITY;
        attn_q_frags<D>(a.q + (long)seq * a.q_seq_stride + (long)(q_ok[nq] ? qi[nq] : a.Lq - 1) * a.q_tok_stride + h * D, g, qf[nq]);
        attn_zero(oacc[nq]);
    }
    const int nkt = (kv_len + KT - 1) / KT;
    const int strideB = (int)a.kv_tok_stride * 2;
    const unsigned nrec = kv_len > 0 ? (unsigned)(kv_len - 1) * (unsigned)strideB + D * 2 : 0u;
    AttnKvDma<D, NW, KT, C::KROW, VRB> dma;
    dma.init(wave, lane, strideB);
    const unsigned lds0 = attn_lds_addr(smem);
    auto issue = [&](int kt, int part = -1) __attribute__((always_inline)) {   // tile kt -> image pair kt & 1
        dma.issue(kbase, vbase, (unsigned)kt * (unsigned)KT * (unsigned)strideB, nrec, lds0 + (kt & 1) * KTB, lds0 + 2 * KTB + (kt & 1) * VT,
                  wave, part);
    };
    attn_fill_pad<D, VRB>(smem + 2 * KTB, 2 * KT, tid, 64 * NW);   // both V images (contiguous)
    if (nkt > 0) issue(0);
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq)
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) asm volatile("" ::"v"(qf[nq][ks]));   // the compiler's wait for the Q loads goes HERE
    attn_wg_barrier();
    const int vtr0 = attn_vtr0<VRB>(lane, g);

    auto tile = [&](auto rag_tag, const int kt) __attribute__((always_inline)) {
        constexpr bool RAG = decltype(rag_tag)::value;
        const uint8_t* kt_ = smem + (kt & 1) * KTB + l31 * C::KROW;
        const uint8_t* vt_ = smem + 2 * KTB + (kt & 1) * VT + vtr0;
#pragma unroll
        for (int sc = 0; sc < KT / 32; ++sc) {
            float16v s[NQ];
            const float16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            AttnVF vf[2 * C::DT];
            half8 kf[C::KS];
            auto rdc = [&](int n) __attribute__((always_inline)) { attn_read_frag<D, VRB>(n, kt_ + sc * 32 * C::KROW, vt_ + sc * 32 * VRB, g, kf, vf); };
#pragma unroll
            for (int n = 0; n < PF; ++n) rdc(n);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < C::KS; ++ks) {                       // two interleaved chains: one K fragment, two MFMAs
                rdc(ks + PF);
#pragma unroll
                for (int nq = 0; nq < NQ; ++nq)
                    s[nq] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qf[nq][ks], ks == 0 ? zero16 : s[nq], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (sc < 2 && kt + 1 < nkt) issue(kt + 1, sc);
            half8 pf[NQ][2];
            float mc[NQ];
            // decide(nq): row maxima of block nq, the lazy rescale of its O (a branch), the exponent offset.  Both blocks
            // decide FIRST, so that what remains - expo(nq): 16 fma + 16 v_exp + 8 cvt, straight-line - can sit between MFMAs
            // (The mask, attn_rowmax_max3's chain, the lazy rescale and exp-and-pack of attn_tile.h, kept written out in this
            //  one kernel: on the helpers it needs 211 VGPRs instead of 208 and 2 x 4096 x 4096 tokens took 174.7-176.6 us
            //  against the parent's 171.2-171.9 us; this form is inside the parent's band - profiles/refactor_attention_isa.md)
            auto decide = [&](int nq) __attribute__((always_inline)) {
                if constexpr (RAG) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (kt * KT + sc * 32 + (r & 3) + 8 * (r >> 2) + 4 * g >= kv_len) s[nq][r] = -INFINITY;
                }
                float mloc;
                {
                    float mx;   // (asm chain and the compiler-visible first read: see attn_rowmax_max3)
                    const float s0 = s[nq][0] + 0.0f;
                    asm("v_max3_f32 %0, %1, %2, %3\n\tv_max3_f32 %0, %0, %4, %5\n\tv_max3_f32 %0, %0, %6, %7\n\t"
                        "v_max3_f32 %0, %0, %8, %9\n\tv_max3_f32 %0, %0, %10, %11\n\tv_max3_f32 %0, %0, %12, %13\n\t"
                        "v_max3_f32 %0, %0, %14, %15\n\tv_max_f32 %0, %0, %16"
                        : "=&v"(mx)
                        : "v"(s0), "v"(s[nq][1]), "v"(s[nq][2]), "v"(s[nq][3]), "v"(s[nq][4]), "v"(s[nq][5]), "v"(s[nq][6]), "v"(s[nq][7]),
                          "v"(s[nq][8]), "v"(s[nq][9]), "v"(s[nq][10]), "v"(s[nq][11]), "v"(s[nq][12]), "v"(s[nq][13]), "v"(s[nq][14]),
                          "v"(s[nq][15]));
                    const unsigned mb = __builtin_bit_cast(unsigned, mx);
                    const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
                    asm("v_max_f32 %0, %1, %2" : "=v"(mloc) : "v"(sw[0]), "v"(sw[1]));
                }
                if (__any((mloc - m_run[nq]) * a.c > 8.0f)) {
                    const float m_new = fmaxf(m_run[nq], mloc);
                    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
                    const float alpha = __builtin_amdgcn_exp2f((m_run[nq] - m_use) * a.c);
#pragma unroll
                    for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) oacc[nq][dt][r] *= alpha;
                    m_run[nq] = m_new;
                }
                mc[nq] = ((m_run[nq] == -INFINITY) ? 0.f : m_run[nq]) * a.c;
            };
            auto expo = [&](int nq) __attribute__((always_inline)) {
#pragma unroll
                for (int r = 0; r < 16; r += 2) {                     // plain v_fma_f32 (see attn_exp_pack)
                    const float t0 = __builtin_fmaf(s[nq][r], a.c, -mc[nq]), t1 = __builtin_fmaf(s[nq][r + 1], a.c, -mc[nq]);
                    pf[nq][r >> 3][r & 7] = (half_t)__builtin_amdgcn_exp2f(t0);
                    pf[nq][r >> 3][(r & 7) + 1] = (half_t)__builtin_amdgcn_exp2f(t1);
                }
            };
            decide(0);
            decide(1);
            expo(0);
            __builtin_amdgcn_sched_barrier(0);
            // block A's P.V MFMAs with block B's exponentials between them (one region for the scheduler), then block B's P.V
#pragma unroll
            for (int idx = 0; idx < 2 * C::DT; ++idx) {
                rdc(C::KS + idx + PF);
                oacc[0][idx % C::DT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[idx].v, pf[0][idx / C::DT], oacc[0][idx % C::DT], 0, 0, 0);
            }
            expo(1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int idx = 0; idx < 2 * C::DT; ++idx)
                oacc[1][idx % C::DT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[idx].v, pf[1][idx / C::DT], oacc[1][idx % C::DT], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        attn_wg_barrier();
    };
    {
        const int nfull = kv_len / KT;
        int kt = 0;
        for (; kt < nfull; ++kt) tile(std::false_type{}, kt);
        if (kt < nkt) tile(std::true_type{}, kt);
    }
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
        half_t* orow = a.o + (long)seq * a.o_seq_stride + (long)(q_ok[nq] ? qi[nq] : a.Lq - 1) * a.o_tok_stride + h * D;
        if constexpr (ST) {
            const float inv = attn_inv_row_sum<D>(oacc[nq], l31);
            if (a.o) attn_store_rows<D>(oacc[nq], inv, orow, g, q_ok[nq]);   // kernel-uniform
            attn_quant_rows<D>(oacc[nq], inv, a, sq, seq * a.Lq + (q_ok[nq] ? qi[nq] : a.Lq - 1), h, g, q_ok[nq]);
        } else {
            attn_store_rows<D>(oacc[nq], attn_inv_row_sum<D>(oacc[nq], l31), orow, g, q_ok[nq]);
        }
    }
}

template <int D, int NW = 8, int KT = 64, class A>
static int launch_attn64d(const A& a, hipStream_t st) {
    constexpr int LDS = 2 * (KT / 64) * Att8Cfg<D, 8>::KTILE + 2 * KT * 192;
    constexpr auto k = attn_fwd64d_kernel<D, NW, KT, A>;
    const int nqt = (a.Lq + 64 * NW - 1) / (64 * NW), G = a.n_seq * a.H;
    if (const int rc = vq_prepare_kernel<k>(LDS)) return rc;
    hipLaunchKernelGGL(k, dim3(8 * ((G + 7) / 8) * nqt), dim3(64 * NW), LDS, st, a);
    return vq_check_launch();
}

// ---------------------------------------------------------------------------
// attn_cross32_kernel (round 4): cross attention against a SHORT key/value sequence (<= 128 keys) as attn_fwd32d_kernel
// with the loops interchanged - K and V of ONE (sequence, head) pair are brought into LDS ONCE per workgroup (two 64-key
// tile images, the layouts and fragment reads of attn_fwd32d_kernel: K rows KROW bytes read as ds_read_b128, V row-major
// read with ds_read_b64_tr_b16, ones column for the row sums), then the workgroup walks its slice of the query tiles:
// 32 queries per wave, no DMA, no barrier and no LDS write inside the walk, the next tile's Q fragments requested
// before the current tile's MFMAs.  Counters of the register-resident kernel it replaces (attn_cross_reg_kernel:
// 33.7 us for 80 MB, profiles/r04_hbm_kernels_pmc.md): 160 of its 256 VGPRs hold K / V^T, which leaves two waves per
// SIMD with ONE 16-query sub-tile in flight each (SQ_WAIT_ANY 0.49, 1.3 resident waves per SIMD on average), and every
// one of its 2048 waves re-reads and transposes its head's K / V in a ~40-instruction-per-key-row prologue (75 MB of L2
// reads - as much as the kernel's HBM traffic).  Here a wave needs ~128 VGPRs: four waves per SIMD, 32 queries each,
// and the K / V images are staged by LDS-DMA once per 8 waves.
// ---------------------------------------------------------------------------
// NT (round 6): 64-key tile images resident in LDS - 2 for the <= 128 prompt tokens of STDiT / PixArt-alpha (two workgroups per
// CU), 3 ... 5 for PixArt-Sigma's prompts of up to 300 tokens (one workgroup per CU; the generic kernel those launches took
// restaged K / V per 128 queries: 25.4 us per launch, 5 % of that step).
template <int D, int NW = 8, int NT = 2, class A = AttnArgs>
__global__ __launch_bounds__(64 * NW, NT == 2 ? 32 / NW : 16 / NW) void attn_cross32_kernel(A a, int nslice) {
    constexpr bool ST = std::is_same<A, AttnQSArgs>::value;
    using C = Att8Cfg<D, NW>;
    constexpr int KT = 64, KTB = C::KTILE, VRB = 192, VT = KT * VRB;
    static_assert(D * 2 + 2 <= VRB && C::DT * 64 <= VRB, "dims + ones column inside a row; every 32-dim tile readable");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, l31 = lane & 31;
    // workgroup -> (query slice, head, sequence): all heads of one slice on ONE XCD (bid % 8), next to each other in its
    // dispatch order - their 144-byte q / o row segments share cache lines, which then meet in that XCD's L2
    const int bid = blockIdx.x, xcd = bid & 7, idx = bid >> 3;
    const int G = a.n_seq * a.H;
    const int slice = (idx / G) * 8 + xcd, pair = idx % G;
    if (slice >= nslice) return;
    const int seq = pair / a.H, h = pair - seq * a.H;
    const half_t* kbase;
    const half_t* vbase;
    const int kv_len = attn_kv_base<D>(a, seq, h, kbase, vbase, NT * KT);   // host guarantees <= NT * 64
    const int strideB = (int)a.kv_tok_stride * 2;
    const unsigned nrec = kv_len > 0 ? (unsigned)(kv_len - 1) * (unsigned)strideB + D * 2 : 0u;
    // ---- prologue: every tile image by LDS-DMA (rows past the last key are outside num_records: zeros)
    {
        AttnKvDma<D, NW, KT, C::KROW, VRB> dma;
        dma.init(wave, lane, strideB);
        const unsigned lds0 = attn_lds_addr(smem);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
            dma.template issue<true>(kbase, vbase, (unsigned)kt * (unsigned)KT * (unsigned)strideB, nrec, lds0 + kt * KTB,
                                     lds0 + NT * KTB + kt * VT, wave);
    }
    attn_fill_pad<D, VRB>(smem + NT * KTB, NT * KT, tid, 64 * NW);   // every V image (contiguous)
    const int nqt = (a.Lq + 32 * NW - 1) / (32 * NW);
    const half_t* qseq = a.q + (long)seq * a.q_seq_stride + h * D;
    half_t* oseq = a.o + (long)seq * a.o_seq_stride + h * D;
    // Q tiles: each wave's 32 rows x D go global -> LDS by LDS-DMA into a PRIVATE image (rows of KROW bytes like the K
    // image: a wave-instruction covers 64 consecutive 16-byte slots = ~7 whole 144-byte row segments - the per-lane
    // fragment loads this replaces touched 32 rows x 32 bytes per instruction), requested one tile ahead; the MFMA
    // operand fragments are then ds_read_b128 of that image (conflict-free: odd number of slots per row).
    constexpr int QSL = C::KROW / 16, QW = 32 * C::KROW, NQI = (32 * QSL + 63) / 64;
    uint8_t* qreg = smem + NT * KTB + NT * VT + wave * QW;
    const unsigned qdst = __builtin_amdgcn_readfirstlane(attn_lds_addr(qreg));
    AttnDmaSlot qsl[NQI];
#pragma unroll
    for (int i = 0; i < NQI; ++i) qsl[i] = attn_dma_slot<QSL, C::CHD, 32>(i, lane, (int)a.q_tok_stride * 2);
    auto issue_q = [&](int qt) __attribute__((always_inline)) {
        int q0 = qt * (32 * NW) + wave * 32;
        const int last = a.Lq - 1;
        const int nrows = q0 > last ? 0 : (last - q0 + 1 < 32 ? last - q0 + 1 : 32);
        q0 = q0 > last ? last : q0;
        // rows past the last query are outside num_records: they land as zeros
        const unsigned nr = nrows > 0 ? (unsigned)(nrows - 1) * (unsigned)a.q_tok_stride * 2u + D * 2 : 0u;
#pragma unroll
        for (int i = 0; i < NQI; ++i) attn_dma_instr(qseq + (long)q0 * a.q_tok_stride, nr, qdst + i * 1024, qsl[i]);
    };
    int qt = slice;
    if (qt < nqt) issue_q(qt);
    attn_wg_barrier();                                     // the K / V images (and the first Q tile) have landed
    const uint8_t* q_l = qreg + l31 * C::KROW;
    int stores_behind = 0;                                 // store instructions issued after the Q DMA in flight (wave-uniform)
    constexpr int NST = (D / 8 + 1) / 2;                   // store instructions per tile (see attn_store_rows)
    const int nhalf = (kv_len + 31) / 32;                  // 32-key half tiles that hold keys (wave-uniform, 1 .. 2 NT)
    const uint8_t* k_l = smem + l31 * C::KROW;
    const uint8_t* v_l = smem + NT * KTB + attn_vtr0<VRB>(lane, g);

    for (; qt < nqt; qt += nslice) {
        const int qnext = qt + nslice;
        // this tile's Q image has landed once at most the stores issued behind its DMA are outstanding (in-order vmcnt)
        if (stores_behind == NST) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NST) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        half8 qf[C::KS];
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) qf[ks] = attn_frag<D>(q_l, ks, g);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // fragments are in registers: the image is free
        if (qnext < nqt) issue_q(qnext);                              // next tile: in flight under this tile's work
        float16v oacc[C::DT];
        attn_zero(oacc);
        float m_run = -INFINITY;
#pragma nounroll
        for (int hf = 0; hf < nhalf; ++hf) {               // the image rows of half hf: K rows hf * 32.., V rows the same
            float16v s;
            const float16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            {
                half8 kf[C::KS];
#pragma unroll
                for (int ks = 0; ks < C::KS; ++ks) kf[ks] = attn_frag<D, false>(k_l + hf * 32 * C::KROW, ks, g);
#pragma unroll
                for (int ks = 0; ks < C::KS; ++ks)
                    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qf[ks], ks == 0 ? zero16 : s, 0, 0, 0);
            }
            AttnVF vf[2 * C::DT];                          // V^T fragments: requested here, they fly under the softmax
#pragma unroll
            for (int idx2 = 0; idx2 < 2 * C::DT; ++idx2) attn_vt_frag<C::DT, VRB>(v_l + hf * 32 * VRB, idx2, vf[idx2]);
            if ((hf + 1) * 32 > kv_len) attn_mask(s, hf * 32, g, kv_len);   // wave-uniform: the ragged last half
            const float mc = attn_lazy_rescale(attn_rowmax_swap(s), m_run, oacc, a.c);
            half8 pf[2];
            attn_exp_pack(s, a.c, mc, pf);
#pragma unroll
            for (int idx2 = 0; idx2 < 2 * C::DT; ++idx2)
                oacc[idx2 % C::DT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[idx2].v, pf[idx2 / C::DT], oacc[idx2 % C::DT], 0, 0, 0);
        }
        const float inv = attn_inv_row_sum<D>(oacc, l31);
        const int qi = qt * (32 * NW) + wave * 32 + l31;
        const bool wave_live = qt * (32 * NW) + wave * 32 < a.Lq;      // wave-uniform
        if (wave_live) {
            half_t* orow = oseq + (long)(qi < a.Lq ? qi : a.Lq - 1) * a.o_tok_stride;
            if constexpr (ST) {
                // (the stores and loads behind the Q DMA in flight are not a fixed number here: the next tile waits for all)
                // (the grid is read per tile - one scalar load and a division - not held in registers across the walk)
                if (a.o) attn_store_rows<D, C::DT>(oacc, inv, orow, g, qi < a.Lq);   // kernel-uniform
                const TqGrid sq = tq_static(a.delta, a.zp, a.n_bits);
                attn_quant_rows<D, C::DT>(oacc, inv, a, sq, seq * a.Lq + (qi < a.Lq ? qi : a.Lq - 1), h, g, qi < a.Lq);
                stores_behind = 0;
            } else {
                attn_store_rows<D, C::DT>(oacc, inv, orow, g, qi < a.Lq);   // 16-byte stores (NST of them per lane, + one 8-byte store for an odd group)
                stores_behind = NST;
            }
        } else {
            stores_behind = 0;
        }
    }
}

template <int D, int NT = 2, class A>
static int launch_cross32(const A& a, hipStream_t st) {
    constexpr int NW = 8;
    constexpr int LDS = NT * Att8Cfg<D, 8>::KTILE + NT * 64 * 192 + NW * 32 * Att8Cfg<D, 8>::KROW;
    static_assert(LDS <= 163840, "LDS budget of one CU");
    constexpr auto k = attn_cross32_kernel<D, NW, NT, A>;
    int ncu = 0;
    if (const int rc = vq_prepare_kernel<k>(LDS, &ncu)) return rc;
    // NT == 2: two 8-wave workgroups per CU (four waves per SIMD; 1 / 3 / 4 measured slower, round 6); more tile images: one (LDS).
    // The (sequence, head) pairs share the chip, every workgroup walks >= 1 query tile of 256
    const int G = a.n_seq * a.H, nqt = (a.Lq + 32 * NW - 1) / (32 * NW);
    int nslice = ((NT == 2 ? 2 : 1) * ncu + G - 1) / G;
    nslice = nslice < 1 ? 1 : (nslice > nqt ? nqt : nslice);
    const int s8 = (nslice + 7) / 8;                      // slices are dealt to the 8 XCDs: grid padded to a multiple
    hipLaunchKernelGGL(k, dim3(8 * s8 * G), dim3(64 * NW), LDS, st, a, nslice);
    return vq_check_launch();
}

// ---------------------------------------------------------------------------
// attn_cross_reg_kernel: cross attention against a SHORT key/value sequence (<= 128 keys: the <= 120 prompt tokens of
// STDiT), head_dim 72.  attn_fwd_kernel moved the algorithmic 78 MB in 42 us (1.9 TB/s): 2048 workgroups each staged
// the same K/V tile pair through LDS, read their queries, and ran two short flash iterations behind barriers.  Here
// K and V^T of ONE head live in the REGISTERS of one wave for the whole kernel, already in MFMA operand form:
//   S^T[key][query] = K Q^T : A = K  (16 keys  x 32 dims per lane group: 2 x 16x16x32 + 1 x 16x16x16 for dims 64..71)
//   O^T[dim][query] = V^T P^T: A = V^T (16 dims x 32 keys): 16x16x32; the k-slot order of a 32-key step is
//       slot (g4, e) <-> key (2*kp + (e >> 2)) * 16 + 4*g4 + (e & 3), i.e. exactly the two S^T accumulator quads
//       the lane already holds for key tiles 2*kp and 2*kp + 1: P^T needs no shuffle, only exp2 and cvt.
// A workgroup = 8 waves = 8 consecutive heads walking the same 16-query sub-tiles (their 144-byte row segments
// share cache lines), persistent over sub-tiles; the next sub-tile's q fragments are requested as soon as QK^T is issued.  No LDS in the loop,
// no barriers; V^T is transposed once per wave through a private LDS region.  All keys of a row are present at once,
// so the softmax is the plain two-pass form (no running rescale).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(512) void attn_cross_reg_kernel(AttnArgs a) {
    constexpr int D = 72, NKT = 8, VROWB = 152;    // V staging row stride: 38 dwords -> the four lane groups hit different banks
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 15, g4 = lane >> 4;
    const int h = blockIdx.y * 8 + wave, seq = blockIdx.z;
    const half_t* kbase;
    const half_t* vbase;
    const int kv_len = attn_kv_base<D>(a, seq, h, kbase, vbase, 16 * NKT);   // host guarantees <= 128
    const half8 z8 = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
    const half4 z4 = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};

    // ---- V of this head -> private LDS region (row-major, coalesced 16-byte chunks), then V^T operand fragments
    uint8_t* vreg = smem + wave * (16 * NKT * VROWB);
    {
        constexpr int CH = D / 8, NCH = 16 * NKT * CH;           // 9 chunks per key row
#pragma unroll
        for (int i = 0; i < (NCH + 63) / 64; ++i) {
            const int c = lane + i * 64;
            const int key = c / CH, ch = c - key * CH;
            int4v val = {0, 0, 0, 0};
            if (c < NCH && key < kv_len) val = *reinterpret_cast<const int4v*>(vbase + (long)key * a.kv_tok_stride + ch * 8);
            if (c < NCH) {
                *reinterpret_cast<int2v*>(vreg + key * VROWB + ch * 16) = int2v{val[0], val[1]};
                *reinterpret_cast<int2v*>(vreg + key * VROWB + ch * 16 + 8) = int2v{val[2], val[3]};
            }
        }
    }
    // K operand fragments straight from global: lane = key lq of tile kt, 8 dims per 32-dim step
    half8 kf[NKT][2];
    half4 kt4[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        const int key = kt * 16 + lq;
        const half_t* kr = kbase + (long)(key < kv_len ? key : 0) * a.kv_tok_stride;
        const bool ok = key < kv_len;
        kf[kt][0] = ok ? *reinterpret_cast<const half8*>(kr + 8 * g4) : z8;
        kf[kt][1] = ok ? *reinterpret_cast<const half8*>(kr + 32 + 8 * g4) : z8;
        kt4[kt] = (ok && g4 < 2) ? *reinterpret_cast<const half4*>(kr + 64 + 4 * g4) : z4;
    }
    // (the LDS writes above are this wave's own: in-order LDS, no workgroup barrier needed)
    half8 vf[5][4];
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) {
        const int d = dt * 16 + lq;
#pragma unroll
        for (int kp = 0; kp < 4; ++kp)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int key = (2 * kp + (e >> 2)) * 16 + 4 * g4 + (e & 3);
                // dim D (= 72, inside the zero-padded fifth tile) is a row of ones: the softmax row sum then comes out
                // of the P.V MFMAs (O^T row D) instead of 32 adds per sub-tile
                vf[dt][kp][e] = d < D ? *reinterpret_cast<const half_t*>(vreg + key * VROWB + d * 2)
                                      : (d == D ? (half_t)1.f : (half_t)0.f);
            }
    }

    // ---- persistent walk over 16-query sub-tiles
    const int nsub = (a.Lq + 15) / 16;
    const half_t* qseq = a.q + (long)seq * a.q_seq_stride + h * D;
    half_t* oseq = a.o + (long)seq * a.o_seq_stride + h * D;
    half8 qa, qb;
    half4 qc;
    auto load_q = [&](int st, half8& x0, half8& x1, half4& x2) {
        int qi = st * 16 + lq;
        qi = qi < a.Lq ? qi : a.Lq - 1;
        const half_t* qr = qseq + (long)qi * a.q_tok_stride;
        x0 = *reinterpret_cast<const half8*>(qr + 8 * g4);
        x1 = *reinterpret_cast<const half8*>(qr + 32 + 8 * g4);
        x2 = g4 < 2 ? *reinterpret_cast<const half4*>(qr + 64 + 4 * g4) : z4;
    };
    int st = blockIdx.x;
    if (st < nsub) load_q(st, qa, qb, qc);
    for (; st < nsub; st += gridDim.x) {
        const int nst = st + (int)gridDim.x;
        float4v sc[NKT];
        float m = -INFINITY;
        // MFMA HAZARD (measured, tools/dbg_cross.py): a 16x16x16 MFMA that takes the result of a 16x16x32 MFMA as
        // its SrcC right behind it (or the other way round) reads a STALE accumulator on gfx950 with this compiler -
        // the wait states inserted between dependent MFMAs of different shapes are too few (32 cycles of s_nop fix
        // it; same-shape chains are fine).  So the two shapes are issued in separate phases: all 32-dim steps of
        // the eight key tiles, then the eight 16-dim tails, each >= 7 MFMAs behind the instruction it accumulates on
        // (skipping the empty key tiles of short prompts behind wave-uniform branches was slower: 38.7 vs 35.2 us).
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            float4v s = {0.f, 0.f, 0.f, 0.f};
            s = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][0], qa, s, 0, 0, 0);
            sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][1], qb, s, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) sc[kt] = __builtin_amdgcn_mfma_f32_16x16x16f16(kt4[kt], qc, sc[kt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (kt * 16 + 4 * g4 + r >= kv_len) sc[kt][r] = -INFINITY;
                m = fmaxf(m, sc[kt][r]);
            }
        if (nst < nsub) load_q(nst, qa, qb, qc);       // next sub-tile's fragments land during softmax and P.V
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const float m_use = (m == -INFINITY) ? 0.f : m;
        const float nmc = -m_use * a.c;                // exp2(s*c - m*c): one fma per score instead of sub + mul
        half8 pf[4];
        {
            typedef float float2v __attribute__((ext_vector_type(2)));
            const float2v cc2 = {a.c, a.c}, nm2 = {nmc, nmc};
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const float2v t = __builtin_elementwise_fma(float2v{sc[kt][r], sc[kt][r + 1]}, cc2, nm2);   // v_pk_fma_f32
                    pf[kt >> 1][(kt & 1) * 4 + r] = (half_t)__builtin_amdgcn_exp2f(t[0]);
                    pf[kt >> 1][(kt & 1) * 4 + r + 1] = (half_t)__builtin_amdgcn_exp2f(t[1]);
                }
        }
        const int qi = st * 16 + lq;
        half_t* orow = oseq + (long)qi * a.o_tok_stride;
        // fifth dim tile first: its row D - 64 = 8 (lane group g4 = 2, register 0) is the row sum of this lane's query
        float inv;
        float4v o4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kp = 0; kp < 4; ++kp) o4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[4][kp], pf[kp], o4, 0, 0, 0);
        {
            const float psum = __shfl(o4[0], lq + 32);
            inv = psum > 0.f ? __fdiv_rn(1.0f, psum) : 0.f;
        }
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) {
            float4v o = o4;
            if (dt < 4) {
                o = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kp = 0; kp < 4; ++kp) o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[dt][kp], pf[kp], o, 0, 0, 0);
            }
            const int d0 = dt * 16 + 4 * g4;
            if (d0 < D && qi < a.Lq) {
                half4 ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[r] = (half_t)(o[r] * inv);
                *reinterpret_cast<half4*>(orow + d0) = ov;
            }
        }
    }
}

static int launch_cross_reg(const AttnArgs& a, hipStream_t st) {
    constexpr int LDS = 8 * 128 * 152;
    constexpr auto k = attn_cross_reg_kernel;
    int ncu = 0;
    if (const int rc = vq_prepare_kernel<k>(LDS, &ncu)) return rc;
    const int groups = a.n_seq * (a.H / 8);            // (sequence, 8-head group) pairs share the CUs
    const int nsub = (a.Lq + 15) / 16;
    int gx = ncu / groups;
    gx = gx < 1 ? 1 : (gx > nsub ? nsub : gx);
    hipLaunchKernelGGL(k, dim3(gx, a.H / 8, a.n_seq), dim3(512), LDS, st, a);
    return vq_check_launch();
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
template <int D, int NW>
static int launch_attn8(const AttnArgs& a, hipStream_t st) {
    using C = Att8Cfg<D, NW>;
    constexpr auto k = attn_fwd8_kernel<D, NW>;
    if (const int rc = vq_prepare_kernel<k>(C::LDS)) return rc;
    const int nqt = (a.Lq + 32 * NW - 1) / (32 * NW), G = a.n_seq * a.H;
    dim3 grid(8 * ((G + 7) / 8) * nqt);
    hipLaunchKernelGGL(k, grid, dim3(64 * NW), C::LDS, st, a);
    return vq_check_launch();
}

// The kernel vq_attn_fwd runs for these (checked) arguments: a VQ_ATTN_K_* id of include/viditq.h, whose comments give the
// same table.  The one place the dispatch is decided - launch_attn switches on it and vq_attn_fwd_route returns it - so the
// test hook cannot disagree with the launch.  No HIP call, no switch: the retired arms live in the lab's attn_lab.hip.
template <int D>
static int attn_route(const AttnArgs& a) {
    const bool off32 = (long)a.Lk * a.kv_tok_stride * 2 < (1l << 31);     // K / V addressed with 32-bit byte offsets
    // cross attention, Lq >= 256: K / V of a (sequence, head) pair resident in LDS - two 64-key tile images for a known
    // bound of <= 128 prompt tokens, 3 ... 5 (one workgroup per CU) for bounds up to 320 with per-sample offsets
    // (PixArt-Sigma: 300)
    if (a.Lk > 0 && a.Lk <= 128 && a.Lq >= 256 && off32) return VQ_ATTN_K_CROSS32_2;
    if constexpr (D >= 64) {
        if (a.kv_off && a.Lk > 128 && a.Lk <= 320 && a.Lq >= 256 && off32)
            return a.Lk <= 192 ? VQ_ATTN_K_CROSS32_3 : a.Lk <= 256 ? VQ_ATTN_K_CROSS32_4 : VQ_ATTN_K_CROSS32_5;
    }
    // ... and shorter query sequences: K, V^T in registers
    if (D == 72 && a.Lk > 0 && a.Lk <= 128 && a.H % 8 == 0 && a.Lq >= 64) return VQ_ATTN_K_CROSS_REG;
    // long key sequences of one length: the LDS-DMA kernels.  Short ones (<= 2 key tiles, where the per-workgroup
    // prologue dominates), short query sequences and offsets with an unknown bound keep the first kernel.
    if (!a.kv_off && a.Lk > 128 && a.Lq >= 96) {
        // 64 queries per wave (attn_fwd64d_kernel) where a workgroup walks MANY key tiles (PixArt-Sigma's 4096-token images:
        // 181.4 vs 188.1 us, round 6); at 1024 keys the two forms tie (111.7 vs 111.6 us) and the 32-query form stays
        if (off32 && a.Lq >= 2048 && a.Lk >= 2048) return VQ_ATTN_K_FWD64D;
        // 32 queries per wave, four waves per SIMD (attn_fwd32d_kernel)
        if (off32 && a.Lq >= 192) return VQ_ATTN_K_FWD32D;
        return a.Lq >= 192 ? VQ_ATTN_K_FWD8_NW8 : VQ_ATTN_K_FWD8_NW4;
    }
    return VQ_ATTN_K_FWD;
}

// R[0, n) = 0 in front of a static-grid launch.  A kernel, not hipMemsetAsync: captured into a graph by the runtime of
// ROCm 7.2 the memset took effect in no replay (R kept growing from replay to replay; measured, GPU test
// test_switched_on_forward_replays_from_a_graph replays twice), a kernel node does.
__global__ void attn_zero_rows_kernel(int32_t* R, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) R[i] = 0;
}

// A = AttnQSArgs (vq_attn_fwd_rowquant_static): the static-grid form of the route's kernel; the routes without one
// (attn_fwd8_kernel, attn_cross_reg_kernel) return VQ_EUNSUP before any HIP call, the others zero R first on the same
// stream (every head adds its part of a row's term - attn_quant_rows).
template <int D, class A>
static int launch_attn(const A& a, hipStream_t st) {
    constexpr bool ST = std::is_same<A, AttnQSArgs>::value;
    const int route = attn_route<D>(a);
    if constexpr (ST) {
        if (route == VQ_ATTN_K_CROSS_REG || route == VQ_ATTN_K_FWD8_NW8 || route == VQ_ATTN_K_FWD8_NW4) return VQ_EUNSUP;
        const int rows = a.n_seq * a.Lq;
        hipLaunchKernelGGL(attn_zero_rows_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, a.R, rows);
        if (const int rc = vq_check_launch()) return rc;
    }
    switch (route) {
        case VQ_ATTN_K_CROSS32_2: return launch_cross32<D>(a, st);
        case VQ_ATTN_K_CROSS32_3: if constexpr (D >= 64) return launch_cross32<D, 3>(a, st); break;
        case VQ_ATTN_K_CROSS32_4: if constexpr (D >= 64) return launch_cross32<D, 4>(a, st); break;
        case VQ_ATTN_K_CROSS32_5: if constexpr (D >= 64) return launch_cross32<D, 5>(a, st); break;
        case VQ_ATTN_K_CROSS_REG: if constexpr (!ST) return launch_cross_reg(a, st); break;
        case VQ_ATTN_K_FWD64D: return launch_attn64d<D>(a, st);
        case VQ_ATTN_K_FWD32D: return launch_attn32d<D>(a, st);
        case VQ_ATTN_K_FWD8_NW8: if constexpr (!ST) return launch_attn8<D, 8>(a, st); break;
        case VQ_ATTN_K_FWD8_NW4: if constexpr (!ST) return launch_attn8<D, 4>(a, st); break;
        case VQ_ATTN_K_FWD: {
            using C = AttCfg<D>;
            constexpr auto k = attn_fwd_kernel<D, A>;
            if (const int rc = vq_prepare_kernel<k>(C::LDS)) return rc;
            dim3 grid((a.Lq + 127) / 128, a.H, a.n_seq);
            hipLaunchKernelGGL(k, grid, dim3(256), C::LDS, st, a);
            return vq_check_launch();
        }
        default: break;
    }
    return VQ_EUNSUP;     // (a route without a kernel for this head dim: attn_route never returns one)
}

// Argument checks of vq_attn_fwd / vq_attn_fwd_route (no dereference, no HIP call): VQ_OK with *a filled, or the error code.
// o_optional: vq_attn_fwd_rowquant_static, whose fp16 output is a copy for callers that need both.
static int attn_fwd_args(const void* q, const void* k, const void* v, void* o, int n_seq, int Lq, int Lk, int H,
                         long q_seq_stride, long q_tok_stride, long kv_seq_stride, long kv_tok_stride,
                         long o_seq_stride, long o_tok_stride, const int32_t* kv_off, float scale, AttnArgs* a,
                         bool o_optional = false) {
    if (!q || !k || !v || (!o && !o_optional)) return VQ_EINVAL;
    if (n_seq <= 0 || Lq <= 0 || H <= 0 || (Lk <= 0 && !kv_off)) return VQ_EINVAL;
    if ((q_tok_stride | kv_tok_stride | o_tok_stride | q_seq_stride | kv_seq_stride | o_seq_stride) % 8 != 0)
        return VQ_ESHAPE;  // 16-byte alignment of every row
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 != 0) return VQ_ESHAPE;   // ... and of its base
    if (n_seq > 65535 || H > 65535) return VQ_ESHAPE;
    *a = AttnArgs{(const half_t*)q, (const half_t*)k, (const half_t*)v, (half_t*)o, q_seq_stride, q_tok_stride,
                  kv_seq_stride, kv_tok_stride, o_seq_stride, o_tok_stride, kv_off, n_seq, Lq, Lk, H,
                  scale * ATT_LOG2E};
    return VQ_OK;
}

extern "C" int vq_attn_fwd(const void* q, const void* k, const void* v, void* o, int n_seq, int Lq, int Lk, int H,
                           int D, long q_seq_stride, long q_tok_stride, long kv_seq_stride, long kv_tok_stride,
                           long o_seq_stride, long o_tok_stride, const int32_t* kv_off, float scale, void* stream) {
    AttnArgs a;
    const int rc = attn_fwd_args(q, k, v, o, n_seq, Lq, Lk, H, q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride,
                                 o_seq_stride, o_tok_stride, kv_off, scale, &a);
    if (rc != VQ_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    return vq_dispatch_head_dim(D, [&](auto d) { return launch_attn<d()>(a, st); });
}

// Spatial / cross attention + the consuming Linear's STATIC (calibrated, tensor-wise) quantizer: the static-grid forms of
// attn_fwd_kernel, attn_fwd32d_kernel, attn_fwd64d_kernel and attn_cross32_kernel, chosen by the same attn_route.  Every
// check comes before any HIP call or dereference.
extern "C" int vq_attn_fwd_rowquant_static(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                                           const float* delta, const float* zp, int8_t* xq, float* sx, int32_t* zx,
                                           int32_t* R, void* o, int n_seq, int Lq, int Lk, int H, int D, long q_seq_stride,
                                           long q_tok_stride, long kv_seq_stride, long kv_tok_stride, long o_seq_stride,
                                           long o_tok_stride, const int32_t* kv_off, int Kp, int n_bits, float scale,
                                           void* stream) {
    if (!delta || !zp || !xq || !sx || !zx || !R) return VQ_EINVAL;
    if ((s != nullptr) != (s_rcp != nullptr)) return VQ_EINVAL;     // the division exists in reciprocal form only
    if (D <= 0 || Kp <= 0) return VQ_EINVAL;
    AttnQSArgs a{};
    const int rc = attn_fwd_args(q, k, v, o, n_seq, Lq, Lk, H, q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride,
                                 o_seq_stride, o_tok_stride, kv_off, scale, &a, /*o_optional*/ true);
    if (rc != VQ_OK) return rc;
    if (Kp % 128 != 0 || Kp < (long)H * D || D % 4 != 0) return VQ_ESHAPE;
    // float4 reads of s / s_rcp, 8-byte code stores (16 bytes asked, as everywhere else)
    if (((uintptr_t)xq | (uintptr_t)s | (uintptr_t)s_rcp) % 16 != 0) return VQ_ESHAPE;
    if ((long)n_seq * Lq > 0x7fffffffL) return VQ_ESHAPE;            // rows are indexed with 32 bits
    if (n_bits < 2 || n_bits > 8) return VQ_EUNSUP;
    if (D != 72 && D != 64 && D != 32 && D != 16) return VQ_EUNSUP;  // (vq_dispatch_head_dim)
    a.s = s, a.s_rcp = s_rcp, a.delta = delta, a.zp = zp, a.xq = xq, a.sx = sx, a.zx = zx, a.R = R, a.Kp = Kp, a.n_bits = n_bits;
    hipStream_t st = (hipStream_t)stream;
    return vq_dispatch_head_dim(D, [&](auto d) { return launch_attn<d()>(a, st); });
}

extern "C" int vq_attn_fwd_route(const void* q, const void* k, const void* v, void* o, int n_seq, int Lq, int Lk, int H,
                                 int D, long q_seq_stride, long q_tok_stride, long kv_seq_stride, long kv_tok_stride,
                                 long o_seq_stride, long o_tok_stride, const int32_t* kv_off, float scale, void* stream) {
    (void)stream;
    AttnArgs a;
    const int rc = attn_fwd_args(q, k, v, o, n_seq, Lq, Lk, H, q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride,
                                 o_seq_stride, o_tok_stride, kv_off, scale, &a);
    if (rc != VQ_OK) return rc;
    return vq_dispatch_head_dim(D, [&](auto d) { return attn_route<d()>(a); });
}

template <int D>
static int launch_temporal(const TempArgs& a, hipStream_t st) {
    constexpr int LDS = 3 * 32 * (4 * D * 2 + 16);
    constexpr auto k = attn_temporal_kernel<D>;
    if (const int rc = vq_prepare_kernel<k>(LDS)) return rc;
    dim3 grid((a.S + 1) / 2, (a.H + 3) / 4, a.B);
    hipLaunchKernelGGL(k, grid, dim3(256), LDS, st, a);
    return vq_check_launch();
}

extern "C" int vq_attn_temporal(const void* q, const void* k, const void* v, void* o, int B, int T, int S, int H,
                                int D, long ld_in, long ld_out, float scale, void* stream) {
    if (!q || !k || !v || !o) return VQ_EINVAL;
    if (B <= 0 || T <= 0 || S <= 0 || H <= 0) return VQ_EINVAL;
    if (T > 16 || ld_in % 8 != 0 || ld_out % 8 != 0 || B > 65535) return VQ_ESHAPE;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 != 0) return VQ_ESHAPE;   // 16-byte loads (o: as vq_attn_temporal_long)
    TempArgs a{(const half_t*)q, (const half_t*)k, (const half_t*)v, (half_t*)o, ld_in, ld_out, B, T, S, H,
               scale * ATT_LOG2E};
    hipStream_t st = (hipStream_t)stream;
    return vq_dispatch_head_dim(D, [&](auto d) { return launch_temporal<d()>(a, st); });
}

// H = 16 heads, 32-bit byte offsets inside a position's rows: the instruction-trimmed kernel (round 6)
static bool temporal_quant_trimmed(const TempQArgs& a) {
    return a.H == 16 && a.Kp <= 2048 && (long)a.T * a.S * a.ld_in * 2 < (1l << 31) && (long)a.T * a.S * a.Kp < (1l << 31);
}

template <int D, class A>
static int launch_temporal_quant(const A& a, hipStream_t st, bool trimmed) {
    const int C = a.H * D;
    const int LDS = 16 * (C * 2 + 16) + 16 * (C + 16) + 3 * 1024;
    constexpr int LDS_MAX = 16 * (16 * 72 * 2 + 16) + 16 * (16 * 72 + 16) + 3 * 1024;
    constexpr auto k2 = attn_temporal_quant2_kernel<D, A>;
    constexpr auto k1 = attn_temporal_quant_kernel<D, A>;
    int ncu = 0;
    if (const int rc = trimmed ? vq_prepare_kernel<k2>(LDS_MAX, &ncu) : vq_prepare_kernel<k1>(LDS_MAX, &ncu)) return rc;
    // persistent: a 1024-thread workgroup at up to 128 VGPRs owns its CU; small problems get one position each
    const int npos = a.S * a.B;
    const int per_cu = a.H > 8 ? 1 : (LDS > 80 * 1024 ? 1 : (LDS > 52 * 1024 ? 2 : 3));
    const int grid = npos < ncu * per_cu ? npos : ncu * per_cu;
    hipLaunchKernelGGL(trimmed ? k2 : k1, dim3(grid), dim3(64 * a.H), LDS, st, a);
    return vq_check_launch();
}

// Argument checks of vq_attn_temporal_rowquant (no dereference, no HIP call): VQ_OK with *a filled, or the error code.
static int temporal_quant_args(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                               int8_t* xq, float* sx, int32_t* zx, int32_t* R, int32_t* status, void* o, int B,
                               int T, int S, int H, int D, long ld_in, int Kp, float scale, TempQArgs* a) {
    if (!q || !k || !v || !xq || !sx || !zx || !R) return VQ_EINVAL;
    if ((s != nullptr) != (s_rcp != nullptr)) return VQ_EINVAL;     // the division exists in reciprocal form only here
    if (B <= 0 || T <= 0 || S <= 0 || H <= 0) return VQ_EINVAL;
    const int C = H * D;
    if (T > 16 || H > 16 || ld_in % 8 != 0 || B > 65535 || C % 16 != 0 || Kp % 128 != 0 || Kp < C) return VQ_ESHAPE;
    if (16 * (C / 8) > 3 * 64 * H || D % 4 != 0) return VQ_ESHAPE;   // V staging registers of the kernel
    // 16-byte loads of q / k / v, float4 reads of s / s_rcp, 16-byte code stores; o: 16 bytes as everywhere else
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)xq | (uintptr_t)s | (uintptr_t)s_rcp | (uintptr_t)o) % 16 != 0)
        return VQ_ESHAPE;
    *a = TempQArgs{(const half_t*)q, (const half_t*)k, (const half_t*)v, xq, sx, zx, R, status, (half_t*)o, s, s_rcp, ld_in, /*ld_out*/ C,
                   B, T, S, H, Kp, scale * ATT_LOG2E};
    return VQ_OK;
}

extern "C" int vq_attn_temporal_rowquant(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                                         int8_t* xq, float* sx, int32_t* zx, int32_t* R, int32_t* status, void* o, int B,
                                         int T, int S, int H, int D, long ld_in, int Kp, float scale, void* stream) {
    TempQArgs a;
    if (const int rc = temporal_quant_args(q, k, v, s, s_rcp, xq, sx, zx, R, status, o, B, T, S, H, D, ld_in, Kp, scale, &a)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return vq_dispatch_head_dim(D, [&](auto d) { return launch_temporal_quant<d()>(a, st, temporal_quant_trimmed(a)); });
}

// The shared-grid forms of the two T <= 16 kernels: one workgroup per spatial position (of both samples).  LDS: the V tile,
// a code area per sample, the row statistics with a sum area per sample, and the parked fp16 output of each sample
// (8 bytes per thread and 16-dim tile): 160 512 of 163 840 B at H = 16, D = 72 - one workgroup per CU, as the dynamic form there.
template <int D>
static int launch_temporal_shared(const TempQPArgs& a, hipStream_t st, bool trimmed) {
    constexpr int KS = (D + 15) / 16;
    const int C = a.H * D;
    const int LDS = 16 * (C * 2 + 16) + 2 * 16 * (C + 16) + 4 * 1024 + 2 * KS * 64 * a.H * 8;
    constexpr int LDS_MAX = 16 * (16 * D * 2 + 16) + 2 * 16 * (16 * D + 16) + 4 * 1024 + 2 * KS * 64 * 16 * 8;
    constexpr auto k2 = attn_temporal_quant2_kernel<D, TempQPArgs>;
    constexpr auto k1 = attn_temporal_quant_kernel<D, TempQPArgs>;
    int ncu = 0;
    if (const int rc = trimmed ? vq_prepare_kernel<k2>(LDS_MAX, &ncu) : vq_prepare_kernel<k1>(LDS_MAX, &ncu)) return rc;
    // persistent: a 1024-thread workgroup owns its CU; smaller ones share its 160 KB of LDS, three at the most
    const int fit = 160 * 1024 / LDS;
    const int per_cu = a.H > 8 || fit < 2 ? 1 : (fit > 3 ? 3 : fit);
    const int grid = a.S < ncu * per_cu ? a.S : ncu * per_cu;
    hipLaunchKernelGGL(trimmed ? k2 : k1, dim3(grid), dim3(64 * a.H), LDS, st, a);
    return vq_check_launch();
}

// Temporal attention + attn_temp.proj's dynamic per-token quantizer for a joint forward: B <= 2 samples share a token's grid,
// n_bits 2..8.  Every check comes before any HIP call or dereference: null pointers and extents, then shapes, then the width.
extern "C" int vq_attn_temporal_rowquant_shared(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                                                int8_t* xq, float* sx, int32_t* zx, int32_t* R, int32_t* status, void* o,
                                                int B, int T, int S, int H, int D, long ld_in, int Kp, int n_bits,
                                                float scale, void* stream) {
    if (!q || !k || !v || !xq || !sx || !zx || !R) return VQ_EINVAL;
    if ((s != nullptr) != (s_rcp != nullptr)) return VQ_EINVAL;     // the division exists in reciprocal form only here
    if (B <= 0 || T <= 0 || S <= 0 || H <= 0 || D <= 0 || Kp <= 0) return VQ_EINVAL;
    TempQPArgs a{};
    if (const int rc = temporal_quant_args(q, k, v, s, s_rcp, xq, sx, zx, R, status, o, B, T, S, H, D, ld_in, Kp, scale, &a)) return rc;
    if (D != 72 && D != 64 && D != 32 && D != 16) return VQ_ESHAPE;  // (vq_dispatch_head_dim)
    if (B > 2) return VQ_ESHAPE;                                     // one workgroup holds a position of every sample
    if (n_bits < 2 || n_bits > 8) return VQ_EUNSUP;
    a.n_bits = n_bits;
    hipStream_t st = (hipStream_t)stream;
    return vq_dispatch_head_dim(D, [&](auto d) { return launch_temporal_shared<d()>(a, st, temporal_quant_trimmed(a)); });
}

template <int D, class A>
static int launch_temporal_long(const A& a, hipStream_t st) {
    constexpr int LDS_MAX = 16 * 64 * D * 2 + 64 + 3 * 1024;
    const int LDS = a.H * 64 * D * 2 + 64 + 3 * 1024;
    constexpr auto k = attn_temporal_long_kernel<D, A>;
    int ncu = 0;
    if (const int rc = vq_prepare_kernel<k>(LDS_MAX, &ncu)) return rc;
    // persistent: 16 heads x 150 KB of LDS own a CU; small head counts fit two workgroups
    const int npos = a.S * a.B;
    const int per_cu = (a.H <= 8 && 2 * LDS <= 160 * 1024) ? 2 : 1;
    const int grid = npos < ncu * per_cu ? npos : ncu * per_cu;
    hipLaunchKernelGGL(k, dim3(grid), dim3(64 * a.H), LDS, st, a);
    return vq_check_launch();
}

extern "C" int vq_attn_temporal_long(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                                     int8_t* xq, float* sx, int32_t* zx, int32_t* R, int32_t* status, void* o, int B,
                                     int T, int S, int H, int D, long ld_in, long ld_out, int Kp, float scale,
                                     void* stream) {
    if (!q || !k || !v || (!o && !xq)) return VQ_EINVAL;
    if (xq && (!sx || !zx || !R)) return VQ_EINVAL;
    if ((s != nullptr) != (s_rcp != nullptr)) return VQ_EINVAL;     // the division exists in reciprocal form only
    if (B <= 0 || T <= 0 || S <= 0 || H <= 0) return VQ_EINVAL;
    const long C = (long)H * D;
    if (T > 64 || H > 16 || B > 65535 || C % 16 != 0 || ld_in % 8 != 0) return VQ_ESHAPE;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 != 0) return VQ_ESHAPE;
    if (o && (ld_out % 8 != 0 || ld_out < C || (uintptr_t)o % 16 != 0)) return VQ_ESHAPE;
    if (((uintptr_t)s | (uintptr_t)s_rcp) % 16 != 0) return VQ_ESHAPE;    // read as float4 per 4 channels
    // per-token grids: one row statistic per (t, s), shared over the batch by the caller's contract
    if (xq && (B != 1 || Kp % 128 != 0 || Kp < C || (uintptr_t)xq % 16 != 0)) return VQ_ESHAPE;
    // 32-bit byte offsets of a position's rows
    if ((long)T * S * ld_in * 2 >= (1l << 31) || (xq && (long)T * S * Kp >= (1l << 31))) return VQ_ESHAPE;
    TempQArgs a{(const half_t*)q, (const half_t*)k, (const half_t*)v, xq, sx, zx, R, status, (half_t*)o, s, s_rcp, ld_in,
                ld_out, B, T, S, H, Kp, scale * ATT_LOG2E};
    hipStream_t st = (hipStream_t)stream;
    return vq_dispatch_head_dim(D, [&](auto d) { return launch_temporal_long<d()>(a, st); });
}

// Temporal attention + attn_temp.proj's STATIC (calibrated, tensor-wise) quantizer: the static-grid forms of the three
// kernels above.  Every check comes before any HIP call or dereference.
extern "C" int vq_attn_temporal_rowquant_static(const void* q, const void* k, const void* v, const float* s,
                                                const float* s_rcp, const float* delta, const float* zp, int8_t* xq,
                                                float* sx, int32_t* zx, int32_t* R, void* o, int B, int T, int S, int H,
                                                int D, long ld_in, long ld_out, int Kp, int n_bits, float scale,
                                                void* stream) {
    if (!q || !k || !v || !delta || !zp || !xq || !sx || !zx || !R) return VQ_EINVAL;
    if ((s != nullptr) != (s_rcp != nullptr)) return VQ_EINVAL;     // the division exists in reciprocal form only
    if (B <= 0 || T <= 0 || S <= 0 || H <= 0 || D <= 0 || Kp <= 0 || T > 64) return VQ_EINVAL;
    const long C = (long)H * D;
    const bool is_long = T > 16;
    if (D != 72 && D != 64 && D != 32 && D != 16) return VQ_ESHAPE;  // (vq_dispatch_head_dim)
    if (H > 16 || B > 65535 || C % 16 != 0 || ld_in % 8 != 0 || Kp % 128 != 0 || Kp < C) return VQ_ESHAPE;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)xq | (uintptr_t)s | (uintptr_t)s_rcp | (uintptr_t)o) % 16 != 0)
        return VQ_ESHAPE;
    // o: dense rows in the T <= 16 kernels, rows of stride ld_out in the long one
    if (o && (is_long ? (ld_out % 8 != 0 || ld_out < C) : ld_out != C)) return VQ_ESHAPE;
    // the long kernel: 32-bit byte offsets inside a position's rows
    if (is_long && ((long)T * S * ld_in * 2 >= (1l << 31) || (long)T * S * Kp >= (1l << 31))) return VQ_ESHAPE;
    if (n_bits < 2 || n_bits > 8) return VQ_EUNSUP;
    TempQSArgs a{};
    static_cast<TempQArgs&>(a) = TempQArgs{(const half_t*)q, (const half_t*)k, (const half_t*)v, xq, sx, zx, R, /*status*/ nullptr,
                                           (half_t*)o, s, s_rcp, ld_in, is_long ? ld_out : C, B, T, S, H, Kp, scale * ATT_LOG2E};
    a.delta = delta, a.zp = zp, a.n_bits = n_bits;
    hipStream_t st = (hipStream_t)stream;
    if (is_long) return vq_dispatch_head_dim(D, [&](auto d) { return launch_temporal_long<d()>(a, st); });
    return vq_dispatch_head_dim(D, [&](auto d) { return launch_temporal_quant<d()>(a, st, temporal_quant_trimmed(a)); });
}

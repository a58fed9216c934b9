// gemm_common.h - shared pieces of the int8 GEMM kernels: argument block, XCD-aware tile map, per-tile dequant
// parameter staging and the epilogues (plain, quantizing, cross-attention) of the kernels csrc/gemm_i8.hip ships.  Product
// forms only: the retired kernel generations and what they needed of this header live in tools/lab/gemm_common_lab.h.
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "vq_common.h"
#include "attn_rowquant.h"   // tq_isum4rows; rowquant_shared.h: rqs_grid / rqs_quant, the one copy of the static rounding rule
#include "attn_tile.h"       // the attention steps of the cross-attention epilogue (ring_epilogue_cross)

__device__ __forceinline__ float gelu_tanh_f(float x) {
    // nn.GELU(approximate='tanh'): 0.5*x*(1+tanh(u)), u = sqrt(2/pi)*(x+0.044715 x^3)
    //   = x * sigmoid(2u) = x / (1 + 2^(-2u*log2 e)):  3 fma/mul + v_exp_f32 + v_rcp_f32 (1 ulp each; the result
    // is rounded to fp16 right after) instead of an IEEE division and an exp with range reduction.
    const float x2 = x * x;
    const float w = x * fmaf(x2, -0.044715f * 2.302208198f, -2.302208198f);   // -2u*log2(e); 2*sqrt(2/pi)*log2(e) = 2.3022082
    const float e = __builtin_amdgcn_exp2f(w);                                 // +inf for very negative x -> y = -0
    return x * __builtin_amdgcn_rcpf(1.0f + e);
}

struct GemmArgs {
    const int8_t* xq;
    const float* sx;
    const int32_t* zx;
    const int32_t* R;
    const uint8_t* wq;
    const float* sw;
    const int32_t* zw;
    const int32_t* cs;
    const float* bias;
    half_t* out;
    const half_t* resid;
    const float* gate;
    int ldo, rows_per_gate, M, N, K, Kp, epilogue;
    int nkt_dbg;  // > 0: run only this many k-tiles (ablation for profiling; results are then wrong)
    // batched launch (vq_gemm_i8_batched): nbatch weight sets applied to the SAME activation; strides in elements
    // of the respective arrays (wq bytes, per-channel arrays, out halves)
    int nbatch;
    long bs_w, bs_ch, bs_out;
    // grouped launch (vq_gemm_i8_grouped): ngroups > 1 independent problems of one shape in ONE grid, group-major
    // (q / k / v Linears whose inputs were quantized against three smoothing vectors).  Group 0 is the fields above.
    int ngroups;
    struct Group {
        const int8_t* xq;
        const float* sx;
        const int32_t* zx;
        const int32_t* R;
        const uint8_t* wq;
        const float* sw;
        const int32_t* zw;
        const int32_t* cs;
        const float* bias;
        half_t* out;
    } grp[2];         // groups 1 and 2
};

// Workgroup -> tile map.  Workgroups are dealt round-robin to the 8 XCDs (bid % 8), each with its own 4 MiB
// L2, so XCD x takes a CONTIGUOUS range of the tile order below and the 32 tiles it runs at a time share
// operands through that L2.  Order: super-rows of SM token tiles; inside a super-row, groups of SN channel
// tiles, token tile fastest.  One round of an XCD is then a few token panels x a few weight panels, 3.7-3.8 MB
// at K = 1152 - instead of 2 token panels x ALL weight panels (5.9 MB at N = 4608, measured 8x over-fetch of the
// fc1 operands from the fabric: profiles/r01_hbm_traffic.md).  Bijective for any tile counts.
// SM x SN = 8 x 4.  Round 5 measured 4 x 8 and 16 x 2 against it inside the two-stream step (alternating on one box, twice):
// 4 x 8 shortens the GEMM launch average by 1-2 % (58.4 vs 59.0 us, 57.3 vs 58.5 us) at EQUAL step time and moves 8 % more
// fabric bytes per launch (169.6 vs 156.7 MB: the channel-heavy round re-fetches token panels), 16 x 2 loses 2 % of the
// step: 8 x 4 stays (profiles/r05_experiments.md).  VQ_XCD_SM / VQ_XCD_SN: A/B builds of other panel shapes.
#ifndef VQ_XCD_SM
#define VQ_XCD_SM 8
#endif
#ifndef VQ_XCD_SN
#define VQ_XCD_SN 4
#endif
__device__ __forceinline__ void xcd_tile(int bid, int MT, int NTl, int& mt, int& nt) {
    constexpr int SM = VQ_XCD_SM, SN = VQ_XCD_SN;
    const int T = MT * NTl;
    const int q8 = T / 8, r8 = T % 8, xcd = bid % 8, idx = bid / 8;
    const int t = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int per_sr = SM * NTl;
    const int sr = t / per_sr, rem = t - sr * per_sr;
    const int smr = MT - sr * SM < SM ? MT - sr * SM : SM;     // token tiles in this super-row
    const int per_g = smr * SN;
    const int ng = rem / per_g, r2 = rem - ng * per_g;
    mt = sr * SM + r2 % smr;
    nt = ng * SN + r2 / smr;
}

// ---------------------------------------------------------------------------------------------------------------
// Epilogue layer.  After the main loop the workgroup's LDS holds, in this order (EpiGeom, the one place that knows):
//   one fp16 slab per wave (its WTM x WTN block of the tile, row stride ROWB) | per-channel terms sw, P, Q, b (BN floats
//   each) | per-token terms sx, V, U (BM floats each); the quantizing epilogue parks the consuming Linear's smoothing vector
//   (s, 1/s) in the 8 * BN bytes in front of the channel terms.
// The zero-point terms are parked as fp32 PRODUCTS with the scale - P = sw * (-zw), Q = sw * cs per channel, V = sx * (-zx),
// U = sx * R per token - for the float form of the dequantisation (ring_dequant).
// ---------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int WAVES_M, int WAVES_N>
struct EpiGeom {
    static constexpr int NW = WAVES_M * WAVES_N, NT = 64 * NW;
    static constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;   // a wave's block of the tile
    static constexpr int TM = WTM / 16, TN = WTN / 16;             // ... in 16 x 16 accumulator quads
    static constexpr int ROWB = WTN * 2 + 16;                      // slab row stride in bytes (16 B aligned; pad 16: 2-way write conflicts)
    static constexpr int SLAB = WTM * ROWB;
    static constexpr int PAR_OFF = NW * SLAB;                      // channel terms behind the slabs
    static constexpr int ROW_OFF = PAR_OFF + 16 * BN;              // token terms behind them
    static constexpr int QS_OFF = PAR_OFF - 8 * BN;                // smoothing vector in front of them
    static constexpr int BYTES = ROW_OFF + 12 * BM;
    static_assert(BN <= NT && BM <= NT, "one channel and one token row per thread");
    static_assert(BYTES <= 163840, "LDS budget");
};

// Per-channel dequant parameters of a tile (sw, -zw, cs, bias) and per-token ones (sx, -zx, R): one channel and one token
// row per thread, loaded into registers behind the main loop and parked in LDS as the terms above.
struct ColParams {
    float sw, b;
    int nzw, cs;
};
template <int BN>
__device__ __forceinline__ ColParams ring_load_col_params(const GemmArgs& a, int n0, int tx, const float* gate_row) {
    ColParams c{0.f, 0.f, 0, 0};
    const int gn = n0 + tx;
    if (tx < BN && gn < a.N) {
        c.sw = a.sw[gn];
        c.nzw = -a.zw[gn];
        c.cs = a.cs[gn];
        c.b = a.bias ? a.bias[gn] : 0.f;
        if (gate_row) {                                // gate * (sx*sw*t + b): folded into the per-channel terms
            const float g = gate_row[gn];
            c.sw *= g;
            c.b *= g;
        }
    }
    return c;
}
template <int BM, int BN, int WAVES_M, int WAVES_N>
__device__ __forceinline__ void ring_park_col_params(const ColParams& c, uint8_t* smem, int tx) {
    constexpr int PAR_OFF = EpiGeom<BM, BN, WAVES_M, WAVES_N>::PAR_OFF;
    if (tx < BN) {
        reinterpret_cast<float*>(smem + PAR_OFF)[tx] = c.sw;
        reinterpret_cast<float*>(smem + PAR_OFF)[BN + tx] = c.sw * (float)c.nzw;
        reinterpret_cast<float*>(smem + PAR_OFF)[2 * BN + tx] = c.sw * (float)c.cs;
        reinterpret_cast<float*>(smem + PAR_OFF)[3 * BN + tx] = c.b;
    }
}

struct RowParams {
    float sx;
    int nzx, R;
};
template <int BM>
__device__ __forceinline__ RowParams ring_load_row_params(const GemmArgs& a, int m0, int tx) {
    RowParams r{0.f, 0, 0};
    if (tx < BM) {
        const int m = m0 + tx;
        const int mc = m < a.M ? m : a.M - 1;
        r.sx = a.sx[mc];
        r.nzx = -a.zx[mc];
        r.R = a.R[mc];
    }
    return r;
}
template <int BM, int BN, int WAVES_M, int WAVES_N>
__device__ __forceinline__ void ring_park_row_params(const RowParams& r, uint8_t* smem, int tx) {
    constexpr int ROW_OFF = EpiGeom<BM, BN, WAVES_M, WAVES_N>::ROW_OFF;
    if (tx < BM) {
        reinterpret_cast<float*>(smem + ROW_OFF)[tx] = r.sx;
        reinterpret_cast<float*>(smem + ROW_OFF)[BM + tx] = r.sx * (float)r.nzx;
        reinterpret_cast<float*>(smem + ROW_OFF)[2 * BM + tx] = r.sx * (float)r.R;
    }
}

// VQ_EPI_GATE_RESID: the gate row (sample) of a token tile when all its rows belong to ONE sample, else nullptr.
// With it the gate is folded into the staged per-channel scale and bias, and the store loop only adds the residual:
// the two 16-byte gate loads per lane in each of its 18 iterations cost 5 us per N = K = 1152 launch.
template <int BM>
__device__ __forceinline__ const float* ring_tile_gate_row(const GemmArgs& a, int m0) {
    if (a.epilogue != VQ_EPI_GATE_RESID) return nullptr;
    const int mlast = (m0 + BM < a.M ? m0 + BM : a.M) - 1;
    const int s0 = __builtin_amdgcn_readfirstlane(m0 / a.rows_per_gate);
    const int s1 = __builtin_amdgcn_readfirstlane(mlast / a.rows_per_gate);
    return s0 == s1 ? a.gate + (size_t)s0 * a.N : nullptr;
}

// ---------------------------------------------------------------------------------------------------------------
// Epilogue of an INTERIOR tile (all BM x BN outputs inside the matrix, N % 8 == 0, gate - if any - folded into the
// staged scale / bias): the same arithmetic and the same LDS-transposed store pattern as ring_epilogue below, minus
// everything a full tile does not need.  The general path spends ~1000 of its ~1700 instructions per wave on
// bounds checks (an exec-mask branch per store iteration), chunk -> (row, column) divisions and 64-bit address
// arithmetic, and the epilogue is instruction-issue bound (3.2 cycles per issued instruction over 2 waves per SIMD).
// Here: the chunk walk c -> c + 64 is an incremental (row, column) update, global accesses are SGPR base + 32-bit
// lane offset, and the residual add is v_pk_add_f16 (bit-identical to fp32 add + round: the sum of two fp16
// values whose exponents differ by <= 13 is exact in fp32, and beyond that the smaller one cannot move the rounding).
// ---------------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) _Float16 half2v;

// One output of the dequantisation, y = sx sw (acc - zw R - zx cs) + b, in floating point on the parked products V = sx (-zx),
// U = sx R, P = sw (-zw), Q = sw cs: y = (sx sw) float(acc) + (U P + (V Q + b)) - the compiler packs the four operations of
// neighbouring outputs into v_pk_mul_f32 / v_pk_fma_f32: 1 conversion + 4 packed fp32 operations per PAIR of outputs, 3.5
// VALU issue slots per output where the exact integer correction took 4.5, in a phase that is VALU-bound (144 outputs per
// lane, 4 cycles per wave-instruction, two waves per SIMD = the 6.5 k cycles the stamps show).  The three products are rounded
// separately - the terms are up to ~50 x the result, so outputs move by <= 2e-5 relative against the integer form, 1/25 of the
// fp16 rounding that follows (rel-L2 vs the fp32 reference unchanged, asserted by the GEMM tests).
__device__ __forceinline__ float ring_dequant(int acc, float sx, float V, float U, float sw, float P, float Q, float b) {
    return __builtin_fmaf(sx * sw, (float)acc, __builtin_fmaf(U, P, __builtin_fmaf(V, Q, b)));
}

// STORE = false: the tile stays parked in the waves' slabs (every slab row one token, WTN halves) and nothing is stored -
// the first step of ring_epilogue_cross, which consumes it there.
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, bool STORE = true>
__device__ __forceinline__ void ring_epilogue_interior(const GemmArgs& a, uint8_t* smem,
                                                       int4v (&acc)[BN / WAVES_N / 16][BM / WAVES_M / 16], int m0, int n0,
                                                       int tid) {
    using G = EpiGeom<BM, BN, WAVES_M, WAVES_N>;
    constexpr int WTM = G::WTM, WTN = G::WTN, TM = G::TM, TN = G::TN;
    constexpr int ROWB = G::ROWB, SLAB = G::SLAB, PAR_OFF = G::PAR_OFF;
    constexpr int CPR = WTN / 8, NCH = WTM * CPR, NITER = NCH / 64;
    constexpr int QS = 64 / CPR, RS = 64 % CPR;       // chunk c + 64: QS rows further (+1 on wrap), RS chunks to the right
    static_assert(NCH % 64 == 0 && CPR < 64, "whole passes");
    constexpr bool HAS_RES = (EPI == VQ_EPI_GATE_RESID || EPI == VQ_EPI_RESID);
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int frow = lane & 15, fc = lane >> 4;
    const float* l_sw = reinterpret_cast<const float*>(smem + PAR_OFF);
    const float* l_P = reinterpret_cast<const float*>(smem + PAR_OFF) + BN;
    const float* l_Q = reinterpret_cast<const float*>(smem + PAR_OFF) + 2 * BN;
    const float* l_b = reinterpret_cast<const float*>(smem + PAR_OFF) + 3 * BN;
    const float* l_sx = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN);
    const float* l_V = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN) + BM;
    const float* l_U = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN) + 2 * BM;
    uint8_t* slab = smem + wave * SLAB;
    // wave-uniform byte bases of this wave's 64 x WTN output block; lane offsets stay 32-bit
    const size_t tile_off = ((size_t)(m0 + wm * WTM) * a.ldo + (n0 + wn * WTN)) * 2;
    uint8_t* obase = reinterpret_cast<uint8_t*>(a.out) + tile_off;
    const uint8_t* rbase = reinterpret_cast<const uint8_t*>(a.resid) + tile_off;
    const int ldb = a.ldo * 2;                        // row pitch in bytes
    const int row0 = lane / CPR, cc0 = lane - row0 * CPR;
    const int step_g = QS * ldb + RS * 16, wrap_g = ldb - CPR * 16;   // + wrap_g when the column wraps
    constexpr int step_s = QS * ROWB + RS * 16, wrap_s = ROWB - CPR * 16;
    // Two half passes (rows 0..WTM/2-1, then the rest): the stores of the first half are in flight while the second half
    // is dequantised, instead of all VALU work first and all stores after it.
    constexpr int NH = (TM % 2 == 0 && NITER % 2 == 0 && ((WTM / 2) * CPR) % 64 == 0) ? 2 : 1;
    constexpr int TMH = TM / NH, NITH = NITER / NH;
    static_assert(STORE || !HAS_RES, "a parked tile: no residual");
    // the residual operand: requested during the dequant phase (its HBM latency hides under the VALU work)
    half8 rres[HAS_RES ? NITH : 1];
    int pcc = cc0;
    uint32_t pgo = (uint32_t)(row0 * ldb + cc0 * 16);
    auto fetch_res = [&](int it) {
        rres[it] = *reinterpret_cast<const half8*>(rbase + pgo);
        const bool w = pcc >= CPR - RS;
        pcc += w ? RS - CPR : RS;
        pgo += w ? step_g + wrap_g : step_g;
    };
    float sxm[TM];
    float Vm[TM], Um[TM];                             // V = sx * (-zx), U = sx * R
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int rl = wm * WTM + i * 16 + frow;
        sxm[i] = l_sx[rl];
        Vm[i] = l_V[rl];
        Um[i] = l_U[rl];
    }
    int cc = cc0;
    uint32_t go = (uint32_t)(row0 * ldb + cc0 * 16), so = (uint32_t)(row0 * ROWB + cc0 * 16);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nl = wn * WTN + j * 16 + 4 * fc;
            const float4v fsw_ = *reinterpret_cast<const float4v*>(l_sw + nl);
            const float4v fP = *reinterpret_cast<const float4v*>(l_P + nl);
            const float4v fQ = *reinterpret_cast<const float4v*>(l_Q + nl);
            const float4v fb = *reinterpret_cast<const float4v*>(l_b + nl);
#pragma unroll
            for (int i = h * TMH; i < (h + 1) * TMH; ++i) {
                half4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float y = ring_dequant(acc[j][i][e], sxm[i], Vm[i], Um[i], fsw_[e], fP[e], fQ[e], fb[e]);
                    if constexpr (EPI == VQ_EPI_GELU) y = gelu_tanh_f(y);
                    o[e] = (half_t)y;
                }
                *reinterpret_cast<half4*>(slab + (i * 16 + frow) * ROWB + (j * 16 + 4 * fc) * 2) = o;
            }
            if constexpr (HAS_RES) {
                constexpr int PER = (NITH + TN - 1) / TN;
#pragma unroll
                for (int u = 0; u < PER; ++u)
                    if (j * PER + u < NITH) fetch_res(j * PER + u);
            }
        }
        // store pass of this half: the wave's slab rows as row-major 16-byte chunks (same wave wrote them: LDS
        // operations are in order)
#pragma unroll
        for (int it = 0; STORE && it < NITH; ++it) {
            half8 y = *reinterpret_cast<const half8*>(slab + so);
            if constexpr (HAS_RES) {
                const half8 rr = rres[it];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const half2v s2 = half2v{y[2 * q], y[2 * q + 1]} + half2v{rr[2 * q], rr[2 * q + 1]};
                    y[2 * q] = s2[0];
                    y[2 * q + 1] = s2[1];
                }
            }
            *reinterpret_cast<half8*>(obase + go) = y;
            const bool w = cc >= CPR - RS;
            cc += w ? RS - CPR : RS;
            go += w ? step_g + wrap_g : step_g;
            so += w ? step_s + wrap_s : step_s;
        }
    }
}

// Shared epilogue of the LDS-DMA ring kernels (called after the workgroup barrier that publishes the parked terms; uses all of
// smem).
// INTERIOR_ONLY: the launcher guarantees what the interior path needs for EVERY tile (interior tiles, 8-element aligned rows,
// the gate folded into the staged scales) - the general path below is then not even compiled into the kernel: the resid
// epilogues' 18 x 16-byte residual registers of that path were what put those kernels at 244 VGPRs (round 5).
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, bool INTERIOR_ONLY>
__device__ __forceinline__ void ring_epilogue(const GemmArgs& a, uint8_t* smem,
                                              int4v (&acc)[BN / WAVES_N / 16][BM / WAVES_M / 16], int m0, int n0,
                                              long long* ts, int tid, bool gate_folded) {
    // gate_folded (workgroup-uniform): VQ_EPI_GATE_RESID with the gate already inside the staged scale / bias
    // ts: the stamped kernel's stamp block of this wave, else nullptr
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    constexpr int TM = WTM / 16, TN = WTN / 16;
    const int lane = tid & 63;
    if constexpr ((BM / WAVES_M) * (BN / WAVES_N / 8) % 64 == 0) {
        if constexpr (INTERIOR_ONLY) {
            ring_epilogue_interior<BM, BN, WAVES_M, WAVES_N, EPI>(a, smem, acc, m0, n0, tid);
            return;
        }
        // workgroup-uniform: every tile of the benchmark shapes is interior and takes the lean path
        const bool interior = m0 + BM <= a.M && n0 + BN <= a.N && (a.N & 7) == 0 && (a.ldo & 7) == 0 &&
                              (EPI != VQ_EPI_GATE_RESID || gate_folded);
        if (!ts && interior) {
            ring_epilogue_interior<BM, BN, WAVES_M, WAVES_N, EPI>(a, smem, acc, m0, n0, tid);
            return;
        }
    }
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int frow = lane & 15, fc = lane >> 4;
    // ---- epilogue: dequantise in the MFMA layout, transpose through LDS, store whole row runs ----
    // The v2 epilogue stored 8 bytes per lane (16 rows x 32 B per instruction) and reached 2.9 TB/s of
    // output; a plain fill of the same buffer runs at 5-6.4 TB/s (tools/write_bw.py).  Here every wave
    // parks its 64 x WTN fp16 sub-tile in its own LDS slab (row stride ROWB), then re-reads it as 16-byte
    // chunks in row-major order, so one store instruction covers contiguous WTN*2-byte runs of ~3.5 rows;
    // the residual / gate operands of the fused adds are read with the same coalesced pattern.
    using G = EpiGeom<BM, BN, WAVES_M, WAVES_N>;
    constexpr int ROWB = G::ROWB, SLAB = G::SLAB, PAR_OFF = G::PAR_OFF;
    const float* l_sw = reinterpret_cast<const float*>(smem + PAR_OFF);
    const float* l_P = reinterpret_cast<const float*>(smem + PAR_OFF) + BN;
    const float* l_Q = reinterpret_cast<const float*>(smem + PAR_OFF) + 2 * BN;
    const float* l_b = reinterpret_cast<const float*>(smem + PAR_OFF) + 3 * BN;
    const float* l_sx = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN);
    const float* l_V = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN) + BM;
    const float* l_U = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN) + 2 * BM;
    uint8_t* slab = smem + wave * SLAB;
    if (ts) ts[3] = __builtin_readcyclecounter();
    constexpr int CPR = WTN / 8;                      // 16-byte chunks per slab row
    constexpr int NCH = WTM * CPR;
    constexpr int NITER = (NCH + 63) / 64;
    const int mrow0 = m0 + wm * WTM, ncol0 = n0 + wn * WTN;
    // residual operand of the fused adds: this lane's chunks are requested DURING the dequant phase, two per finished
    // channel tile (whose 16 accumulator registers they inherit), so that the ~3 us of VALU work covers their HBM
    // latency; requested one unrolled batch at a time inside the store loop they cost +8..10 us per launch
    constexpr bool HAS_RES = (EPI == VQ_EPI_GATE_RESID || EPI == VQ_EPI_RESID);
    half8 rres[HAS_RES ? NITER : 1];
    auto fetch_res = [&](int it) {
        const int c = lane + it * 64;
        const int row = c / CPR, col = (c % CPR) * 8;
        const int m = mrow0 + row, n = ncol0 + col;
#pragma unroll
        for (int q = 0; q < 8; ++q) rres[it][q] = (half_t)0.f;
        if (c < NCH && m < a.M && n < a.N) {
            const size_t off = (size_t)m * a.ldo + n;
            if (n + 8 <= a.N) rres[it] = *reinterpret_cast<const half8*>(a.resid + off);
            else {
                const half4 r4 = *reinterpret_cast<const half4*>(a.resid + off);
#pragma unroll
                for (int q = 0; q < 4; ++q) rres[it][q] = r4[q];
            }
        }
    };
    {
        float sxm[TM];
        float Vm[TM], Um[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int rl = wm * WTM + i * 16 + frow;
            sxm[i] = l_sx[rl];
            Vm[i] = l_V[rl];
            Um[i] = l_U[rl];
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nl = wn * WTN + j * 16 + 4 * fc;
            const float4v fsw_ = *reinterpret_cast<const float4v*>(l_sw + nl);
            const float4v fP = *reinterpret_cast<const float4v*>(l_P + nl);
            const float4v fQ = *reinterpret_cast<const float4v*>(l_Q + nl);
            const float4v fb = *reinterpret_cast<const float4v*>(l_b + nl);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                half4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float y = ring_dequant(acc[j][i][e], sxm[i], Vm[i], Um[i], fsw_[e], fP[e], fQ[e], fb[e]);
                    if constexpr (EPI == VQ_EPI_GELU) y = gelu_tanh_f(y);
                    o[e] = (half_t)y;
                }
                *reinterpret_cast<half4*>(slab + (i * 16 + frow) * ROWB + (j * 16 + 4 * fc) * 2) = o;
            }
            if constexpr (HAS_RES) {
                constexpr int PER = (NITER + TN - 1) / TN;
#pragma unroll
                for (int u = 0; u < PER; ++u)
                    if (j * PER + u < NITER) fetch_res(j * PER + u);
            }
        }
    }
    if (ts) ts[4] = __builtin_readcyclecounter();
    // second pass: this wave's slab, row-major 16-byte chunks (same wave wrote it: LDS ops are in order)
#pragma unroll
    for (int it = 0; it < NITER; ++it) {
        const int c = lane + it * 64;
        if (NCH % 64 != 0 && c >= NCH) continue;
        const int row = c / CPR, col = (c % CPR) * 8;
        const int m = mrow0 + row, n = ncol0 + col;
        if (m >= a.M || n >= a.N) continue;
        half8 y = *reinterpret_cast<const half8*>(slab + row * ROWB + col * 2);
        const size_t off = (size_t)m * a.ldo + n;
        const bool full = n + 8 <= a.N;               // N % 4 == 0: otherwise exactly 4 valid
        if constexpr (EPI == VQ_EPI_GATE_RESID || EPI == VQ_EPI_RESID) {
            const half8 rr = rres[it];
            if (EPI == VQ_EPI_GATE_RESID && !gate_folded) {
                const float* g = a.gate + (size_t)(m / a.rows_per_gate) * a.N + n;
                const float4v g0 = *reinterpret_cast<const float4v*>(g);
                const float4v g1 = full ? *reinterpret_cast<const float4v*>(g + 4) : float4v{0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < 8; ++q) y[q] = (half_t)((float)rr[q] + (q < 4 ? g0[q] : g1[q - 4]) * (float)y[q]);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) y[q] = (half_t)((float)rr[q] + (float)y[q]);
            }
        }
        if (full) *reinterpret_cast<half8*>(a.out + off) = y;
        else {
            half4 y4;
#pragma unroll
            for (int q = 0; q < 4; ++q) y4[q] = y[q];
            *reinterpret_cast<half4*>(a.out + off) = y4;
        }
    }
    if (ts) {
        ts[5] = __builtin_readcyclecounter();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ts[6] = __builtin_readcyclecounter();
        ts[8] = wall_clock64();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Quantizing epilogue (vq_gemm_i8_rowquant_static): GELU(tanh), rounded to fp16 as VQ_EPI_GELU stores it, then the
// STATIC tensor-wise quantizer of the Linear that consumes the output - never the fp16 matrix itself.  (delta, zp) is known
// before the launch, so every accumulator element is quantized where it sits; only the integer row sum crosses waves
// and workgroups (one relaxed agent-scope atomic per row and wave: integer adds commute, R is bit-reproducible).
// Internal epilogue id of the kernel templates; vq_gemm_i8 does not accept it.
// ---------------------------------------------------------------------------------------------------------------
#define VQ_EPI_GELU_QUANT 8
struct GemmQArgs : GemmArgs {
    const float* qs;       // smoothing vector of the consuming Linear per output column [N], or null
    const float* qs_rcp;   // RN(1 / qs) (set whenever qs is)
    const float* qdelta;   // one fp32 each, read on the device
    const float* qzp;
    int8_t* qxq;           // [M, Kp_out] codes - cx, pad columns [N, Kp_out) zero
    float* qsx;
    int32_t* qzx;
    int32_t* qR;           // zeroed in front of the launch
    int Kp_out, n_bits;
};

// The smoothing vector of a tile's BN columns travels like the channel parameters: one column per thread, loaded with them,
// parked in the 8 * BN bytes in front of the parameter block (EpiGeom::QS_OFF).  The codes' slabs (below) end far in front of it.
struct SmoothParams {
    float s, r;
};
template <int BN>
__device__ __forceinline__ SmoothParams ring_load_smooth(const GemmQArgs& a, int n0, int tid) {
    SmoothParams p{1.0f, 1.0f};
    if (a.qs && tid < BN && n0 + tid < a.N) {
        p.s = a.qs[n0 + tid];
        p.r = a.qs_rcp[n0 + tid];
    }
    return p;
}
template <int BM, int BN, int WAVES_M, int WAVES_N>
__device__ __forceinline__ void ring_park_smooth(const GemmQArgs& a, const SmoothParams& p, uint8_t* smem, int tid) {
    constexpr int QS_OFF = EpiGeom<BM, BN, WAVES_M, WAVES_N>::QS_OFF;
    if (a.qs && tid < BN) {
        reinterpret_cast<float*>(smem + QS_OFF)[tid] = p.s;
        reinterpret_cast<float*>(smem + QS_OFF)[BN + tid] = p.r;
    }
}

// Called like ring_epilogue (after the barrier that publishes the parameter blocks, which lie where the fp16 epilogues keep
// them).  A lane holds four consecutive columns of one row per (i, j): rqs_quant<4> -> one dword of codes, written to the
// wave's LDS slab, which is LINEAR (row pitch WTN bytes, no pad: 2-way write conflicts as the fp16 slabs have, conflict-free
// 16-byte reads); the store pass moves it as 16-byte chunks of 16 codes, WTN / 16 per row.  INTERIOR: every tile of the
// launch lies inside the matrix (the launcher checks) - no bounds in the kernel.  Otherwise columns >= N and rows >= M
// neither store nor count (N % 8 == 0: a lane's four columns and a chunk's halves are inside or outside together).
// sx / zx: the workgroups of the first column tile; pad columns: those of the last.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool INTERIOR>
__device__ __forceinline__ void ring_epilogue_quant(const GemmQArgs& a, uint8_t* smem,
                                                    int4v (&acc)[BN / WAVES_N / 16][BM / WAVES_M / 16], int m0, int n0,
                                                    int tid) {
    constexpr int NW = WAVES_M * WAVES_N, NT = 64 * NW;
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    constexpr int TM = WTM / 16, TN = WTN / 16;
    constexpr int PAR_OFF = EpiGeom<BM, BN, WAVES_M, WAVES_N>::PAR_OFF, QS_OFF = EpiGeom<BM, BN, WAVES_M, WAVES_N>::QS_OFF;
    constexpr int SLAB = WTM * WTN;
    constexpr int CPR = WTN / 16, NCH = WTM * CPR, NITER = (NCH + 63) / 64;
    static_assert(WTN % 16 == 0 && NW * SLAB <= QS_OFF, "whole chunks; slabs in front of the smoothing vector");
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int frow = lane & 15, fc = lane >> 4;
    const float* l_sw = reinterpret_cast<const float*>(smem + PAR_OFF);
    const float* l_P = reinterpret_cast<const float*>(smem + PAR_OFF) + BN;
    const float* l_Q = reinterpret_cast<const float*>(smem + PAR_OFF) + 2 * BN;
    const float* l_b = reinterpret_cast<const float*>(smem + PAR_OFF) + 3 * BN;
    const float* l_sx = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN);
    const float* l_V = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN) + BM;
    const float* l_U = reinterpret_cast<const float*>(smem + PAR_OFF + 16 * BN) + 2 * BM;
    const float* l_qs = reinterpret_cast<const float*>(smem + QS_OFF);
    uint8_t* slab = smem + wave * SLAB;
    const int mrow0 = m0 + wm * WTM, ncol0 = n0 + wn * WTN;

    const RqWidth wd = rq_width(a.n_bits);
    RqsGrid g = rqs_grid(a.qdelta, a.qzp, 0, wd.qmax);
    g.delta = tq_uniform(g.delta), g.zp = tq_uniform(g.zp), g.inv = tq_uniform(g.inv), g.thr = tq_uniform(g.thr);
    const bool smooth = a.qs != nullptr;              // kernel-uniform

    float sxm[TM];
    float Vm[TM], Um[TM];                             // V = sx * (-zx), U = sx * R
    uint32_t csum[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int rl = wm * WTM + i * 16 + frow;
        sxm[i] = l_sx[rl];
        Vm[i] = l_V[rl];
        Um[i] = l_U[rl];
        csum[i] = 0;
    }
    // one kernel-uniform branch on the code width and one on the smoothing vector around the whole phase
    auto phase = [&](auto sat8, auto sm) {
        constexpr bool SAT8_ = decltype(sat8)::value, SM_ = decltype(sm)::value;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nl = wn * WTN + j * 16 + 4 * fc;
            const float4v fsw_ = *reinterpret_cast<const float4v*>(l_sw + nl);
            const float4v fP = *reinterpret_cast<const float4v*>(l_P + nl);
            const float4v fQ = *reinterpret_cast<const float4v*>(l_Q + nl);
            const float4v fb = *reinterpret_cast<const float4v*>(l_b + nl);
            float4v s4 = {1.f, 1.f, 1.f, 1.f}, r4 = {1.f, 1.f, 1.f, 1.f};
            if constexpr (SM_) {
                s4 = *reinterpret_cast<const float4v*>(l_qs + nl);
                r4 = *reinterpret_cast<const float4v*>(l_qs + BN + nl);
            }
            const bool col_ok = INTERIOR || n0 + nl < a.N;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                float x4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float y = ring_dequant(acc[j][i][e], sxm[i], Vm[i], Um[i], fsw_[e], fP[e], fQ[e], fb[e]);
                    y = gelu_tanh_f(y);
                    x4[e] = (float)(half_t)y;         // the value VQ_EPI_GELU stores: the quantizer's input
                    if constexpr (SM_) x4[e] = rq_div_rcp(x4[e], s4[e], r4[e]);
                }
                uint32_t pk[1];
                rqs_quant<4, SAT8_>(x4, g, wd.qmax, pk);
                const uint32_t cs1 = __builtin_amdgcn_sad_u8(pk[0], 0u, csum[i]);
                csum[i] = col_ok ? cs1 : csum[i];
                asm volatile("" : "+v"(csum[i]));     // summed HERE: left to the scheduler, the codes were held (spilled) to the end of the phase
                *reinterpret_cast<uint32_t*>(slab + (i * 16 + frow) * WTN + j * 16 + 4 * fc) = pk[0] ^ wd.flip;
            }
        }
    };
    if (wd.qmax == 255.0f) {
        if (smooth) phase(std::true_type{}, std::true_type{});
        else phase(std::true_type{}, std::false_type{});
    } else {
        if (smooth) phase(std::false_type{}, std::true_type{});
        else phase(std::false_type{}, std::false_type{});
    }
    // store pass: this wave's slab as row-major 16-byte chunks (same wave wrote it: LDS operations are in order); the last
    // pass is masked where the slab is no whole number of passes (32-row wave tiles: 288 chunks)
    {
        uint8_t* obase = reinterpret_cast<uint8_t*>(a.qxq) + ((size_t)mrow0 * a.Kp_out + ncol0);   // wave-uniform
#pragma unroll
        for (int it = 0; it < NITER; ++it) {
            const int c = lane + it * 64;
            if (NCH % 64 != 0 && it == NITER - 1 && c >= NCH) continue;
            const int row = c / CPR, cc = c - row * CPR;
            const int4v v = *reinterpret_cast<const int4v*>(slab + c * 16);
            uint8_t* dst = obase + (uint32_t)(row * a.Kp_out + cc * 16);
            if constexpr (INTERIOR) {
                *reinterpret_cast<int4v*>(dst) = v;
            } else {
                const int n = ncol0 + cc * 16;
                if (mrow0 + row < a.M) {
                    if (n + 16 <= a.N) *reinterpret_cast<int4v*>(dst) = v;
                    else if (n + 8 <= a.N) *reinterpret_cast<int2v*>(dst) = int2v{v[0], v[1]};
                }
            }
        }
    }
    // row terms: this wave's columns of R = sum(raw codes) - N * (int)zp, reduced over the four column groups of a row
    {
        const int izp = (int)g.zp;
        const int ncw = INTERIOR ? WTN : (a.N - ncol0 < WTN ? a.N - ncol0 : WTN);   // this wave's columns inside the matrix
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int rs = tq_isum4rows((int)csum[i]);
            const int m = mrow0 + i * 16 + frow;
            if (fc == 0 && (INTERIOR || m < a.M) && ncw > 0) {
                __hip_atomic_fetch_add(a.qR + m, rs - ncw * izp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (ncol0 == 0) {
                    a.qsx[m] = g.delta;
                    a.qzx[m] = izp - wd.cx;
                }
            }
        }
    }
    // pad columns [N, Kp_out) of the tile's rows, zeroed like the row quantizers do (8-byte steps: N % 8 == 0)
    if (n0 + BN >= a.N) {
        const int padc = (a.Kp_out - a.N) >> 3;
        for (int idx = tid; idx < BM * padc; idx += NT) {
            const int row = idx / padc, c = idx - row * padc;
            if (INTERIOR || m0 + row < a.M)
                *reinterpret_cast<int2v*>(a.qxq + ((size_t)(m0 + row) * a.Kp_out + a.N + c * 8)) = int2v{0, 0};
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Cross-attention epilogue (vq_gemm_i8_cross_attn): the tile is cross_attn.q_linear's output, and the workgroup holds
// everything its (query, head) pairs need - a 256 x 288 tile is 256 queries x 4 heads of 72, a wave's 64 x 144 block
// 2 heads x 2 blocks of 32 queries, and the keys are the prompt's <= 128 tokens - so attention runs here and q is never
// written.  att_o is bit-identical to vq_gemm_i8(VQ_EPI_NONE) followed by vq_attn_fwd (attn_cross32_kernel<72, 8, 2>):
//   1. the tile is dequantised, rounded to fp16 and parked in the waves' slabs by the one copy of that step
//      (ring_epilogue_interior<STORE = false>, the expression of the plain epilogue);
//   2. every wave reads its own slab rows back as the B-operand fragments of its 2 heads x 2 query blocks (attn_q_frags
//      on a slab row: 80 VGPRs; the int32 accumulators are dead);
//   3. workgroup barrier: slabs and ring are free.  K | V of a head travel by LDS-DMA as the two 64-key images of
//      attn_cross32_kernel (AttnKvDma, zero fill past the last key, ones column by attn_fill_pad): 42 KiB per head, so
//      four heads (168 KiB) do not fit the 160 KiB of a CU and three (126 KiB) do.  Two phases, one head per wave column
//      each: slots A, B, C receive the tile's heads 0, 2, 1 at once; phase 0 runs heads 0 | 2 (wave columns 0 | 1) from
//      A | B; behind it head 3 goes into A, and phase 1 runs heads 1 | 3 from C | A.  So of phase 1's two heads one is
//      delivered under phase 0's arithmetic and the other has to wait for the slot phase 0 frees: a fourth slot is what
//      LDS does not allow.
//   4. a (head, 32-query block) unit is attn_cross32_kernel's walk of one query tile: the 32-key half tiles in order,
//      the same steps of attn_tile.h, the same 32 queries per rescale decision (query blocks start at multiples of 32 of
//      the sample's tokens in both kernels), attn_store_rows straight to att_o.
// No spin, no atomics, no traffic between workgroups.
// ---------------------------------------------------------------------------------------------------------------
#define VQ_EPI_CROSS_ATTN 9
struct GemmXArgs : GemmArgs {
    AttnArgs at;           // k, v, o with their strides, kv_off, Lq (tokens per sample), Lk (<= 128), H, c; q unused
};

template <int BM, int BN, int WAVES_M, int WAVES_N>
__device__ __forceinline__ void ring_epilogue_cross(const GemmArgs& a, const AttnArgs& at, uint8_t* smem,
                                                    int4v (&acc)[BN / WAVES_N / 16][BM / WAVES_M / 16], int m0, int n0, int tid) {
    constexpr int D = 72, NW = WAVES_M * WAVES_N;
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    constexpr int HPW = WTN / D, QB = WTM / 32;                    // heads and 32-query blocks of a wave's block
    static_assert(WTN % D == 0 && WTM % 32 == 0 && HPW == 2 && WAVES_N == 2, "two phases of one head per wave column");
    // the image geometry of attn_cross32_kernel<72, 8, 2> (Att8Cfg<72, 8> of attention.hip)
    constexpr int KS = (D + 15) / 16, DT = (D + 32) / 32, KROW = ((D / 8) | 1) * 16, VRB = 192;
    constexpr int KT = 64, NT = 2, KTB = KT * KROW, VT = KT * VRB, SLOT = NT * (KTB + VT);
    constexpr int ROWB = EpiGeom<BM, BN, WAVES_M, WAVES_N>::ROWB, SLAB = EpiGeom<BM, BN, WAVES_M, WAVES_N>::SLAB;   // the waves' fp16 slabs
    static_assert(3 * SLOT <= NW * SLAB, "three head slots inside the vacated slabs");
    static_assert(D * 2 + 2 <= VRB && DT * 64 <= VRB, "dims + ones column inside a row; every 32-dim tile readable");
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int g = lane >> 5, l31 = lane & 31;

    // 1. dequantise + park
    ring_epilogue_interior<BM, BN, WAVES_M, WAVES_N, VQ_EPI_NONE, false>(a, smem, acc, m0, n0, tid);
    // 2. q fragments of this wave's units from its own slab (same wave wrote it: LDS operations are in order)
    half8 qf[HPW][QB][KS];
    {
        const uint8_t* slab = smem + wave * SLAB;
#pragma unroll
        for (int hh = 0; hh < HPW; ++hh)
#pragma unroll
            for (int b = 0; b < QB; ++b)
                attn_q_frags<D>(reinterpret_cast<const half_t*>(slab + (b * 32 + l31) * ROWB + hh * D * 2), g, qf[hh][b]);
#pragma unroll
        for (int hh = 0; hh < HPW; ++hh)
#pragma unroll
            for (int b = 0; b < QB; ++b)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[hh][b][ks]));   // read HERE, in front of the barrier
    }
    // 3. the slabs are free once every wave holds its fragments
    attn_wg_barrier();
    const int seq = __builtin_amdgcn_readfirstlane(m0 / at.Lq);    // all rows of the tile belong to one sample (launcher)
    const int h0 = n0 / D;                                         // the tile's first head
    const int strideB = (int)at.kv_tok_stride * 2;
    AttnKvDma<D, NW, KT, KROW, VRB> dma;
    dma.init(wave, lane, strideB);
    const unsigned lds0 = attn_lds_addr(smem);
    int kv_len = 0;
    auto deliver = [&](int hl, int slot) __attribute__((always_inline)) {   // head h0 + hl -> slot
        const half_t* kbase;
        const half_t* vbase;
        kv_len = attn_kv_base<D>(at, seq, h0 + hl, kbase, vbase, NT * KT);   // host guarantees <= 128
        const unsigned nrec = kv_len > 0 ? (unsigned)(kv_len - 1) * (unsigned)strideB + D * 2 : 0u;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
            dma.template issue<true>(kbase, vbase, (unsigned)kt * (unsigned)KT * (unsigned)strideB, nrec,
                                     lds0 + slot * SLOT + kt * KTB, lds0 + slot * SLOT + NT * KTB + kt * VT, wave);
    };
    deliver(0, 0);
    deliver(2, 1);
    deliver(1, 2);
#pragma unroll
    for (int s = 0; s < 3; ++s) attn_fill_pad<D, VRB>(smem + s * SLOT + NT * KTB, NT * KT, tid, 64 * NW);
    attn_wg_barrier();                                             // heads 0, 2, 1 have landed
    const int nhalf = (kv_len + 31) / 32;                          // 32-key half tiles that hold keys (wave-uniform)
    const int vtr0 = attn_vtr0<VRB>(lane, g);
    half_t* otile = at.o + (long)seq * at.o_seq_stride + (long)(m0 - seq * at.Lq + wm * WTM + l31) * at.o_tok_stride + (h0 + wn * HPW) * D;
#pragma unroll
    for (int hh = 0; hh < HPW; ++hh) {
        if (hh == 1) {
            // every wave is done with phase 0: slot A takes head 3 (the LDS reads of phase 0 have returned - their MFMAs
            // were issued; the stores of phase 0 stay in flight until the second barrier)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            deliver(3, 0);
            attn_wg_barrier();
        }
        const int slot = hh == 0 ? wn : (wn == 0 ? 2 : 0);         // wave-uniform
        const uint8_t* k_l = smem + slot * SLOT + l31 * KROW;
        const uint8_t* v_l = smem + slot * SLOT + NT * KTB + vtr0;
#pragma unroll
        for (int b = 0; b < QB; ++b) {
            float16v oacc[DT];
            attn_zero(oacc);
            float m_run = -INFINITY;
#pragma nounroll
            for (int hf = 0; hf < nhalf; ++hf) {                   // attn_cross32_kernel's walk of one query tile
                float16v s;
                const float16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                {
                    half8 kf[KS];
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) kf[ks] = attn_frag<D, false>(k_l + hf * 32 * KROW, ks, g);
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qf[hh][b][ks], ks == 0 ? zero16 : s, 0, 0, 0);
                }
                AttnVF vf[2 * DT];                                 // V^T fragments: requested here, they fly under the softmax
#pragma unroll
                for (int idx2 = 0; idx2 < 2 * DT; ++idx2) attn_vt_frag<DT, VRB>(v_l + hf * 32 * VRB, idx2, vf[idx2]);
                if ((hf + 1) * 32 > kv_len) attn_mask(s, hf * 32, g, kv_len);   // wave-uniform: the ragged last half
                const float mc = attn_lazy_rescale(attn_rowmax_swap(s), m_run, oacc, at.c);
                half8 pf[2];
                attn_exp_pack(s, at.c, mc, pf);
#pragma unroll
                for (int idx2 = 0; idx2 < 2 * DT; ++idx2)
                    oacc[idx2 % DT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[idx2].v, pf[idx2 / DT], oacc[idx2 % DT], 0, 0, 0);
            }
            const float inv = attn_inv_row_sum<D>(oacc, l31);
            attn_store_rows<D, DT>(oacc, inv, otile + (long)(b * 32) * at.o_tok_stride + hh * D, g, true);
        }
    }
}

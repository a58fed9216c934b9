// rowquant_fast.hip - register-resident per-token quantizers (the per-step hot variants).
//
// Same arithmetic and C ABI semantics as the generic kernels in rowquant.hip (which remain the
// fallback for batch-shared scales B > 1 and rows longer than 4608; static grids: rowquant_static.hip), but:
//   - the token's row is loaded ONCE into registers (16 B / lane coalesced), nothing is re-read;
//   - min/max of the plain quantizer runs on packed fp16 (v_pk_min/max_f16: exact, fp16 inputs);
//   - round(x/delta) is computed as rint(x * (1/delta)) with an exact-division fallback for the
//     lanes whose product lies within 1e-4 of a rounding boundary (|err| of the product form is
//     < 2.5e-5 for |x/delta| < 400), so the integer codes stay bit-identical to rint(x/delta);
//   - codes are packed with v_cvt_pk_u8_f32 and row sums taken with v_sad_u8;
//   - LN + modulate keeps the modulated row in fp32 registers between the min/max and the
//     quantize pass and reads shift/scale as 16-byte vectors.
// HBM-bound: algorithmic bytes per row = 2*C read + Kp written.
// The per-row steps (lane maps, reductions, row load, LayerNorm statistics, modulate, the quantize / store / row-sum
// tail) are in rowquant_shared.h; a kernel here is what is its own: which rows a wave takes, where its vectors live,
// how min / max are collected and exchanged.
#include <stdlib.h>
#include "vq_common.h"
#include "rowquant_shared.h"

#define RQF_WAVES 4
#define RQF_THREADS (RQF_WAVES * 64)

// The two environment variables this file reads, each here and nowhere else, once per process.  They are TEST ARMS, not
// tuning knobs: tests/test_kernels_gpu.py and tests/test_quantizer_edges_gpu.py start a child process with VQ_RQ_SPLIT=0 /
// VQ_RQ_SM1=0 to obtain the kernel the default one must match bit for bit (one row per wave at C = 4608;
// smooth_rowquant_half_kernel for one smoothed output).
static bool rq_split_enabled() {
    static const bool on = !(getenv("VQ_RQ_SPLIT") && atoi(getenv("VQ_RQ_SPLIT")) == 0);
    return on;
}
static int vq_sm1_mode() {
    static const int mode = getenv("VQ_RQ_SM1") ? atoi(getenv("VQ_RQ_SM1")) : 1;
    return mode;
}

// smooth-quant division of one chunk, w = u / s in the reciprocal form, and the lane's running min / max of the quotients
template <int W>
__device__ __forceinline__ void rq_smooth_chunk(const float (&u)[W], const float (&s)[W], const float (&r)[W], float (&w)[W],
                                                float& vmin, float& vmax) {
#pragma unroll
    for (int e = 0; e < W; ++e) {
        w[e] = rq_div_rcp(u[e], s[e], r[e]);
        vmin = fminf(vmin, w[e]);
        vmax = fmaxf(vmax, w[e]);
    }
}
// min / max over the lanes' packed fp16 running values
template <class V>
__device__ __forceinline__ void rq_minmax_h(const V& mn, const V& mx, float& vmin, float& vmax) {
    vmin = (float)mn[0];
    vmax = (float)mx[0];
#pragma unroll
    for (int e = 1; e < (int)(sizeof(V) / sizeof(half_t)); ++e) {
        vmin = fminf(vmin, (float)mn[e]);
        vmax = fmaxf(vmax, (float)mx[e]);
    }
}

// ---------------------------------------------------------------------------
// plain per-token quantizer, B == 1
// ---------------------------------------------------------------------------
// PAIR: x [2, n_tok, C] with the quantization grid of a token shared by its two samples (base_quantizer.py:185; the
// t2i loop's uncond | cond batch): waves 2k and 2k + 1 of a workgroup take the two rows of one token and exchange their
// min / max through LDS; outputs are indexed by row (sample * n_tok + token) with the shared step replicated, as the
// generic kernel writes them.
template <int MAXCH, bool HAS_S, bool HAS_ADD, bool GELU = false, bool PAIR = false>
__global__ __launch_bounds__(RQF_THREADS) void rowquant_fast_kernel(
    const half_t* __restrict__ x, const half_t* __restrict__ add_rows, int add_div, const float* __restrict__ s,
    const float* __restrict__ s_rcp, int8_t* __restrict__ xq, float* __restrict__ sx, int32_t* __restrict__ zx,
    int32_t* __restrict__ R, float* __restrict__ zpf, int n_tok, int C, int Kp, int n_bits, int32_t* status) {
    static_assert(!PAIR || (!HAS_ADD && RQF_WAVES % 2 == 0), "pairs of waves; added rows are per token");
    using L = RqWave<MAXCH>;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = L::lane_col(lane);
    int tok = PAIR ? blockIdx.x * (RQF_WAVES / 2) + (wv >> 1) : blockIdx.x * RQF_WAVES + wv;
    const bool live = tok < n_tok;
    if (!live) {
        if constexpr (!PAIR) return;
        tok = n_tok - 1;                                // stays for the workgroup barrier below, writes nothing
    }
    if (PAIR && (wv & 1)) tok += n_tok;                 // row index of (sample 1, token)
    const RqWidth wd = rq_width(n_bits);

    half8 h[MAXCH];
    // act(fc1 output) applied here, under the HBM stream, instead of in the GEMM epilogue
    if constexpr (GELU) rq_load_row<L>(x + (size_t)tok * C, lc, C, h, [](half8& v) { rq_gelu_tanh<8>(v); });
    else rq_load_row<L>(x + (size_t)tok * C, lc, C, h);
    float vmin, vmax;
    float w[(HAS_S || HAS_ADD) ? MAXCH : 1][8];     // the quantizer's input when it is not the row itself
    if constexpr (!HAS_S && !HAS_ADD) {
        half8 mn, mx;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mn[e] = (half_t)65504.f;
            mx[e] = (half_t)-65504.f;
        }
#pragma unroll
        for (int i = 0; i < MAXCH; ++i)
            if (lc + i * 512 < C) {
                mn = __builtin_elementwise_min(mn, h[i]);
                mx = __builtin_elementwise_max(mx, h[i]);
            }
        rq_minmax_h(mn, mx, vmin, vmax);
    } else {
        const half_t* addp = HAS_ADD ? add_rows + (size_t)(tok / add_div) * C : nullptr;
        vmin = INFINITY;
        vmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int c0 = lc + i * 512;
            if (c0 < C) {
                float sv[8], rv[8];
                if constexpr (HAS_S) {
                    rq_load_f<8>(s + c0, sv);
                    if (s_rcp) rq_load_f<8>(s_rcp + c0, rv);   // kernel-uniform
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = (float)h[i][e];
                    if constexpr (HAS_ADD) v += (float)addp[c0 + e];
                    if constexpr (HAS_S) v = s_rcp ? rq_div_rcp(v, sv[e], rv[e]) : __fdiv_rn(v, sv[e]);
                    w[i][e] = v;
                    vmin = fminf(vmin, v);
                    vmax = fmaxf(vmax, v);
                }
            }
        }
    }
    vmin = rq_min_f<L::HALF>(vmin, false);
    vmax = rq_max_f<L::HALF>(vmax, false);
    if constexpr (PAIR) {
        __shared__ float pm[RQF_WAVES][2];
        if (lane == 0) {
            pm[wv][0] = vmin;
            pm[wv][1] = vmax;
        }
        __syncthreads();
        vmin = fminf(vmin, pm[wv ^ 1][0]);
        vmax = fmaxf(vmax, pm[wv ^ 1][1]);
    }
    float delta, zp, inv;
    bool small;
    vq_row_grid(vmin, vmax, wd.qmax, delta, zp, small, inv);
    if (small && lane == 0 && live && status) atomicOr(status, VQ_ST_EPSFILL);

    int8_t* qrow = xq + (size_t)tok * Kp;
    int cs;
    if constexpr (HAS_S || HAS_ADD) cs = rq_quant_row<L>(w, lc, C, Kp, delta, zp, inv, wd, qrow, live, false);
    else cs = rq_quant_row<L>(h, lc, C, Kp, delta, zp, inv, wd, qrow, live, false);
    if (lane == 0 && live) rq_write_row(sx, zx, R, zpf, tok, delta, zp, cs, C, wd.cx);
}

// ---------------------------------------------------------------------------
// LONG rows split over TWO partner waves (round 5; C = 4608: the fc2 input behind GELU, 59 us per launch = the largest
// HBM-bound kernel of a block).  rowquant_fast_kernel<9> gives a wave a whole 4608-channel row: 72 elements per lane, 1205
// VALU instructions (144 of them transcendental) between its loads and its stores, 16384 waves = 2.3 generations of resident
// waves that load, compute and store in step - 39 us of VALU issue and ~40 us of HBM time that overlap only partly
// (profiles/r04_hbm_kernels_pmc.md: WAIT_ANY 0.35-0.66, fabric bytes exactly algorithmic).  Here waves 2k / 2k + 1 of a
// workgroup take the two HALVES of a row - 36 elements per lane, the per-lane work of the C = 1152 half-wave kernels, the
// fastest quantizers of the step - and exchange min / max and the code sums through LDS: half the instruction stream per
// wave, half the registers (8 resident waves per SIMD), twice the wave generations, so loads, arithmetic and stores of
// different waves interleave instead of alternating chip-wide.  Same per-element expressions as rowquant_fast_kernel
// (rq_gelu_tanh, packed fp16 min / max, vq_row_grid, rq_quant): bit-identical outputs (tested).
// C / 2 = NF * 512 + (TAIL8 ? 256 : 0) channels per wave: NF 16-byte loads per lane + one 8-byte load.
// ---------------------------------------------------------------------------
// PAIR: x [2, n_tok, C] with the grid of a token shared by its two samples (the t2i uncond | cond forward): the four waves of a
// workgroup are (sample, half) of ONE token - min / max over all four, code sums per sample.
struct RqTail4 {             // one unmasked chunk of four channels for each of the 64 lanes (loaded and quantized, never reduced by this map)
    static constexpr bool HALF = true;
    static constexpr int NCH = 1, W = 4, STEP = 0;
    typedef half4 hvec;
    static __device__ __forceinline__ int lane_col(int lane) { return lane * 4; }
};
template <int NF, bool TAIL8, bool GELU, bool PAIR = false>
__global__ __launch_bounds__(RQF_THREADS) void rowquant_split_kernel(const half_t* __restrict__ x, int8_t* __restrict__ xq,
                                                                     float* __restrict__ sx, int32_t* __restrict__ zx,
                                                                     int32_t* __restrict__ R, int n_tok, int n_bits,
                                                                     int32_t* status) {
    static_assert(!PAIR || RQF_WAVES == 4, "(sample, half) = the four waves of a workgroup");
    using L = RqWave<NF>;        // the NF full chunks of the wave's half row (HC is a constant: no chunk is masked)
    using LT = RqTail4;          // its 8-byte tail
    constexpr int HC = NF * 512 + (TAIL8 ? 256 : 0), C = 2 * HC;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = wv & 1, lc = L::lane_col(lane);
    int tok = PAIR ? blockIdx.x : blockIdx.x * (RQF_WAVES / 2) + (wv >> 1);
    const bool live = tok < n_tok;
    if (!live) tok = n_tok - 1;                        // stays for the workgroup barriers, writes nothing
    if (PAIR && (wv >> 1)) tok += n_tok;               // row index of (sample 1, token)
    const RqWidth wd = rq_width(n_bits);
    const half_t* row = x + (size_t)tok * C + half * HC;

    half8 h[NF];
    half4 ht[1];
    rq_load_row<L>(row, lc, HC, h);
    if constexpr (TAIL8) rq_load_row<LT>(row + NF * 512, LT::lane_col(lane), 256, ht);
    half8 mn, mx;
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        if constexpr (GELU) rq_gelu_tanh<8>(h[i]);
        mn = i == 0 ? h[0] : __builtin_elementwise_min(mn, h[i]);
        mx = i == 0 ? h[0] : __builtin_elementwise_max(mx, h[i]);
    }
    if constexpr (TAIL8) {
        if constexpr (GELU) rq_gelu_tanh<4>(ht[0]);
        const half8 t8 = {ht[0][0], ht[0][1], ht[0][2], ht[0][3], ht[0][0], ht[0][1], ht[0][2], ht[0][3]};
        mn = NF == 0 ? t8 : __builtin_elementwise_min(mn, t8);
        mx = NF == 0 ? t8 : __builtin_elementwise_max(mx, t8);
    }
    float vmin, vmax;
    rq_minmax_h(mn, mx, vmin, vmax);
    vmin = rq_min_f<L::HALF>(vmin, false);
    vmax = rq_max_f<L::HALF>(vmax, false);
    __shared__ float pm[RQF_WAVES][2];
    __shared__ int ps[RQF_WAVES];
    if (lane == 0) {
        pm[wv][0] = vmin;
        pm[wv][1] = vmax;
    }
    __syncthreads();
    if constexpr (PAIR) {
#pragma unroll
        for (int w = 0; w < RQF_WAVES; ++w) {
            vmin = fminf(vmin, pm[w][0]);
            vmax = fmaxf(vmax, pm[w][1]);
        }
    } else {
        vmin = fminf(vmin, pm[wv ^ 1][0]);
        vmax = fmaxf(vmax, pm[wv ^ 1][1]);
    }
    float delta, zp, inv;
    bool small;
    vq_row_grid(vmin, vmax, wd.qmax, delta, zp, small, inv);
    if (small && lane == 0 && (PAIR ? wv == 0 : half == 0) && live && status) atomicOr(status, VQ_ST_EPSFILL);

    int8_t* qrow = xq + (size_t)tok * C + half * HC;
    uint32_t csum = rq_quant_lane<L>(h, lc, HC, HC, delta, zp, inv, wd, qrow, live);
    if constexpr (TAIL8) csum = rq_quant_lane<LT>(ht, LT::lane_col(lane), 256, 256, delta, zp, inv, wd, qrow + NF * 512, live, csum);
    const int rs_half = rq_sum_i<L::HALF>((int)csum, false);
    if (lane == 0) ps[wv] = rs_half;
    __syncthreads();
    if (lane == 0 && half == 0 && live) rq_write_row(sx, zx, R, nullptr, tok, delta, zp, rs_half + ps[wv ^ 1], C, wd.cx);
}

// ---------------------------------------------------------------------------
// smoothed per-token quantizer for LONG rows (C up to 4608: the fc2 input of the smooth-quant plans, optionally behind
// GELU): rowquant_fast_kernel<9, true> read the smoothing vector and its reciprocal from global memory for every row -
// 36.9 KB through the L1 per 9.2 KB row - and ran 69 us where the un-smoothed kernel takes 44.  Here a workgroup
// stages s and 1/s in LDS once and its waves walk rows grid-stride (next row's data requested before the current one
// is processed).  Same arithmetic in the same order as rowquant_fast_kernel's reciprocal path: bit-identical outputs.
// ---------------------------------------------------------------------------
// PAIR: x [2, n_tok, C], partner waves 2k / 2k + 1 take the two samples of a token and exchange min / max through LDS
// (one workgroup barrier per walk step, parity-double-buffered slots; every wave of a workgroup runs the same number
// of steps)
template <int MAXCH, bool GELU, bool PAIR = false>
__global__ __launch_bounds__(RQF_THREADS) void rowquant_smooth_lds_kernel(
    const half_t* __restrict__ x, const float* __restrict__ s, const float* __restrict__ s_rcp, int8_t* __restrict__ xq,
    float* __restrict__ sx, int32_t* __restrict__ zx, int32_t* __restrict__ R, int n_tok, int C, int Kp, int n_bits,
    int32_t* status) {
    using L = RqWave<MAXCH>;
    extern __shared__ __attribute__((aligned(16))) float rq_lds[];
    float* ls = rq_lds;
    float* lr = rq_lds + C;
    for (int c = threadIdx.x * 4; c < C; c += RQF_THREADS * 4) {
        *reinterpret_cast<float4v*>(ls + c) = *reinterpret_cast<const float4v*>(s + c);
        *reinterpret_cast<float4v*>(lr + c) = *reinterpret_cast<const float4v*>(s_rcp + c);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = L::lane_col(lane);
    const RqWidth wd = rq_width(n_bits);
    const int stride = PAIR ? gridDim.x * (RQF_WAVES / 2) : gridDim.x * RQF_WAVES;
    const int tok0 = PAIR ? blockIdx.x * (RQF_WAVES / 2) + (wv >> 1) : blockIdx.x * RQF_WAVES + wv;
    const size_t roff = (PAIR && (wv & 1)) ? (size_t)n_tok : 0;   // row = token + roff
    // walk steps: per wave, or (PAIR) per workgroup - the count of its first pair, the others idle through their tail
    const int base = PAIR ? blockIdx.x * (RQF_WAVES / 2) : tok0;
    const int n_it = base < n_tok ? (n_tok - base + stride - 1) / stride : 0;
    __shared__ float pm[2][RQF_WAVES][2];
    half8 hn[MAXCH];
    if (n_it > 0) rq_load_row<L>(x + ((size_t)(tok0 < n_tok ? tok0 : n_tok - 1) + roff) * C, lc, C, hn);
    for (int it = 0; it < n_it; ++it) {
        const int tk = tok0 + it * stride;
        const bool live = tk < n_tok;
        const size_t tok = (size_t)(live ? tk : n_tok - 1) + roff;
        float w[MAXCH][8];
#pragma unroll
        for (int i = 0; i < MAXCH; ++i)
            if (lc + i * 512 < C) {
                half8 g = hn[i];
                if constexpr (GELU) rq_gelu_tanh<8>(g);
                rq_widen(g, w[i]);
            }
        if (it + 1 < n_it) {                               // next row in flight under this row's arithmetic
            const int tn = tk + stride;
            rq_load_row<L>(x + ((size_t)(tn < n_tok ? tn : n_tok - 1) + roff) * C, lc, C, hn);
        }
        float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int c0 = lc + i * 512;
            if (c0 < C) {
                float sv[8], rv[8];
                rq_load_f<8>(ls + c0, sv);
                rq_load_f<8>(lr + c0, rv);
                rq_smooth_chunk<8>(w[i], sv, rv, w[i], vmin, vmax);
            }
        }
        vmin = rq_min_f<L::HALF>(vmin, false);
        vmax = rq_max_f<L::HALF>(vmax, false);
        if constexpr (PAIR) {
            if (lane == 0) {
                pm[it & 1][wv][0] = vmin;
                pm[it & 1][wv][1] = vmax;
            }
            __syncthreads();
            vmin = fminf(vmin, pm[it & 1][wv ^ 1][0]);
            vmax = fmaxf(vmax, pm[it & 1][wv ^ 1][1]);
        }
        float delta, zp, inv;
        bool small;
        vq_row_grid(vmin, vmax, wd.qmax, delta, zp, small, inv);
        if (small && lane == 0 && live && status) atomicOr(status, VQ_ST_EPSFILL);
        const int cs = rq_quant_row<L>(w, lc, C, Kp, delta, zp, inv, wd, xq + tok * Kp, live, false);
        if (lane == 0 && live) rq_write_row(sx, zx, R, nullptr, tok, delta, zp, cs, C, wd.cx);
    }
}

template <bool GELU, bool PAIR = false>
static bool launch_rq_smooth_lds(const half_t* x, const float* s, const float* s_rcp, int8_t* xq, float* sx, int32_t* zx,
                                 int32_t* R, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st) {
    if (C % 8 != 0 || C <= 1536 || C > 4608) return false;
    const int lds = 2 * C * (int)sizeof(float);
    constexpr auto k = rowquant_smooth_lds_kernel<9, GELU, PAIR>;
    if (vq_prepare_kernel<k>(2 * 4608 * (int)sizeof(float)) != VQ_OK) return false;
    constexpr int PER = PAIR ? RQF_WAVES / 2 : RQF_WAVES;  // tokens per workgroup and walk step
    int grid = (n_tok + PER - 1) / PER;
    if (grid > 1024) grid = 1024;                          // 4 workgroups of 36.9 KB LDS per CU; rows grid-stride
    hipLaunchKernelGGL(k, dim3(grid), dim3(RQF_THREADS), lds, st, x, s, s_rcp, xq, sx, zx, R, n_tok, C, Kp, n_bits, status);
    return true;
}

// ---------------------------------------------------------------------------
// plain per-token quantizer, TWO rows per wave (C % 128 == 0, C <= 1536, no smoothing / added rows).
// At C = 1152 the one-row-per-wave kernel above is VALU-bound, and half of its VALU work is per ROW, not per
// element (two DPP reductions, three IEEE divisions for delta / 1/delta / zp, the row-sum reduction), with a
// quarter of the lanes idle in the last 512-element pass.  Here a half-wave of 32 lanes owns a row (C/32
// elements per lane, 8-byte coalesced loads), so the per-row sequence runs once for two rows and every lane
// is busy.
// ---------------------------------------------------------------------------
// PAIR (round 3): the two rows of a wave are the SAME token of a batch of two (x [2, n_tok, C]: the t2i loop's
// uncond | cond forward), whose quantization grid the reference shares over the batch (base_quantizer.py:185): the
// min / max of the two half-waves are combined, everything else stays per row.  The generic B > 1 kernel this
// replaces for B == 2 took 24 us per launch at 2 x 4096 rows (13.5 % of a PixArt-Sigma step).
// The row of this half-wave when its wave takes pair p: two consecutive rows, or (PAIR) the two samples of token p.
// Odd tail: the upper half re-does the last row and writes nothing (``live``).
template <bool PAIR>
__device__ __forceinline__ int rqh_row(int p, bool hi, int n_tok, bool& live) {
    const int t = PAIR ? p : p * 2 + (hi ? 1 : 0);
    live = t < n_tok;
    return (live ? t : n_tok - 1) + ((PAIR && hi) ? n_tok : 0);
}
// min / max of a half-wave's row; PAIR: one grid for the token's two samples
template <bool PAIR>
__device__ __forceinline__ void rqh_minmax(float& vmin, float& vmax, bool hi) {
    vmin = rq_min_f<true>(vmin, hi);
    vmax = rq_max_f<true>(vmax, hi);
    if constexpr (PAIR) {
        vmin = fminf(vmin, __shfl_xor(vmin, 32));
        vmax = fmaxf(vmax, __shfl_xor(vmax, 32));
    }
}

template <int NIT, bool PAIR = false>   // C = 128 * NIT
__global__ __launch_bounds__(RQF_THREADS) void rowquant_half_kernel(const half_t* __restrict__ x, int8_t* __restrict__ xq,
                                                                    float* __restrict__ sx, int32_t* __restrict__ zx,
                                                                    int32_t* __restrict__ R, float* __restrict__ zpf,
                                                                    int n_tok, int n_bits, int32_t* status) {
    using L = RqHalf<NIT>;
    constexpr int C = 128 * NIT;
    const int lane = threadIdx.x & 63, hl = lane & 31, lc = L::lane_col(lane);
    const bool hi = lane >= 32;
    bool live;
    const int tok = rqh_row<PAIR>(blockIdx.x * RQF_WAVES + (threadIdx.x >> 6), hi, n_tok, live);
    const RqWidth wd = rq_width(n_bits);

    half4 h[NIT];
    rq_load_row<L>(x + (size_t)tok * C, lc, C, h);
    half4 mn = h[0], mx = h[0];
#pragma unroll
    for (int i = 1; i < NIT; ++i) {
        mn = __builtin_elementwise_min(mn, h[i]);
        mx = __builtin_elementwise_max(mx, h[i]);
    }
    float vmin = fminf(fminf((float)mn[0], (float)mn[1]), fminf((float)mn[2], (float)mn[3]));
    float vmax = fmaxf(fmaxf((float)mx[0], (float)mx[1]), fmaxf((float)mx[2], (float)mx[3]));
    rqh_minmax<PAIR>(vmin, vmax, hi);
    float delta, zp, inv;
    bool small;
    vq_row_grid(vmin, vmax, wd.qmax, delta, zp, small, inv);
    if (small && hl == 0 && live && status) atomicOr(status, VQ_ST_EPSFILL);
    const int cs = rq_quant_row<L>(h, lc, C, C, delta, zp, inv, wd, xq + (size_t)tok * C, live, hi);
    if (hl == 0 && live) rq_write_row(sx, zx, R, zpf, tok, delta, zp, cs, C, wd.cx);
}

// ---------------------------------------------------------------------------
// LayerNorm(no affine) + AdaLN modulate + NOUT smoothed quantizers, B == 1 per token row
// (rows of different batch samples are independent here because every row gets its own scale
//  only when B == 1; the host dispatches B > 1 to the generic kernel)
// ---------------------------------------------------------------------------
template <int MAXCH, int NOUT>
__global__ __launch_bounds__(RQF_THREADS) void ln_modulate_rowquant_fast_kernel(
    const half_t* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ scale, float ln_eps,
    LnqOut o, half_t* __restrict__ xm_out, int n_tok, int C, int Kp, int n_bits, int32_t* status) {
    using L = RqWave<MAXCH>;
    const int lane = threadIdx.x & 63, lc = L::lane_col(lane);
    const int tok = blockIdx.x * RQF_WAVES + (threadIdx.x >> 6);
    if (tok >= n_tok) return;
    const RqWidth wd = rq_width(n_bits);

    half8 h[MAXCH];
    float v[MAXCH][8];
    rq_load_row<L>(x + (size_t)tok * C, lc, C, h);
    rq_widen_row<L>(h, lc, C, v);
    float mu, rstd;
    rq_ln_stats<L>(v, lc, C, ln_eps, false, mu, rstd);

    float vmin[NOUT], vmax[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        vmin[j] = INFINITY;
        vmax[j] = -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c0 = lc + i * 512;
        if (c0 < C) {
            float sc1[8], sh[8];
            rq_load_mod<8>(scale + c0, shift + c0, sc1, sh);
            rq_modulate<8>(v[i], mu, rstd, sc1, sh, xm_out != nullptr, xm_out, (size_t)tok * C + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int j = 0; j < NOUT; ++j) {
                    const float w = o.s[j] ? __fdiv_rn(v[i][e], o.s[j][c0 + e]) : v[i][e];
                    vmin[j] = fminf(vmin[j], w);
                    vmax[j] = fmaxf(vmax[j], w);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        float delta, zp, inv;
        bool small;
        vq_row_grid(rq_min_f<L::HALF>(vmin[j], false), rq_max_f<L::HALF>(vmax[j], false), wd.qmax, delta, zp, small, inv);
        if (small && lane == 0 && status) atomicOr(status, VQ_ST_EPSFILL);
        const float* sj = o.s[j];                          // (IEEE division again: the quotients are not kept, NOUT x 72 registers)
        const int cs = rq_quant_row<L>(v, lc, C, Kp, delta, zp, inv, wd, o.xq[j] + (size_t)tok * Kp, true, false,
                                       [&](int, int c0, float (&w)[8]) {
                                           if (sj) {
#pragma unroll
                                               for (int e = 0; e < 8; ++e) w[e] = __fdiv_rn(w[e], sj[c0 + e]);
                                           }
                                       });
        if (lane == 0) rq_write_row(o.sx[j], o.zx[j], o.R[j], nullptr, tok, delta, zp, cs, C, wd.cx);
    }
}

// LN + modulate + ONE un-smoothed quantizer, two rows per wave (same reasoning as rowquant_half_kernel; this
// kernel has five per-row reductions and four IEEE divisions / a square root per row).
// XM: also store the modulated activation as fp16 (the t2i final layer's LayerNorm + modulate in front of a Linear that
// quantizes its own input: for B = 2 that call used to fall to the generic kernel, 74 us per PixArt-Sigma step)
template <int NIT, bool PAIR = false, bool XM = false>   // PAIR: see rowquant_half_kernel; shift / scale [2, C], one row per sample
__global__ __launch_bounds__(RQF_THREADS) void ln_modulate_rowquant_half_kernel(
    const half_t* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ scale, float ln_eps,
    int8_t* __restrict__ xq, float* __restrict__ sx, int32_t* __restrict__ zx, int32_t* __restrict__ R, int n_tok,
    int n_bits, int32_t* status, half_t* __restrict__ xm = nullptr) {
    using L = RqHalf<NIT>;
    constexpr int C = 128 * NIT;
    const int lane = threadIdx.x & 63, hl = lane & 31, lc = L::lane_col(lane);
    const bool hi = lane >= 32;
    bool live;
    const int tok = rqh_row<PAIR>(blockIdx.x * RQF_WAVES + (threadIdx.x >> 6), hi, n_tok, live);
    if (PAIR && hi) {
        shift += C;
        scale += C;
    }
    const RqWidth wd = rq_width(n_bits);

    half4 h[NIT];
    float v[NIT][4];
    rq_load_row<L>(x + (size_t)tok * C, lc, C, h);
    rq_widen_row<L>(h, lc, C, v);
    float mu, rstd;
    rq_ln_stats<L>(v, lc, C, ln_eps, hi, mu, rstd);

    float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const float4v sc = *reinterpret_cast<const float4v*>(scale + i * 128 + hl * 4);
        const float4v sh = *reinterpret_cast<const float4v*>(shift + i * 128 + hl * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float y = (v[i][e] - mu) * rstd;
            const float u = y * (1.0f + sc[e]) + sh[e];
            v[i][e] = u;
            vmin = fminf(vmin, u);
            vmax = fmaxf(vmax, u);
        }
        if constexpr (XM) {
            if (live) {
                const half4 hm = {(half_t)v[i][0], (half_t)v[i][1], (half_t)v[i][2], (half_t)v[i][3]};
                *reinterpret_cast<half4*>(xm + (size_t)tok * C + hl * 4 + i * 128) = hm;
            }
        }
    }
    rqh_minmax<PAIR>(vmin, vmax, hi);
    float delta, zp, inv;
    bool small;
    vq_row_grid(vmin, vmax, wd.qmax, delta, zp, small, inv);
    if (small && hl == 0 && live && status) atomicOr(status, VQ_ST_EPSFILL);
    int8_t* qrow = xq + (size_t)tok * C + hl * 4;
    uint32_t csum = 0;
    RQ_BY_WIDTH(wd.qmax, _Pragma("unroll") for (int i = 0; i < NIT; ++i) {
        uint32_t pk[1];
        rq_quant<4, SAT8_>(v[i], inv, delta, zp, wd.qmax, pk);
        csum = __builtin_amdgcn_sad_u8(pk[0], 0u, csum);
        if (live) *reinterpret_cast<uint32_t*>(qrow + i * 128) = pk[0] ^ wd.flip;
    })
    int cs = (int)csum;
    RQH_REDUCE2(int, vq_addi, cs)
    if (hl == 0 && live) rq_write_row(sx, zx, R, nullptr, tok, delta, zp, cs, C, wd.cx);
}

// ---------------------------------------------------------------------------
// smoothed per-token quantizers at C = 128 * NIT <= 1536, optionally behind LayerNorm + AdaLN modulate, for the plans
// that balance every Linear against its own weight (W4A8: q / k / v carry three smoothing vectors).
// What the one-row-per-wave kernels above paid for smoothing was two IEEE divisions per element and output (min/max
// pass and quantize pass, ~12 VALU instructions each) on top of ~7 for the quantizer itself.  Here
//   - a half-wave owns a row as in rowquant_half_kernel, and a wave walks RPW row pairs with the smoothing vector, its
//     reciprocal and (LN) the modulation vectors of ITS output resident in registers;
//   - x / s is rq_div_rcp (3 instructions, bit-identical to the IEEE quotient) and computed once per element;
//   - blockIdx.y is the output: the q / k / v copies of one row are produced by three workgroups that each re-read the
//     row (L2 / MALL hits: the activation is 38 MB) and redo the cheap LN, instead of one wave carrying 3 x 72 extra
//     registers.  Output 0 also writes the modulated activation when asked for.
// ---------------------------------------------------------------------------
template <int NIT, bool LN, int RPW, bool PAIR = false>   // PAIR: the wave's two rows are ONE token of a batch of two (see rowquant_half_kernel)
__global__ __launch_bounds__(RQF_THREADS) void smooth_rowquant_half_kernel(
    const half_t* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ scale, float ln_eps,
    LnqOut o, half_t* __restrict__ xm_out, int n_tok, int n_bits, int32_t* status) {
    using L = RqHalf<NIT>;
    constexpr int C = 128 * NIT;
    const int lane = threadIdx.x & 63, hl = lane & 31, lc = L::lane_col(lane);
    const bool hi = lane >= 32;
    const int j = blockIdx.y;
    const RqWidth wd = rq_width(n_bits);
    const float* __restrict__ sp = o.s[j];
    const float* __restrict__ rp = o.r[j];
    float s4[NIT][4], r4[NIT][4], sc1[LN ? NIT : 1][4], sh[LN ? NIT : 1][4];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        rq_load_f<4>(sp + lc + i * 128, s4[i]);
        rq_load_f<4>(rp + lc + i * 128, r4[i]);
        if constexpr (LN) {
            const int bo = (PAIR && hi) ? C : 0;           // modulation vectors of the upper half's sample
            rq_load_mod<4>(scale + bo + lc + i * 128, shift + bo + lc + i * 128, sc1[i], sh[i]);
        }
    }
    const int pair0 = (blockIdx.x * RQF_WAVES + (threadIdx.x >> 6)) * RPW;
    bool live;
    half4 hn[NIT];
    rq_load_row<L>(x + (size_t)rqh_row<PAIR>(pair0, hi, n_tok, live) * C, lc, C, hn);
    for (int it = 0; it < RPW; ++it) {
        if ((PAIR ? pair0 + it : (pair0 + it) * 2) >= n_tok) break;   // wave-uniform
        const int tok = rqh_row<PAIR>(pair0 + it, hi, n_tok, live);
        float w[NIT][4];
        rq_widen_row<L>(hn, lc, C, w);
        if (it + 1 < RPW) {                                // next pair's rows fly under this pair's arithmetic
            bool unused;
            rq_load_row<L>(x + (size_t)rqh_row<PAIR>(pair0 + it + 1, hi, n_tok, unused) * C, lc, C, hn);
        }
        if constexpr (LN) {
            float mu, rstd;
            rq_ln_stats<L>(w, lc, C, ln_eps, hi, mu, rstd);
#pragma unroll
            for (int i = 0; i < NIT; ++i)
                rq_modulate<4>(w[i], mu, rstd, sc1[i], sh[i], xm_out && j == 0 && live, xm_out, (size_t)tok * C + lc + i * 128);
        }
        float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < NIT; ++i) rq_smooth_chunk<4>(w[i], s4[i], r4[i], w[i], vmin, vmax);
        rqh_minmax<PAIR>(vmin, vmax, hi);
        float delta, zp, inv;
        bool small;
        vq_row_grid(vmin, vmax, wd.qmax, delta, zp, small, inv);
        if (small && hl == 0 && live && status) atomicOr(status, VQ_ST_EPSFILL);
        const int cs = rq_quant_row<L>(w, lc, C, C, delta, zp, inv, wd, o.xq[j] + (size_t)tok * C, live, hi);
        if (hl == 0 && live) rq_write_row(o.sx[j], o.zx[j], o.R[j], nullptr, tok, delta, zp, cs, C, wd.cx);
    }
}

template <bool LN, int RPW, bool PAIR = false>
static bool launch_smooth_half(const half_t* x, const float* shift, const float* scale, float eps, const LnqOut& o,
                               int n_out, half_t* xm, int n_tok, int C, int n_bits, int32_t* status, hipStream_t st) {
    constexpr int PER = (PAIR ? 1 : 2) * RQF_WAVES * RPW;   // rows (PAIR: tokens) per workgroup
    dim3 grid((n_tok + PER - 1) / PER, n_out);
    return vq_dispatch_nit(C, [&](auto nit) {
        hipLaunchKernelGGL((smooth_rowquant_half_kernel<nit(), LN, RPW, PAIR>), grid, dim3(RQF_THREADS), 0, st, x, shift, scale,
                           eps, o, xm, n_tok, n_bits, status);
    });
}

// ---------------------------------------------------------------------------
// Two or three smoothed outputs of ONE pass over the rows (round 3).  smooth_rowquant_half_kernel above gives every
// output its own workgroups: the q / k / v copies re-read the row from L2 / MALL and redo the LayerNorm, and a launch
// moved 3 x 38 MB + 57 MB (LN + modulate + 3 outputs: 38 us = 2.5 TB/s of useful bytes).  Here a half-wave still owns a
// row and still computes the same per-lane expressions in the same order (codes, steps, zero points and row sums are
// bit-identical to that kernel's - tested), but the smoothing vectors, their reciprocals and (LN) the modulation
// vectors of all outputs live in LDS (8 x 4.6 KB at C = 1152, staged once per workgroup of NWV waves; one
// conflict-free ds_read_b128 per four channels, both half-waves reading the same words), so one set of row registers
// serves every output: the row is read once, normalised once, and quantized NOUT times.
// ---------------------------------------------------------------------------
// One smoothed output through the same kernel (round 5; VQ_RQ_SM1=0 keeps smooth_rowquant_half_kernel): with the vectors in
// LDS a wave needs ~80 registers instead of 167 (LN: 248), i.e. every wave of a launch is resident at once.
// waves per SIMD asked of the compiler, row pairs per wave, waves per workgroup: one output / two or three
constexpr int VQ_SM1_MINW = 6, VQ_SM1_RPW = 1, VQ_SM1_NWV = 8;
constexpr int VQ_SMM_MINW = 4, VQ_SMM_RPW = 1, VQ_SMM_NWV = 8;
// PAIR (vq_rowquant_smooth_multi_shared): x [2, n_tok, C], the wave's two rows are the two samples of ONE token (see
// rowquant_half_kernel), whose grid the reference shares over the batch (base_quantizer.py:185): per output the min / max
// of the two half-waves are combined, everything else - the LayerNorm statistics, the codes, the row sums - stays per
// row, and both samples' modulation vectors ([2, C]) are staged, the upper half reading sample 1's.  A workgroup owns
// NWV * RPW tokens.  Same per-lane expressions in the same order as smooth_rowquant_half_kernel<.., PAIR>: output j is
// that kernel's launch with vector j, bit for bit (tested).  No xm_out in this form.
template <int NIT, bool LN, int NOUT, int RPW, int NWV, bool PAIR = false>
__global__ __launch_bounds__(64 * NWV, NOUT == 1 ? VQ_SM1_MINW : VQ_SMM_MINW) void smooth_rowquant_multi_kernel(
    const half_t* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ scale, float ln_eps,
    LnqOut o, half_t* __restrict__ xm_out, int n_tok, int n_bits, int32_t* status) {
    using L = RqHalf<NIT>;
    constexpr int C = 128 * NIT;
    constexpr int NMOD = PAIR ? 2 : 1;                     // samples whose [1 + scale | shift] are staged
    extern __shared__ __attribute__((aligned(16))) float smq_lds[];   // [NOUT][s | r][C], then (LN) [NMOD][1 + scale | shift][C]
    const int lane = threadIdx.x & 63, hl = lane & 31, lc = L::lane_col(lane);
    const bool hi = lane >= 32;
    const RqWidth wd = rq_width(n_bits);
    const int pair0 = (blockIdx.x * NWV + (threadIdx.x >> 6)) * RPW;
    bool live;
    half4 hn[NIT];                                         // the first rows are requested before the staging loads
    rq_load_row<L>(x + (size_t)rqh_row<PAIR>(pair0, hi, n_tok, live) * C, lc, C, hn);
    for (int i = threadIdx.x; i < C / 4; i += 64 * NWV) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            reinterpret_cast<float4v*>(smq_lds + (2 * j) * C)[i] = reinterpret_cast<const float4v*>(o.s[j])[i];
            reinterpret_cast<float4v*>(smq_lds + (2 * j + 1) * C)[i] = reinterpret_cast<const float4v*>(o.r[j])[i];
        }
        if constexpr (LN) {
#pragma unroll
            for (int b = 0; b < NMOD; ++b) {
                float sc1[4], sh[4];
                rq_load_mod<4>(scale + b * C + 4 * i, shift + b * C + 4 * i, sc1, sh);
                reinterpret_cast<float4v*>(smq_lds + (2 * NOUT + 2 * b) * C)[i] = *reinterpret_cast<const float4v*>(sc1);
                reinterpret_cast<float4v*>(smq_lds + (2 * NOUT + 2 * b + 1) * C)[i] = *reinterpret_cast<const float4v*>(sh);
            }
        }
    }
    __syncthreads();
    const float* lmod = smq_lds + (2 * NOUT + ((PAIR && hi) ? 2 : 0)) * C;   // modulation vectors of this half's sample
    for (int it = 0; it < RPW; ++it) {
        if ((PAIR ? pair0 + it : (pair0 + it) * 2) >= n_tok) break;   // wave-uniform
        const int tok = rqh_row<PAIR>(pair0 + it, hi, n_tok, live);
        float w[NIT][4];
        rq_widen_row<L>(hn, lc, C, w);
        if (it + 1 < RPW) {                                // next pair's rows fly under this pair's arithmetic
            bool unused;
            rq_load_row<L>(x + (size_t)rqh_row<PAIR>(pair0 + it + 1, hi, n_tok, unused) * C, lc, C, hn);
        }
        if constexpr (LN) {
            float mu, rstd;
            rq_ln_stats<L>(w, lc, C, ln_eps, hi, mu, rstd);
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                float sc1[4], sh[4];
                rq_load_f<4>(lmod + lc + i * 128, sc1);
                rq_load_f<4>(lmod + C + lc + i * 128, sh);
                rq_modulate<4>(w[i], mu, rstd, sc1, sh, !PAIR && xm_out && live, xm_out, (size_t)tok * C + lc + i * 128);
            }
        }
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            float q[NIT][4];
            float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                float s4[4], r4[4];
                rq_load_f<4>(smq_lds + (2 * j) * C + lc + i * 128, s4);
                rq_load_f<4>(smq_lds + (2 * j + 1) * C + lc + i * 128, r4);
                rq_smooth_chunk<4>(w[i], s4, r4, q[i], vmin, vmax);
            }
            rqh_minmax<PAIR>(vmin, vmax, hi);
            float delta, zp, inv;
            bool small;
            vq_row_grid(vmin, vmax, wd.qmax, delta, zp, small, inv);
            if (small && (PAIR ? lane == 0 : hl == 0) && live && status) atomicOr(status, VQ_ST_EPSFILL);   // once per grid
            const int cs = rq_quant_row<L>(q, lc, C, C, delta, zp, inv, wd, o.xq[j] + (size_t)tok * C, live, hi);
            if (hl == 0 && live) rq_write_row(o.sx[j], o.zx[j], o.R[j], nullptr, tok, delta, zp, cs, C, wd.cx);
        }
    }
}

template <bool LN, int NOUT, bool PAIR = false>
static bool launch_smooth_multi(const half_t* x, const float* shift, const float* scale, float eps, const LnqOut& o,
                                half_t* xm, int n_tok, int C, int n_bits, int32_t* status, hipStream_t st) {
    constexpr int RPW = NOUT == 1 ? VQ_SM1_RPW : VQ_SMM_RPW, NWV = NOUT == 1 ? VQ_SM1_NWV : VQ_SMM_NWV;
    constexpr int PER = (PAIR ? 1 : 2) * NWV * RPW;        // rows (PAIR: tokens) per workgroup
    const size_t lds = (size_t)(2 * NOUT + (LN ? (PAIR ? 4 : 2) : 0)) * C * sizeof(float);
    dim3 grid((n_tok + PER - 1) / PER);
    return vq_dispatch_nit(C, [&](auto nit) {              // <= 10 x 5 KB of LDS: inside the 64 KB every kernel may use
        hipLaunchKernelGGL((smooth_rowquant_multi_kernel<nit(), LN, NOUT, RPW, NWV, PAIR>), grid, dim3(64 * NWV), lds, st, x,
                           shift, scale, eps, o, xm, n_tok, n_bits, status);
    });
}

// ---------------------------------------------------------------------------
// host dispatch (called from the C ABI entry points in rowquant.hip)
// ---------------------------------------------------------------------------
// rowquant_fast_kernel<MAXCH, HAS_S, HAS_ADD, GELU, PAIR>, one row per wave (PAIR: per partner wave), for these operands.
// Only the forms an entry point can ask for are compiled: added rows exist for the plain quantizer alone, and the plain
// pair quantizer takes no smoothing vector.
template <bool GELU, bool PAIR>
static void launch_rq(const half_t* x, const half_t* add_rows, int add_div, const float* s, const float* s_rcp, int8_t* xq,
                      float* sx, int32_t* zx, int32_t* R, float* zpf, int n_tok, int C, int Kp, int n_bits, int32_t* status,
                      hipStream_t st) {
    constexpr int PER = PAIR ? RQF_WAVES / 2 : RQF_WAVES;   // tokens per workgroup
    dim3 grid((n_tok + PER - 1) / PER);
    vq_dispatch_maxch(Kp, [&](auto m) {
        vq_dispatch_bool(s != nullptr, [&](auto hs) {
            vq_dispatch_bool(add_rows != nullptr, [&](auto ha) {
                if constexpr ((!ha() || (!GELU && !PAIR)) && (!hs() || GELU || !PAIR))
                    hipLaunchKernelGGL((rowquant_fast_kernel<m(), hs(), ha(), GELU, PAIR>), grid, dim3(RQF_THREADS), 0, st, x, add_rows,
                                       add_div, s, s_rcp, xq, sx, zx, R, zpf, n_tok, C, Kp, n_bits, status);
            });
        });
    });
}

bool vq_rowquant_fast(const half_t* x, const half_t* add_rows, int add_div, const float* s, const float* s_rcp,
                      int8_t* xq, float* sx, int32_t* zx, int32_t* R, float* zpf, int n_tok, int C, int Kp, int n_bits,
                      int32_t* status, hipStream_t st) {
    if (C > 4608 || Kp > 4608) return false;
    const bool hs = s != nullptr, ha = add_rows != nullptr;
    if (hs && s_rcp && !ha && !zpf && C > 1536 && n_tok >= 64 &&
        launch_rq_smooth_lds<false>(x, s, s_rcp, xq, sx, zx, R, n_tok, C, Kp, n_bits, status, st))
        return true;
    const bool half_wave = rq_block_width(C) && Kp == C && n_tok >= 2;
    if (hs && s_rcp && !ha && !zpf && half_wave) {
        const LnqOut o = lnq_one(s, s_rcp, xq, sx, zx, R);
        if (vq_sm1_mode() && launch_smooth_multi<false, 1>(x, nullptr, nullptr, 0.f, o, nullptr, n_tok, C, n_bits, status, st)) return true;
        if (launch_smooth_half<false, 2>(x, nullptr, nullptr, 0.f, o, 1, nullptr, n_tok, C, n_bits, status, st)) return true;
    }
    if (!hs && !ha && half_wave) {
        dim3 g2((n_tok + 2 * RQF_WAVES - 1) / (2 * RQF_WAVES));
        return vq_dispatch_nit(C, [&](auto nit) {
            hipLaunchKernelGGL((rowquant_half_kernel<nit()>), g2, dim3(RQF_THREADS), 0, st, x, xq, sx, zx, R, zpf, n_tok, n_bits, status);
        });
    }
    launch_rq<false, false>(x, add_rows, add_div, s, s_rcp, xq, sx, zx, R, zpf, n_tok, C, Kp, n_bits, status, st);
    return true;
}

// x [2, n_tok, C], grids shared by the two samples of a token (B == 2 of the C ABI): the half-wave kernel at the block
// widths, one row per wave with an LDS exchange between partner waves elsewhere
bool vq_rowquant_pair_fast(const half_t* x, int8_t* xq, float* sx, int32_t* zx, int32_t* R, float* zpf, int n_tok, int C,
                           int Kp, int n_bits, int32_t* status, hipStream_t st) {
    if (C > 4608 || Kp > 4608) return false;
    if (rq_block_width(C) && Kp == C) {
        dim3 g2((n_tok + RQF_WAVES - 1) / RQF_WAVES);
        return vq_dispatch_nit(C, [&](auto nit) {
            hipLaunchKernelGGL((rowquant_half_kernel<nit(), true>), g2, dim3(RQF_THREADS), 0, st, x, xq, sx, zx, R, zpf, n_tok, n_bits, status);
        });
    }
    launch_rq<false, true>(x, nullptr, 1, nullptr, nullptr, xq, sx, zx, R, zpf, n_tok, C, Kp, n_bits, status, st);
    return true;
}

// the same with the smooth-quant division x / s (reciprocal form) in front of the quantizer
bool vq_rowquant_pair_smooth_fast(const half_t* x, const float* s, const float* s_rcp, int8_t* xq, float* sx, int32_t* zx,
                                  int32_t* R, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st) {
    if (C > 1536)
        return n_tok >= 2 && launch_rq_smooth_lds<false, true>(x, s, s_rcp, xq, sx, zx, R, n_tok, C, Kp, n_bits, status, st);
    if (!rq_block_width(C) || Kp != C) return false;
    return launch_smooth_half<false, 2, true>(x, nullptr, nullptr, 0.f, lnq_one(s, s_rcp, xq, sx, zx, R), 1, nullptr, n_tok, C, n_bits,
                                              status, st);
}

bool vq_lnq_pair_fast(const half_t* x, const float* shift, const float* scale, float eps, const float* s, const float* s_rcp,
                      int8_t* xq, float* sx,
                      int32_t* zx, int32_t* R, half_t* xm, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st) {
    if (Kp != C || !rq_block_width(C)) return false;
    if (s) {
        if (!s_rcp || xm) return false;
        return launch_smooth_half<true, 2, true>(x, shift, scale, eps, lnq_one(s, s_rcp, xq, sx, zx, R), 1, nullptr, n_tok, C, n_bits,
                                                 status, st);
    }
    dim3 g2((n_tok + RQF_WAVES - 1) / RQF_WAVES);
    return vq_dispatch_nit(C, [&](auto nit) {
        vq_dispatch_bool(xm != nullptr, [&](auto has_xm) {
            hipLaunchKernelGGL((ln_modulate_rowquant_half_kernel<nit(), true, has_xm()>), g2, dim3(RQF_THREADS), 0, st, x, shift,
                               scale, eps, xq, sx, zx, R, n_tok, n_bits, status, xm);
        });
    });
}

template <int MAXCH>
static void launch_lnq(int n_out, dim3 grid, hipStream_t st, const half_t* x, const float* shift, const float* scale,
                       float eps, const LnqOut& o, half_t* xm, int n_tok, int C, int Kp, int n_bits,
                       int32_t* status) {
    auto go = [&](auto nout) {
        hipLaunchKernelGGL((ln_modulate_rowquant_fast_kernel<MAXCH, nout()>), grid, dim3(RQF_THREADS), 0, st, x, shift, scale, eps, o,
                           xm, n_tok, C, Kp, n_bits, status);
    };
    if (n_out == 1) go(std::integral_constant<int, 1>{});
    else if (n_out == 2) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 3>{});
}

// GELU(tanh) + (x / s) + per-token quantizer: mlp.act + the activation quantizer of mlp.fc2 in one pass
bool vq_gelu_rowquant_fast(const half_t* x, const float* s, const float* s_rcp, int8_t* xq, float* sx, int32_t* zx,
                           int32_t* R, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st) {
    if (C > 4608 || Kp > 4608) return false;
    if (s && s_rcp && C > 1536 && n_tok >= 64 &&
        launch_rq_smooth_lds<true>(x, s, s_rcp, xq, sx, zx, R, n_tok, C, Kp, n_bits, status, st))
        return true;
    // C = 4608 (the fc2 input of the XL models), no smoothing: the row split over two partner waves (bit-identical to the
    // one-row-per-wave kernel below, rq_split_enabled).  (The SMOOTHED long-row kernel above - persistent workgroups,
    // vectors in LDS, next row in flight - was also built in the split form, bit-identical, and the W4A8 step lost 0.8 % with
    // it in an A/B on one box (23.75 vs 23.56 steps/s, profiles/r05_experiments.md): it already overlaps its loads with its
    // arithmetic, the split only added a barrier per row.  Not kept.)
    if (!s && rq_split_enabled() && C == 4608 && Kp == C && n_tok >= 2) {
        hipLaunchKernelGGL((rowquant_split_kernel<4, true, true>), dim3((n_tok + RQF_WAVES / 2 - 1) / (RQF_WAVES / 2)),
                           dim3(RQF_THREADS), 0, st, x, xq, sx, zx, R, n_tok, n_bits, status);
        return true;
    }
    launch_rq<true, false>(x, nullptr, 1, s, s_rcp, xq, sx, zx, R, nullptr, n_tok, C, Kp, n_bits, status, st);
    return true;
}

// The same for a batch of TWO whose token grids the reference shares over the batch (the t2i loop's uncond | cond forward:
// x [2, n_tok, C], base_quantizer.py:185): partner waves take the two samples of a token and combine their min / max
// (after the GELU), as vq_rowquant's pair kernels do.
bool vq_gelu_rowquant_pair_fast(const half_t* x, const float* s, const float* s_rcp, int8_t* xq, float* sx, int32_t* zx,
                                int32_t* R, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st) {
    if (C > 4608 || Kp > 4608 || n_tok < 1) return false;
    if (s && s_rcp && C > 1536 && n_tok >= 2 &&
        launch_rq_smooth_lds<true, true>(x, s, s_rcp, xq, sx, zx, R, n_tok, C, Kp, n_bits, status, st))
        return true;
    // C = 4608 without smoothing: the (sample, half) split - four waves per token
    if (!s && rq_split_enabled() && C == 4608 && Kp == C) {
        hipLaunchKernelGGL((rowquant_split_kernel<4, true, true, true>), dim3(n_tok), dim3(RQF_THREADS), 0, st, x, xq, sx, zx, R, n_tok,
                           n_bits, status);
        return true;
    }
    // every other smoothed case - a vector without a usable reciprocal (vq_smooth_reciprocal flagged a channel, or an
    // unseen vector under graph capture: s_rcp == nullptr -> IEEE division, as B = 1 falls back), short rows - takes the
    // register kernel with the smoothing operands from global memory, like the un-smoothed pair
    launch_rq<true, true>(x, nullptr, 1, s, s_rcp, xq, sx, zx, R, nullptr, n_tok, C, Kp, n_bits, status, st);
    return true;
}

bool vq_lnq_fast(const half_t* x, const float* shift, const float* scale, float eps, int n_out,
                 const float* const* s, const float* const* s_rcp, int8_t* const* xq, float* const* sx,
                 int32_t* const* zx, int32_t* const* R, half_t* xm, int n_tok, int C, int Kp, int n_bits, int32_t* status,
                 hipStream_t st) {
    if (Kp > 1536) return false;
    const bool half_wave = rq_block_width(C) && Kp == C && n_tok >= 2;
    {
        bool all = s && s_rcp && half_wave;
        for (int j = 0; all && j < n_out; ++j) all = s[j] && s_rcp[j];
        if (all) {
            const LnqOut o = lnq_many(n_out, s, s_rcp, xq, sx, zx, R);
            if (n_out == 3 && launch_smooth_multi<true, 3>(x, shift, scale, eps, o, xm, n_tok, C, n_bits, status, st)) return true;
            if (n_out == 2 && launch_smooth_multi<true, 2>(x, shift, scale, eps, o, xm, n_tok, C, n_bits, status, st)) return true;
            if (n_out == 1 && vq_sm1_mode() && launch_smooth_multi<true, 1>(x, shift, scale, eps, o, xm, n_tok, C, n_bits, status, st)) return true;
            if (launch_smooth_half<true, 4>(x, shift, scale, eps, o, n_out, xm, n_tok, C, n_bits, status, st)) return true;
        }
    }
    if (n_out == 1 && !(s && s[0]) && !xm && half_wave) {
        dim3 g2((n_tok + 2 * RQF_WAVES - 1) / (2 * RQF_WAVES));
        return vq_dispatch_nit(C, [&](auto nit) {
            hipLaunchKernelGGL((ln_modulate_rowquant_half_kernel<nit()>), g2, dim3(RQF_THREADS), 0, st, x, shift, scale, eps,
                               xq[0], sx[0], zx[0], R[0], n_tok, n_bits, status);
        });
    }
    const LnqOut o = lnq_many(n_out, s, nullptr, xq, sx, zx, R);       // (IEEE division: no reciprocals)
    dim3 grid((n_tok + RQF_WAVES - 1) / RQF_WAVES);
    vq_dispatch_maxch(Kp, [&](auto m) {
        if constexpr (m() <= 3)                               // (Kp <= 1536 here: no MAXCH = 9 form of this kernel exists)
            launch_lnq<m()>(n_out, grid, st, x, shift, scale, eps, o, xm, n_tok, C, Kp, n_bits, status);
    });
    return true;
}

// n_out smoothed quantizers of one input in one launch (blockIdx.y = output); see smooth_rowquant_half_kernel
bool vq_rowquant_smooth_multi_fast(const half_t* x, int n_out, const float* const* s, const float* const* s_rcp,
                                   int8_t* const* xq, float* const* sx, int32_t* const* zx, int32_t* const* R, int n_tok,
                                   int C, int Kp, int n_bits, int32_t* status, hipStream_t st) {
    if (Kp != C || !rq_block_width(C) || n_tok < 2) return false;
    const LnqOut o = lnq_many(n_out, s, s_rcp, xq, sx, zx, R);
    if (n_out == 3 && launch_smooth_multi<false, 3>(x, nullptr, nullptr, 0.f, o, nullptr, n_tok, C, n_bits, status, st)) return true;
    if (n_out == 2 && launch_smooth_multi<false, 2>(x, nullptr, nullptr, 0.f, o, nullptr, n_tok, C, n_bits, status, st)) return true;
    if (n_out == 1 && vq_sm1_mode() && launch_smooth_multi<false, 1>(x, nullptr, nullptr, 0.f, o, nullptr, n_tok, C, n_bits, status, st)) return true;
    return launch_smooth_half<false, 2>(x, nullptr, nullptr, 0.f, o, n_out, nullptr, n_tok, C, n_bits, status, st);
}

// the same for x [2, n_tok, C] with the grids of a token shared by its two samples, optionally behind LayerNorm + modulate
// (shift / scale [2, C], both or neither): smooth_rowquant_multi_kernel<.., PAIR>
bool vq_rowquant_smooth_multi_pair_fast(const half_t* x, const float* shift, const float* scale, float eps, int n_out,
                                        const float* const* s, const float* const* s_rcp, int8_t* const* xq, float* const* sx,
                                        int32_t* const* zx, int32_t* const* R, int n_tok, int C, int Kp, int n_bits,
                                        int32_t* status, hipStream_t st) {
    if (Kp != C || !rq_block_width(C) || n_out < 1 || n_out > 3) return false;
    const LnqOut o = lnq_many(n_out, s, s_rcp, xq, sx, zx, R);
    bool done = false;
    vq_dispatch_bool(shift != nullptr, [&](auto ln) {
        if (n_out == 3) done = launch_smooth_multi<ln(), 3, true>(x, shift, scale, eps, o, nullptr, n_tok, C, n_bits, status, st);
        else if (n_out == 2) done = launch_smooth_multi<ln(), 2, true>(x, shift, scale, eps, o, nullptr, n_tok, C, n_bits, status, st);
        else done = launch_smooth_multi<ln(), 1, true>(x, shift, scale, eps, o, nullptr, n_tok, C, n_bits, status, st);
    });
    return done;
}

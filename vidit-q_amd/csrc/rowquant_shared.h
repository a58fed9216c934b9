// rowquant_shared.h - what the quantizer sources (rowquant.hip, rowquant_fast.hip, rowquant_static.hip; attention.hip for
// the static grid of its fused quantizers) share: the
// functions they call across files, the output struct, the width dispatch of the register-resident kernels, and the
// per-row steps of those kernels - lane maps, reductions, row load, LayerNorm statistics, modulate, the quantize / store /
// row-sum tail - each written once for both lane maps.
#pragma once
#include "vq_common.h"

// ---- host side: what the files call of each other ----------------------------------
// register-resident hot variants (rowquant_fast.hip); false when the shape is not covered (nothing launched)
bool vq_rowquant_fast(const half_t* x, const half_t* add_rows, int add_div, const float* s, const float* s_rcp,
                      int8_t* xq, float* sx, int32_t* zx, int32_t* R, float* zpf, int n_tok, int C, int Kp, int n_bits,
                      int32_t* status, hipStream_t st);
bool vq_rowquant_pair_fast(const half_t* x, int8_t* xq, float* sx, int32_t* zx, int32_t* R, float* zpf, int n_tok, int C,
                           int Kp, int n_bits, int32_t* status, hipStream_t st);
bool vq_rowquant_pair_smooth_fast(const half_t* x, const float* s, const float* s_rcp, int8_t* xq, float* sx, int32_t* zx,
                                  int32_t* R, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st);
bool vq_gelu_rowquant_fast(const half_t* x, const float* s, const float* s_rcp, int8_t* xq, float* sx, int32_t* zx,
                           int32_t* R, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st);
bool vq_gelu_rowquant_pair_fast(const half_t* x, const float* s, const float* s_rcp, int8_t* xq, float* sx, int32_t* zx,
                                int32_t* R, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st);
bool vq_lnq_fast(const half_t* x, const float* shift, const float* scale, float eps, int n_out, const float* const* s,
                 const float* const* s_rcp, int8_t* const* xq, float* const* sx, int32_t* const* zx, int32_t* const* R,
                 half_t* xm, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st);
bool vq_lnq_pair_fast(const half_t* x, const float* shift, const float* scale, float eps, const float* s, const float* s_rcp,
                      int8_t* xq, float* sx, int32_t* zx, int32_t* R, half_t* xm, int n_tok, int C, int Kp, int n_bits,
                      int32_t* status, hipStream_t st);
bool vq_rowquant_smooth_multi_fast(const half_t* x, int n_out, const float* const* s, const float* const* s_rcp,
                                   int8_t* const* xq, float* const* sx, int32_t* const* zx, int32_t* const* R, int n_tok,
                                   int C, int Kp, int n_bits, int32_t* status, hipStream_t st);
bool vq_rowquant_smooth_multi_pair_fast(const half_t* x, const float* shift, const float* scale, float eps, int n_out,
                                        const float* const* s, const float* const* s_rcp, int8_t* const* xq, float* const* sx,
                                        int32_t* const* zx, int32_t* const* R, int n_tok, int C, int Kp, int n_bits,
                                        int32_t* status, hipStream_t st);
// one-pass kernels for a static grid (rowquant_static.hip); false when the shape is not covered, else *rc = the result
bool vq_rowquant_static_one(const half_t* x, const half_t* add_rows, int n_add, int add_div, const float* s, const float* s_rcp,
                            int8_t* xq, float* sx, int32_t* zx, int32_t* R, const float* delta, const float* zp, int n_param,
                            int B, int n_tok, int C, int Kp, int n_bits, hipStream_t st, int* rc);

// up to three quantized outputs of one input (kernel argument)
struct LnqOut {
    const float* s[3];     // smoothing vector of output j, or null
    const float* r[3];     // RN(1 / s) per channel (the kernels that divide through rq_div_rcp), or null
    int8_t* xq[3];
    float* sx[3];
    int32_t* zx[3];
    int32_t* R[3];
};
static LnqOut lnq_many(int n_out, const float* const* s, const float* const* r, int8_t* const* xq, float* const* sx,
                       int32_t* const* zx, int32_t* const* R) {   // s, r: may be null; outputs >= n_out stay null
    LnqOut o{};
    for (int j = 0; j < n_out; ++j) {
        o.s[j] = s ? s[j] : nullptr, o.r[j] = r ? r[j] : nullptr;
        o.xq[j] = xq[j], o.sx[j] = sx[j], o.zx[j] = zx[j], o.R[j] = R[j];
    }
    return o;
}
static LnqOut lnq_one(const float* s, const float* r, int8_t* xq, float* sx, int32_t* zx, int32_t* R) {
    return lnq_many(1, &s, &r, &xq, &sx, &zx, &R);
}

// ---- host side: the dispatch the register-resident quantizers share -----------------
// The half-wave kernels are compiled for rows of C = 128 * NIT channels, NIT in {6, 8, 9, 10}: the hidden sizes 768, 1024,
// 1152 and 1280.  (The sources used to spell this set in two ways; the second, C % 128 == 0 && 768 <= C <= 1280, also let
// 896 through to a width switch that had no kernel for it and fell back - the assert below pins exactly that.)
constexpr bool rq_block_width(int C) { return C % 128 == 0 && (C / 128 == 6 || C / 128 == 8 || C / 128 == 9 || C / 128 == 10); }
constexpr bool rq_block_width_is_both_spellings() {
    for (int C = 0; C <= 8192; ++C) {
        const bool named = C == 1152 || C == 1024 || C == 1280 || C == 768;
        const bool range = C % 128 == 0 && C >= 768 && C <= 1280;
        if (rq_block_width(C) != named || rq_block_width(C) != (range && C != 896)) return false;
    }
    return true;
}
static_assert(rq_block_width_is_both_spellings(), "one predicate for the widths of the half-wave kernels");

// f(std::integral_constant<int, NIT>) and true at a block width, false (nothing launched) at any other C
template <class F>
static bool vq_dispatch_nit(int C, F&& f) {
    const int nit = rq_block_width(C) ? C / 128 : 0;
    switch (nit) {
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 9: f(std::integral_constant<int, 9>{}); break;
        case 10: f(std::integral_constant<int, 10>{}); break;
        default: return false;
    }
    return true;
}

// f(std::integral_constant<int, MAXCH>): the 16-byte chunks per lane the one-row-per-wave kernels hold for a padded row of Kp
template <class F>
static void vq_dispatch_maxch(int Kp, F&& f) {
    if (Kp <= 512) f(std::integral_constant<int, 1>{});
    else if (Kp <= 1536) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 9>{});
}

template <class F>
static void vq_dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// ---- device side: lane -> column maps ------------------------------------------------
// NCH chunks of W consecutive channels per lane, chunk i at column lc + i * STEP of the lane's segment.  The maps fix the
// access width (8-byte row loads and 4-byte code stores in the half-wave map, 16 and 8 in the wave map) and the order in
// which a row is summed: the two orders give different LayerNorm sums, so a kernel names its map.
template <int NIT>
struct RqHalf {              // a half-wave of 32 lanes owns a row of C = 128 * NIT channels (Kp == C): no chunk is masked
    static constexpr bool HALF = true;
    static constexpr int NCH = NIT, W = 4, STEP = 128;
    typedef half4 hvec;
    static __device__ __forceinline__ int lane_col(int lane) { return (lane & 31) * 4; }
};
template <int MAXCH>
struct RqWave {              // a wave owns a row (or a segment of one) of up to MAXCH * 512 padded channels
    static constexpr bool HALF = false;
    static constexpr int NCH = MAXCH, W = 8, STEP = 512;
    typedef half8 hvec;
    static __device__ __forceinline__ int lane_col(int lane) { return lane * 8; }
};

// reduction over the 32 lanes of a half-wave (two rows per wave; ``hi`` = this lane is in the upper half): DPP inside
// each row of 16 lanes, then the two rows of the half through v_readlane
#define RQH_REDUCE2(T_, OP_, v_)                                                                        \
    {                                                                                                   \
        VQ_DPP_STEP(T_, OP_, v_, 0xB1);                                                                 \
        VQ_DPP_STEP(T_, OP_, v_, 0x4E);                                                                 \
        VQ_DPP_STEP(T_, OP_, v_, 0x141);                                                                \
        VQ_DPP_STEP(T_, OP_, v_, 0x140);                                                                \
        const int b_ = __builtin_bit_cast(int, v_);                                                     \
        const T_ r0_ = __builtin_bit_cast(T_, __builtin_amdgcn_readlane(b_, 0));                        \
        const T_ r1_ = __builtin_bit_cast(T_, __builtin_amdgcn_readlane(b_, 16));                       \
        const T_ r2_ = __builtin_bit_cast(T_, __builtin_amdgcn_readlane(b_, 32));                       \
        const T_ r3_ = __builtin_bit_cast(T_, __builtin_amdgcn_readlane(b_, 48));                       \
        v_ = hi ? OP_(r2_, r3_) : OP_(r0_, r1_);                                                        \
    }
// the reductions over a row, chosen by its map (``hi`` is read by the half-wave form only)
#define RQ_ROW_REDUCE(name_, T_, OP_, wave_)                                                            \
    template <bool HALF>                                                                                \
    __device__ __forceinline__ T_ name_(T_ v, bool hi) {                                                \
        if constexpr (HALF) RQH_REDUCE2(T_, OP_, v)                                                     \
        else v = wave_(v);                                                                              \
        return v;                                                                                       \
    }
RQ_ROW_REDUCE(rq_sum_f, float, vq_addf, wave_sum_f)
RQ_ROW_REDUCE(rq_sum_i, int, vq_addi, wave_sum_i)
RQ_ROW_REDUCE(rq_min_f, float, fminf, wave_min_f)
RQ_ROW_REDUCE(rq_max_f, float, fmaxf, wave_max_f)

// ---- device side: row load, LayerNorm statistics, modulate --------------------------
template <int W>
__device__ __forceinline__ void rq_load_f(const float* p, float (&d)[W]) {   // W fp32 values as 16-byte loads
#pragma unroll
    for (int k = 0; k < W / 4; ++k) *reinterpret_cast<float4v*>(d + 4 * k) = *reinterpret_cast<const float4v*>(p + 4 * k);
}
template <class V, int N>
__device__ __forceinline__ void rq_widen(const V& h, float (&w)[N]) {        // a chunk (half4 / half8 / fp32 already) as fp32
#pragma unroll
    for (int e = 0; e < N; ++e) w[e] = (float)h[e];
}

// the lane's chunks of the n channels at ``seg`` into registers (the walking kernels request their next row with it too)
struct RqNoOp {
    template <class... A>
    __device__ __forceinline__ void operator()(A&&...) const {}
};
// ``act(h[i])`` runs on every chunk under the same mask (the GELU in front of fc2's quantizer)
template <class L, class F = RqNoOp>
__device__ __forceinline__ void rq_load_row(const half_t* seg, int lc, int n, typename L::hvec (&h)[L::NCH], F&& act = F{}) {
#pragma unroll
    for (int i = 0; i < L::NCH; ++i)
        if (L::HALF || lc + i * L::STEP < n) {
            h[i] = reinterpret_cast<const typename L::hvec*>(seg + lc)[i * (L::STEP / L::W)];
            act(h[i]);
        }
}
template <class L>
__device__ __forceinline__ void rq_widen_row(const typename L::hvec (&h)[L::NCH], int lc, int n, float (&v)[L::NCH][L::W]) {
#pragma unroll
    for (int i = 0; i < L::NCH; ++i)
        if (L::HALF || lc + i * L::STEP < n) rq_widen(h[i], v[i]);
}

// LayerNorm (no affine) statistics of a register row of C channels, summed in the map's order.  Both spellings of rstd are
// kept as the kernels had them - 1 / C a compile-time constant in the half-wave map and the variance contracted into
// one expression with eps, a run-time 1 / C and a named variance in the wave map - because the fp16 activation the
// static kernels store must equal the dynamic kernels' bit for bit.
template <class L>
__device__ __forceinline__ void rq_ln_stats(const float (&v)[L::NCH][L::W], int lc, int C, float eps, bool hi, float& mu,
                                            float& rstd) {
    float invC;
    if constexpr (L::HALF) invC = 1.0f / (float)(L::STEP * L::NCH);
    else invC = 1.0f / (float)C;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < L::NCH; ++i)
        if (L::HALF || lc + i * L::STEP < C)
#pragma unroll
            for (int e = 0; e < L::W; ++e) sum += v[i][e];
    sum = rq_sum_f<L::HALF>(sum, hi);
    mu = sum * invC;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < L::NCH; ++i)
        if (L::HALF || lc + i * L::STEP < C)
#pragma unroll
            for (int e = 0; e < L::W; ++e) {
                const float d = v[i][e] - mu;
                sq += d * d;
            }
    sq = rq_sum_f<L::HALF>(sq, hi);
    if constexpr (L::HALF) {
        rstd = __fdiv_rn(1.0f, __fsqrt_rn(sq * invC + eps));
    } else {
        const float var = sq * invC;
        rstd = __fdiv_rn(1.0f, __fsqrt_rn(var + eps));
    }
}

// AdaLN modulate of one chunk: v <- ((v - mu) * rstd) * sc1 + sh with sc1 = 1 + scale; returns it rounded to fp16 (the
// modulated activation) and, when ``store``, writes that to xm + at
template <int W>
__device__ __forceinline__ auto rq_modulate(float (&v)[W], float mu, float rstd, const float (&sc1)[W], const float (&sh)[W],
                                            bool store, half_t* xm, size_t at) {
    typedef _Float16 hvec __attribute__((ext_vector_type(W)));
    hvec hm;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        const float y = (v[e] - mu) * rstd;
        const float u = y * sc1[e] + sh[e];
        hm[e] = (half_t)u;
        v[e] = u;
    }
    if (store) *reinterpret_cast<hvec*>(xm + at) = hm;
    return hm;
}
// 1 + scale and shift of W channels
template <int W>
__device__ __forceinline__ void rq_load_mod(const float* scale, const float* shift, float (&sc1)[W], float (&sh)[W]) {
    rq_load_f<W>(scale, sc1);
    rq_load_f<W>(shift, sh);
#pragma unroll
    for (int e = 0; e < W; ++e) sc1[e] = 1.0f + sc1[e];
}

// ---- device side: GELU ----------------------------------------------------------------
// nn.GELU(approximate='tanh') = x * sigmoid(2u), u = sqrt(2/pi)(x + 0.044715 x^3) (same form as gemm_i8.hip) on N fp16 values
// as packed fp32 math (v_pk_mul / v_pk_fma / v_pk_add: IEEE-identical to the scalar forms, two elements per issue slot;
// exp2 and rcp stay per element), result rounded to fp16 like the activation the reference stores between the two Linears
template <int N, class V>
__device__ __forceinline__ void rq_gelu_tanh(V& h) {
    const float2v c1 = {-0.044715f * 2.302208198f, -0.044715f * 2.302208198f}, c2 = {-2.302208198f, -2.302208198f};
    const float2v one = {1.0f, 1.0f};
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const float2v x = {(float)h[2 * j], (float)h[2 * j + 1]};
        const float2v w = x * __builtin_elementwise_fma(x * x, c1, c2);
        const float2v d = float2v{__builtin_amdgcn_exp2f(w[0]), __builtin_amdgcn_exp2f(w[1])} + one;
        const float2v g = x * float2v{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
        h[2 * j] = (half_t)g[0];
        h[2 * j + 1] = (half_t)g[1];
    }
}

// ---- device side: codes ---------------------------------------------------------------
// what the code width fixes: the last level, the int8 offset of 8-bit codes and its form on a packed dword
struct RqWidth {
    float qmax;
    int cx;
    uint32_t flip;
};
__device__ __forceinline__ RqWidth rq_width(int n_bits) {
    return {(float)((1 << n_bits) - 1), n_bits == 8 ? 128 : 0, n_bits == 8 ? 0x80808080u : 0u};
}

// one kernel-uniform branch on the code width around a whole store loop: SAT8_ (8-bit codes) = v_cvt_pk_u8_f32 saturates to
// [0, 255] by itself, other widths clamp first (as a per-element select it cost a v_med3 + v_cndmask per code)
#define RQ_BY_WIDTH(qmax_, ...)                                       \
    if ((qmax_) == 255.0f) {                                          \
        constexpr bool SAT8_ = true;                                  \
        __VA_ARGS__                                                   \
    } else {                                                          \
        constexpr bool SAT8_ = false;                                 \
        __VA_ARGS__                                                   \
    }

// N integer-valued (or infinite) levels -> N / 4 dwords of raw codes
template <int N, bool SAT8>
__device__ __forceinline__ void rq_pack_codes(const float (&q)[N], float qmax, uint32_t (&pk)[N / 4]) {
    static_assert(N % 4 == 0, "dwords of codes");
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = q[4 * k + e];
            if constexpr (!SAT8) v = __builtin_amdgcn_fmed3f(v, 0.0f, qmax);
            w = __builtin_amdgcn_cvt_pk_u8_f32(v, e, w);      // saturates to [0, 255]
        }
        pk[k] = w;
    }
}
// quantize N values of one lane on the row's own grid (tie test shared by the group, see rq_round_group)
template <int N, bool SAT8>
__device__ __forceinline__ void rq_quant(const float (&v)[N], float inv, float delta, float zp, float qmax, uint32_t (&pk)[N / 4]) {
    float r[N];
    rq_round_group<N>(v, inv, delta, zp, r);
    rq_pack_codes<N, SAT8>(r, qmax, pk);
}
template <int W>
__device__ __forceinline__ void rq_store_codes(int8_t* dst, const uint32_t (&pk)[W / 4]) {
    if constexpr (W == 8) *reinterpret_cast<uint2*>(dst) = make_uint2(pk[0], pk[1]);
    else *reinterpret_cast<uint32_t*>(dst) = pk[0];
}

// ---- device side: codes on a static (calibrated) grid ---------------------------------
// (rowquant_static.hip and the static-grid forms of the fused temporal attention kernels, attention.hip)
// round(x / delta) on a grid the row did not define.  rq_round_group's bound assumes |x / delta| <= 255; here a value
// may lie anywhere (+-65504 against delta = 2^-k).  The product form is kept, with a window and a guard per (row,
// output) - rqs_grid():
//   inv = RN(1 / delta), t = RN(x inv), q = x / delta (exact), Q = RN(q) (what the oracle rounds).
//   t = q (1 + e1)(1 + e2), |e| <= 2^-24 (inv is required to be a normal number, t is normal or rounds to 0 with Q),
//   and |Q - q| <= |q| 2^-24, so |t - Q| <= 1.5 * 2^-23 (1 + 2^-22) |t| < 1.8e-7 |t|.
//   Window W = qmax + |zp| + 2 (zp integer-valued: the precondition).  INSIDE, |t| <= W: |t - Q| < 1.8e-7 W < G with
//   the guard G = max(1e-4, 2.4e-7 W); when |t - rint(t)| <= 0.5 - G, Q lies strictly between the same two ties as t
//   and rint(Q) = rint(t); every other lane takes rint(__fdiv_rn(x, delta)), ties included.  (t - rint(t) is exact.)
//   OUTSIDE, t > W: rint(t) >= W, so rint(t) + zp >= qmax + 2; and Q > (1 - 1.8e-7) W, so rint(Q) >= W - 1 as long as
//   1.8e-7 W < 0.5, i.e. rint(Q) + zp >= qmax + 1: both clamp to qmax (t < -W: both to 0) whichever way each rounds -
//   and a lane out there that fails the guard merely divides.  For W >= 2^21 (no calibrated grid: |zp| <= qmax) the
//   guard 0.5 - G is negative and EVERY lane divides, so no W exists for which the outside argument is needed but
//   fails.  inv outside [1e-30, 1e30] or NaN: guard -1, every lane divides.  +-inf products fail the guard (NaN
//   distance) and divide.  Codes are therefore the oracle's for every input.

// the grid of one (row, output): step, zero point, reciprocal and the tie guard of the product form (above)
struct RqsGrid {
    float delta, zp, inv, thr;
};
__device__ __forceinline__ RqsGrid rqs_grid(const float* __restrict__ delta, const float* __restrict__ zp, int p, float qmax) {
    RqsGrid g;
    g.delta = delta[p];
    g.zp = zp[p];
    g.inv = __fdiv_rn(1.0f, g.delta);
    const float w = qmax + fabsf(g.zp) + 2.0f;
    g.thr = 0.5f - fmaxf(1.0e-4f, w * 2.4e-7f);
    if (!(g.inv >= 1.0e-30f && g.inv <= 1.0e30f)) g.thr = -1.0f;
    return g;
}

// N values -> N / 4 dwords of raw codes clamp(rint(RN(x / delta)) + zp, 0, qmax); one tie test for the group
template <int N, bool SAT8>
__device__ __forceinline__ void rqs_quant(const float (&x)[N], const RqsGrid& g, float qmax, uint32_t (&pk)[N / 4]) {
    static_assert(N % 4 == 0, "dwords of codes");
    const float2v inv2 = {g.inv, g.inv};
    float r[N], t[N];
    float far = 0.f;
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const float2v t2 = float2v{x[2 * j], x[2 * j + 1]} * inv2;
        t[2 * j] = t2[0];
        t[2 * j + 1] = t2[1];
        r[2 * j] = __builtin_rintf(t2[0]);
        r[2 * j + 1] = __builtin_rintf(t2[1]);
        const float2v d = t2 - float2v{r[2 * j], r[2 * j + 1]};
        far = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(d[0]), __builtin_fabsf(d[1])), far);
    }
    if (!(far <= g.thr)) {                               // (also taken by a NaN distance: an infinite product)
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (!(__builtin_fabsf(t[i] - r[i]) <= g.thr)) r[i] = rintf(__fdiv_rn(x[i], g.delta));
    }
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] += g.zp;
    rq_pack_codes<N, SAT8>(r, qmax, pk);
}

// ---- device side: the dynamic tail ----------------------------------------------------
// Quantize the lane's chunks of a register row (half or fp32 chunks; ``pre(i, c, w)`` may finish chunk i at column c
// first) on the row's grid, store the codes (``live``) at qseg - zeros in the pad columns [n, np) of the wave map - and
// return csum + the sum of the lane's raw codes (v_sad_u8).  VALU bounds these kernels at C = 1152, so the per-element
// sequence is minimal: the row's own min / max defines delta, hence |x / delta| <= 255 and no magnitude guard; 8-bit codes
// need no clamp.  The half-wave map branches on the width once around its loop (RQ_BY_WIDTH); the wave map once per chunk
// of 8, which keeps one copy of the stores.
template <class L, class T, class F = RqNoOp>
__device__ __forceinline__ uint32_t rq_quant_lane(const T (&row)[L::NCH], int lc, int n, int np, float delta, float zp,
                                                  float inv, const RqWidth& wd, int8_t* qseg, bool live,
                                                  uint32_t csum = 0, F&& pre = F{}) {
    constexpr int W = L::W;
    int8_t* ql = qseg + lc;
    auto input = [&](int i, float (&w)[W]) {
        rq_widen(row[i], w);
        pre(i, lc + i * L::STEP, w);
    };
    auto put = [&](int i, uint32_t (&pk)[W / 4]) {
#pragma unroll
        for (int k = 0; k < W / 4; ++k) {
            csum = __builtin_amdgcn_sad_u8(pk[k], 0u, csum);
            pk[k] ^= wd.flip;
        }
        if (live) rq_store_codes<W>(ql + i * L::STEP, pk);
    };
    if constexpr (L::HALF) {
        RQ_BY_WIDTH(wd.qmax, _Pragma("unroll") for (int i = 0; i < L::NCH; ++i) {
            float w[W];
            uint32_t pk[W / 4];
            input(i, w);
            rq_quant<W, SAT8_>(w, inv, delta, zp, wd.qmax, pk);
            put(i, pk);
        })
    } else {
#pragma unroll
        for (int i = 0; i < L::NCH; ++i) {
            const int c = lc + i * L::STEP;
            if (c < n) {
                float w[W];
                uint32_t pk[W / 4];
                input(i, w);
                RQ_BY_WIDTH(wd.qmax, rq_quant<W, SAT8_>(w, inv, delta, zp, wd.qmax, pk);)   // wave-uniform
                put(i, pk);
            } else if (c < np) {
                const uint32_t zero[W / 4] = {};
                if (live) rq_store_codes<W>(ql + i * L::STEP, zero);
            }
        }
    }
    return csum;
}
// the same, reduced over the row: the sum of its raw codes
template <class L, class T, class F = RqNoOp>
__device__ __forceinline__ int rq_quant_row(const T (&row)[L::NCH], int lc, int n, int np, float delta, float zp, float inv,
                                            const RqWidth& wd, int8_t* qseg, bool live, bool hi, F&& pre = F{}) {
    return rq_sum_i<L::HALF>((int)rq_quant_lane<L>(row, lc, n, np, delta, zp, inv, wd, qseg, live, 0u, pre), hi);
}
// step, zero point and row term of row r as the int8 GEMM reads them (one lane of the row calls this); zpf: may be null
__device__ __forceinline__ void rq_write_row(float* sx, int32_t* zx, int32_t* R, float* zpf, size_t r, float delta, float zp,
                                             int code_sum, int C, int cx) {
    const int izx = (int)zp - cx;
    sx[r] = delta;
    zx[r] = izx;
    R[r] = code_sum - cx * C - C * izx;
    if (zpf) zpf[r] = zp;
}

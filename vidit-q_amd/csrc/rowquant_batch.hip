// rowquant_batch.hip - one-pass per-token quantizers for batched forwards of 3 to 16 samples (vq_rowquant_batch).
//
// The reference shares a token's dynamic grid over the whole batch (base_quantizer.py:177-189), so a kernel has to see all B
// rows of a token before it encodes one.  rowquant_fast.hip does that for B = 1 (register rows) and B = 2 (wave pairs);
// above that the generic kernels of rowquant.hip read every row twice (LayerNorm: four times) and divide the IEEE way per
// element and output, vq_gelu_rowquant refuses, and vq_ln_modulate_rowquant stops at B = 8.  Here:
//   - a TOKEN GROUP is B waves of one workgroup, wave b owns row (b, tok): loaded once (16 bytes per lane, the wave lane
//     map RqWave<MAXCH>), kept in registers - packed fp16, or the fp32 modulated row behind LayerNorm (Kp <= 1536 there);
//   - the per-row steps are the shared ones (rowquant_shared.h): rq_gelu_tanh on the chunks as they arrive, rq_ln_stats in
//     the wave map's order, rq_load_mod / rq_modulate with sample b's shift / scale, rq_quant_row, rq_write_row;
//   - ONE exchange: lane 0 of every wave puts its n_out (min, max) pairs in LDS, one barrier, every wave of the group
//     reduces the B entries of its token in sample order and calls vq_row_grid - all B waves hold the identical grid;
//   - the smoothing vectors and their reciprocals live in LDS, staged once per workgroup ([n_out][s | r][C] floats), and the
//     quotient (rq_div_rcp with a reciprocal, __fdiv_rn without, the value itself without a vector) is computed in the
//     min / max pass and AGAIN in the encode pass: no second fp32 copy of a 4608-channel row, 128 VGPRs per wave hold;
//   - G = max(1, 16 / B) token groups per workgroup (B * G <= 16 waves); a group past n_tok clamps its token, stays for the
//     barrier and writes nothing; a workgroup walks tokens grid-stride (parity-double-buffered exchange slots), nothing is
//     prefetched or pipelined across tokens.
// Plain, smoothed and GELU arms: the values, their order-free min / max and the codes of the kernels they replace, bit for
// bit.  LayerNorm arm: the wave map's summation order (ln_modulate_rowquant_fast_kernel's), DESIGN section 4.
#include "vq_common.h"
#include "rowquant_shared.h"

#define RQB_MAX_B 16                 // samples = waves of one token group; also the waves of a workgroup
#define RQB_MAX_KP 4608
#define RQB_LN_MAX_KP 1536           // the LayerNorm arm keeps the modulated row in fp32: three chunks per lane
#define RQB_MAX_GRID 1024

enum { RQB_PLAIN = 0, RQB_GELU = 1, RQB_LN = 2 };
enum { RQB_Q_NONE = 0, RQB_Q_RCP = 1, RQB_Q_DIV = 2 };   // the quotient of one output: none, reciprocal form, IEEE division

// q = u / s of one chunk at column c0; sp / rp: the output's vector and reciprocal in LDS (q may be u itself)
__device__ __forceinline__ void rqb_quotient(const float (&u)[8], const float* sp, const float* rp, int mode, int c0,
                                             float (&q)[8]) {
    if (mode == RQB_Q_NONE) {                             // (kernel-uniform)
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = u[e];
        return;
    }
    float sv[8];
    rq_load_f<8>(sp + c0, sv);
    if (mode == RQB_Q_RCP) {
        float rv[8];
        rq_load_f<8>(rp + c0, rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = rq_div_rcp(u[e], sv[e], rv[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = __fdiv_rn(u[e], sv[e]);
    }
}

// Nine chunks per lane (rows beyond 1536 channels): every pass over the packed row - min / max and encode, of every output -
// must widen (and divide) it AGAIN.  Left to itself the compiler keeps one pass's fp32 values for the next (common
// subexpressions: 72 more registers, spilled by a 128-register wave); passing the packed registers through an empty asm in
// front of a pass makes them new values to it.
template <int MAXCH>
__device__ __forceinline__ void rqb_forget_widened(half8 (&h)[MAXCH]) {
    if constexpr (MAXCH > 3) {
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) asm volatile("" : "+v"(h[i]));
    }
}

// f(std::integral_constant<int, j>) for every output j < NOUT (a compile-time index: no table is indexed at run time)
template <int NOUT, class F>
__device__ __forceinline__ void rqb_each_output(F&& f) {
    f(std::integral_constant<int, 0>{});
    if constexpr (NOUT > 1) f(std::integral_constant<int, 1>{});
    if constexpr (NOUT > 2) f(std::integral_constant<int, 2>{});
}

template <int MAXCH, int NOUT, int ARM>
__global__ __launch_bounds__(64 * RQB_MAX_B) void rowquant_batch_kernel(
    const half_t* __restrict__ x, const float* __restrict__ shift, const float* __restrict__ scale, float ln_eps, LnqOut o,
    half_t* __restrict__ xm_out, int B, int G, int n_tok, int C, int Kp, int n_bits, int32_t* status) {
    using L = RqWave<MAXCH>;
    extern __shared__ __attribute__((aligned(16))) float rqb_lds[];   // [NOUT][s | r][C]
    __shared__ float pm[2][RQB_MAX_B][NOUT][2];                         // [walk parity][wave][output][min | max]
    int mode[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) mode[j] = !o.s[j] ? RQB_Q_NONE : (o.r[j] ? RQB_Q_RCP : RQB_Q_DIV);
    for (int c = threadIdx.x * 4; c < C; c += blockDim.x * 4) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            if (mode[j] != RQB_Q_NONE)
                *reinterpret_cast<float4v*>(rqb_lds + (2 * j) * C + c) = *reinterpret_cast<const float4v*>(o.s[j] + c);
            if (mode[j] == RQB_Q_RCP)
                *reinterpret_cast<float4v*>(rqb_lds + (2 * j + 1) * C + c) = *reinterpret_cast<const float4v*>(o.r[j] + c);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = wv / B, b = wv - g * B, lc = L::lane_col(lane);
    const RqWidth wd = rq_width(n_bits);
    int par = 0;
    for (int t0 = blockIdx.x * G; t0 < n_tok; t0 += gridDim.x * G, par ^= 1) {     // (workgroup-uniform trip count)
        const bool live = t0 + g < n_tok;                 // a dead group stays for the barrier and writes nothing
        const size_t row = (size_t)b * n_tok + (live ? t0 + g : n_tok - 1);
        half8 h[MAXCH];
        float v[ARM == RQB_LN ? MAXCH : 1][8];           // the modulated row (LayerNorm arm)
        if constexpr (ARM == RQB_GELU) rq_load_row<L>(x + row * C, lc, C, h, [](half8& c8) { rq_gelu_tanh<8>(c8); });
        else rq_load_row<L>(x + row * C, lc, C, h);
        float mu = 0.f, rstd = 0.f;
        if constexpr (ARM == RQB_LN) {
            rq_widen_row<L>(h, lc, C, v);
            rq_ln_stats<L>(v, lc, C, ln_eps, false, mu, rstd);
        }
        if constexpr (ARM == RQB_LN) {
#pragma unroll
            for (int i = 0; i < MAXCH; ++i) {
                const int c0 = lc + i * 512;
                if (c0 < C) {
                    float sc1[8], sh[8];
                    rq_load_mod<8>(scale + (size_t)b * C + c0, shift + (size_t)b * C + c0, sc1, sh);
                    rq_modulate<8>(v[i], mu, rstd, sc1, sh, xm_out != nullptr && live, xm_out, row * C + c0);
                }
            }
        }
        // output by output (one running min / max and one pair of vector chunks in flight at a time)
        rqb_each_output<NOUT>([&](auto jc) {
            constexpr int j = jc();
            rqb_forget_widened<MAXCH>(h);
            float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < MAXCH; ++i) {
                const int c0 = lc + i * 512;
                if (c0 < C) {
                    float q[8];
                    if constexpr (ARM == RQB_LN) rq_widen(v[i], q);
                    else rq_widen(h[i], q);
                    rqb_quotient(q, rqb_lds + (2 * j) * C, rqb_lds + (2 * j + 1) * C, mode[j], c0, q);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        vmin = fminf(vmin, q[e]);
                        vmax = fmaxf(vmax, q[e]);
                    }
                }
            }
            vmin = rq_min_f<L::HALF>(vmin, false);
            vmax = rq_max_f<L::HALF>(vmax, false);
            if (lane == 0) {
                pm[par][wv][j][0] = vmin;
                pm[par][wv][j][1] = vmax;
            }
        });
        __syncthreads();
        rqb_each_output<NOUT>([&](auto jc) {
            constexpr int j = jc();
            rqb_forget_widened<MAXCH>(h);
            float mn = pm[par][g * B][j][0], mx = pm[par][g * B][j][1];
            for (int sb = 1; sb < B; ++sb) {               // the token's B samples, in sample order
                mn = fminf(mn, pm[par][g * B + sb][j][0]);
                mx = fmaxf(mx, pm[par][g * B + sb][j][1]);
            }
            float delta, zp, inv;
            bool small;
            vq_row_grid(mn, mx, wd.qmax, delta, zp, small, inv);
            if (small && lane == 0 && b == 0 && live && status) atomicOr(status, VQ_ST_EPSFILL);   // once per token
            const float* sp = rqb_lds + (2 * j) * C;
            const int mj = mode[j];
            auto quot = [&](int, int c0, float (&w)[8]) {
                rqb_quotient(w, sp, sp + C, mj, c0, w);
            };
            int8_t* qrow = o.xq[j] + row * Kp;
            int cs;
            if constexpr (ARM == RQB_LN) cs = rq_quant_row<L>(v, lc, C, Kp, delta, zp, inv, wd, qrow, live, false, quot);
            else cs = rq_quant_row<L>(h, lc, C, Kp, delta, zp, inv, wd, qrow, live, false, quot);
            if (lane == 0 && live) rq_write_row(o.sx[j], o.zx[j], o.R[j], nullptr, row, delta, zp, cs, C, wd.cx);
        });
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <int ARM>
static int rqb_launch(const half_t* x, const float* shift, const float* scale, float eps, const LnqOut& o, int n_out, half_t* xm,
                      int B, int n_tok, int C, int Kp, int n_bits, int32_t* status, hipStream_t st) {
    const int G = 16 / B > 1 ? 16 / B : 1;                 // token groups per workgroup: B * G <= 16 waves
    const int groups = (n_tok + G - 1) / G;
    const dim3 grid(groups < RQB_MAX_GRID ? groups : RQB_MAX_GRID), block(64 * B * G);
    int lds = 0;
    for (int j = 0; j < n_out; ++j)
        if (o.s[j]) lds = 2 * n_out * C * (int)sizeof(float);
    int rc = VQ_EUNSUP;
    vq_dispatch_maxch(Kp, [&](auto m) {
        auto go = [&](auto nout) {
            if constexpr ((ARM == RQB_LN && m() > 3) || (ARM == RQB_GELU && nout() > 1)) {
                return;                                     // (refused by the entry point: no such instantiation)
            } else {
                constexpr auto k = rowquant_batch_kernel<m(), nout(), ARM>;
                if (lds > 48 * 1024) {                      // two or three smoothed outputs of rows beyond 2048 channels
                    rc = vq_prepare_kernel<k>(2 * 3 * RQB_MAX_KP * (int)sizeof(float));
                    if (rc != VQ_OK) return;
                }
                hipLaunchKernelGGL(k, grid, block, lds, st, x, shift, scale, eps, o, xm, B, G, n_tok, C, Kp, n_bits, status);
                rc = vq_check_launch();
            }
        };
        if (n_out == 1) go(std::integral_constant<int, 1>{});
        else if (n_out == 2) go(std::integral_constant<int, 2>{});
        else go(std::integral_constant<int, 3>{});
    });
    return rc;
}

extern "C" int vq_rowquant_batch(const void* x, const float* shift, const float* scale, float ln_eps, int act, int n_out,
                                 const float* const* s, const float* const* s_rcp, int8_t* const* xq, float* const* sx,
                                 int32_t* const* zx, int32_t* const* R, void* xm_out, int B, int n_tok, int C, int Kp,
                                 int n_bits, int32_t* status, void* stream) {
    // 1. pointers, counts and the arm
    if (!x || !xq || !sx || !zx || !R || (shift == nullptr) != (scale == nullptr)) return VQ_EINVAL;
    if (n_out < 1 || B <= 0 || n_tok <= 0 || C <= 0 || (long)B * n_tok > 0x7fffffffL) return VQ_EINVAL;
    if ((act != 0 && act != 1) || (act == 1 && shift) || (xm_out && !shift)) return VQ_EINVAL;
    const int n_tab = n_out < 3 ? n_out : 3;               // (the tables hold n_out entries; more than three is refused below)
    for (int j = 0; j < n_tab; ++j)
        if (!xq[j] || !sx[j] || !zx[j] || !R[j]) return VQ_EINVAL;
    // 2. the shape, the code width, 16-byte loads and 8-byte stores
    if (const int e = rq_check_shape(C, Kp, n_bits)) return e;
    if (rq_off16(x) || rq_off16(shift) || rq_off16(scale) || rq_off16(xm_out)) return VQ_ESHAPE;
    for (int j = 0; j < n_tab; ++j)
        if (rq_off16(s ? s[j] : nullptr) || rq_off16((s && s[j] && s_rcp) ? s_rcp[j] : nullptr) || rq_off16(xq[j])) return VQ_ESHAPE;
    // 3. / 4. what the kernel family holds
    if (B > RQB_MAX_B) return VQ_ESHAPE;
    if (B < 3 || Kp > RQB_MAX_KP || n_out > 3 || (n_out > 1 && act == 1)) return VQ_EUNSUP;
    if (shift && Kp > RQB_LN_MAX_KP) return VQ_EUNSUP;
    LnqOut o = lnq_many(n_out, s, nullptr, xq, sx, zx, R);
    for (int j = 0; j < n_out; ++j) o.r[j] = (o.s[j] && s_rcp) ? s_rcp[j] : nullptr;   // a reciprocal without a vector is not read
    const half_t* xh = (const half_t*)x;
    hipStream_t st = (hipStream_t)stream;
    if (shift) return rqb_launch<RQB_LN>(xh, shift, scale, ln_eps, o, n_out, (half_t*)xm_out, B, n_tok, C, Kp, n_bits, status, st);
    if (act) return rqb_launch<RQB_GELU>(xh, nullptr, nullptr, 0.f, o, n_out, nullptr, B, n_tok, C, Kp, n_bits, status, st);
    return rqb_launch<RQB_PLAIN>(xh, nullptr, nullptr, 0.f, o, n_out, nullptr, B, n_tok, C, Kp, n_bits, status, st);
}

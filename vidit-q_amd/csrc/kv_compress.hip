// kv_compress.hip - PixArt-Sigma key / value token compression and the q / k LayerNorms (PixArt_blocks.py:99-124, 135-146)
// in ONE launch between the fused qkv GEMM and vq_attn_fwd.
//
// Work split.  One wave owns one output token for its whole life: the LayerNorm of a token is a wave reduction (DPP +
// readlane, vq_common.h) and nothing crosses waves, so the only barrier of the kernel is the one behind the weight stage.
// A lane holds the 16-byte pieces lane, lane + 64, ... of a C-channel row (C = 1152: 144 pieces, 2.25 per lane, NP = 3 with
// the last round masked), so every load and store of a wave is one contiguous run of the row.  k and v of a token are
// handled by the same wave: the index arithmetic, the depthwise weights and the final LayerNorm's vectors are fetched once
// for both.  The grid is persistent (a few workgroups per CU, item = token, grid stride): the depthwise weights are
// transposed into LDS once per workgroup ([C][sr^2] as the convolution stores them -> [sr^2][C], so that a lane reads its
// 8 channels of a tap as two ds_read_b128), not once per token.
//
// Data movement of the 'conv' arm, per output token: for each of the sr rows of the sr x sr window, the 2 sr input rows
// (k and v of sr neighbouring tokens) are requested as raw half8 pieces before any of them is used - 2 sr NP 16-byte loads
// in flight per lane - then each is widened, k optionally normalised in registers (k_norm, rounded to fp16 where the torch
// route rounds) and accumulated into the two fp32 convolution rows.  Only one window row plus the two accumulators is live:
// sr = 4 costs the registers of sr = 2 twice over in raw pieces only.  The q LayerNorm (in place in the q | k | v buffer)
// runs as further items of the same grid: item >= B Lk is q row item - B Lk.
//
// Every LayerNorm is two-pass (mean, then the centred sum of squares), rstd = 1 / sqrt(var + eps) correctly rounded, as
// rq_ln_stats (rowquant_shared.h).  Without q_norm the q columns are never read or written; nothing outside
// [row * ld + C, row * ld + 3 C) of a row is touched.
#include "vq_common.h"

#define KVC_WAVES 4
#define KVC_THREADS (64 * KVC_WAVES)
#define KVC_MAX_C 2048
#define KVC_WG_PER_CU 4

struct KvcArgs {
    half_t* qkv;
    long ld;
    const float *sr_w, *sr_b, *n_w, *n_b, *kn_w, *kn_b, *qn_w, *qn_b;
    float n_eps, kn_eps, qn_eps;
    half_t *k_out, *v_out;
    int N, W, Wo, Lk, C, sr;
    int n_kv, n_q;      // items: B * Lk output tokens, then B * N q rows (0 without q_norm)
};

template <int NP>
struct KvcLane {        // the lane's pieces of a C-channel row
    int c[NP];
    bool live[NP];
    __device__ __forceinline__ KvcLane(int lane, int C) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            c[i] = 8 * (lane + 64 * i);
            live[i] = c[i] < C;
        }
    }
};

template <int NP>
__device__ __forceinline__ void kvc_load(const half_t* row, const KvcLane<NP>& L, half8 (&h)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i)
        if (L.live[i]) h[i] = *reinterpret_cast<const half8*>(row + L.c[i]);
}
template <int NP>
__device__ __forceinline__ void kvc_store(half_t* row, const KvcLane<NP>& L, const half8 (&h)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i)
        if (L.live[i]) *reinterpret_cast<half8*>(row + L.c[i]) = h[i];
}
template <int NP>
__device__ __forceinline__ void kvc_widen(const half8 (&h)[NP], const KvcLane<NP>& L, float (&x)[NP][8]) {
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) x[i][e] = L.live[i] ? (float)h[i][e] : 0.f;
}
__device__ __forceinline__ void kvc_load8(const float* p, float (&d)[8]) {
    *reinterpret_cast<float4v*>(d) = *reinterpret_cast<const float4v*>(p);
    *reinterpret_cast<float4v*>(d + 4) = *reinterpret_cast<const float4v*>(p + 4);
}

// affine LayerNorm of a register row (dead pieces hold 0), rounded to fp16 once
template <int NP>
__device__ __forceinline__ void kvc_layernorm(const float (&x)[NP][8], const KvcLane<NP>& L, float invC, float eps,
                                              const float* w, const float* b, half8 (&out)[NP]) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += x[i][e];
    const float mu = wave_sum_f(sum) * invC;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = L.live[i] ? x[i][e] - mu : 0.f;
            sq += d * d;
        }
    const float var = wave_sum_f(sq) * invC;
    const float rstd = __fdiv_rn(1.0f, __fsqrt_rn(var + eps));
#pragma unroll
    for (int i = 0; i < NP; ++i)
        if (L.live[i]) {
            float wv[8], bv[8];
            kvc_load8(w + L.c[i], wv);
            kvc_load8(b + L.c[i], bv);
#pragma unroll
            for (int e = 0; e < 8; ++e) out[i][e] = (half_t)(((x[i][e] - mu) * rstd) * wv[e] + bv[e]);
        }
}

// CONV: SR is the window; picks: SR unused (the factor is a.sr), FLAT = every sr-th token of the flat sequence
template <int NP, int SR, bool CONV, bool FLAT, bool KNORM>
__global__ __launch_bounds__(KVC_THREADS) void kv_compress_kernel(const KvcArgs a) {
    extern __shared__ float kvc_w[];                    // [SR * SR][C] depthwise weights (CONV)
    const int C = a.C;
    if constexpr (CONV) {
        constexpr int T = SR * SR;
        for (int i = threadIdx.x; i < C * T; i += KVC_THREADS) kvc_w[(i % T) * C + i / T] = a.sr_w[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const KvcLane<NP> L(lane, C);
    const float invC = 1.0f / (float)C;
    const int total = a.n_kv + a.n_q;
    for (int item = blockIdx.x * KVC_WAVES + wv; item < total; item += gridDim.x * KVC_WAVES) {
        if (item >= a.n_kv) {                           // ---- q_norm, in place
            half_t* row = a.qkv + (size_t)(item - a.n_kv) * a.ld;
            half8 h[NP];
            float x[NP][8];
            kvc_load<NP>(row, L, h);
            kvc_widen<NP>(h, L, x);
            kvc_layernorm<NP>(x, L, invC, a.qn_eps, a.qn_w, a.qn_b, h);
            kvc_store<NP>(row, L, h);
            continue;
        }
        const int b = item / a.Lk, r = item - b * a.Lk;
        half_t* ko = a.k_out + (size_t)item * C;
        half_t* vo = a.v_out + (size_t)item * C;
        if constexpr (!CONV) {                          // ---- picks: one source token
            int tok;
            if constexpr (FLAT) {
                tok = r * a.sr;
            } else {
                const int i = r / a.Wo, j = r - i * a.Wo;
                tok = i * a.sr * a.W + j * a.sr;
            }
            const half_t* src = a.qkv + ((size_t)b * a.N + tok) * a.ld + C;
            half8 hk[NP], hv[NP];
            kvc_load<NP>(src, L, hk);
            kvc_load<NP>(src + C, L, hv);
            if constexpr (KNORM) {
                float x[NP][8];
                kvc_widen<NP>(hk, L, x);
                kvc_layernorm<NP>(x, L, invC, a.kn_eps, a.kn_w, a.kn_b, hk);
            }
            kvc_store<NP>(ko, L, hk);
            kvc_store<NP>(vo, L, hv);
        } else {                                        // ---- depthwise sr x sr convolution + LayerNorm
            const int i = r / a.Wo, j = r - i * a.Wo;
            const half_t* win = a.qkv + ((size_t)b * a.N + (size_t)i * SR * a.W + j * SR) * a.ld + C;
            float ak[NP][8], av[NP][8];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (L.live[p]) {
                    kvc_load8(a.sr_b + L.c[p], ak[p]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) ak[p][e] = 0.f;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) av[p][e] = ak[p][e];
            }
#pragma unroll
            for (int di = 0; di < SR; ++di) {
                half8 hk[SR][NP], hv[SR][NP];
#pragma unroll
                for (int dj = 0; dj < SR; ++dj) {       // the window row's 2 SR input rows, all requested first
                    const half_t* src = win + ((size_t)di * a.W + dj) * a.ld;
                    kvc_load<NP>(src, L, hk[dj]);
                    kvc_load<NP>(src + C, L, hv[dj]);
                }
#pragma unroll
                for (int dj = 0; dj < SR; ++dj) {
                    float xk[NP][8], xv[NP][8];
                    kvc_widen<NP>(hk[dj], L, xk);
                    kvc_widen<NP>(hv[dj], L, xv);
                    if constexpr (KNORM) {
                        kvc_layernorm<NP>(xk, L, invC, a.kn_eps, a.kn_w, a.kn_b, hk[dj]);
                        kvc_widen<NP>(hk[dj], L, xk);   // (rounded to fp16: the torch route's and the reference's point)
                    }
                    const float* wt = kvc_w + (di * SR + dj) * C;
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        if (L.live[p]) {
                            float w8[8];
                            kvc_load8(wt + L.c[p], w8);
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                ak[p][e] = __builtin_fmaf(w8[e], xk[p][e], ak[p][e]);
                                av[p][e] = __builtin_fmaf(w8[e], xv[p][e], av[p][e]);
                            }
                        }
                }
            }
            half8 ok[NP], ov[NP];
            kvc_layernorm<NP>(ak, L, invC, a.n_eps, a.n_w, a.n_b, ok);
            kvc_layernorm<NP>(av, L, invC, a.n_eps, a.n_w, a.n_b, ov);
            kvc_store<NP>(ko, L, ok);
            kvc_store<NP>(vo, L, ov);
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <int NP, int SR, bool CONV, bool FLAT, bool KNORM>
static int kvc_launch(const KvcArgs& a, hipStream_t st) {
    constexpr auto k = kv_compress_kernel<NP, SR, CONV, FLAT, KNORM>;
    const int lds = CONV ? SR * SR * a.C * (int)sizeof(float) : 0;
    int ncu = 0;
    const int e = vq_prepare_kernel<k>(CONV ? SR * SR * KVC_MAX_C * (int)sizeof(float) : 1024, &ncu);
    if (e != VQ_OK) return e;
    const long total = (long)a.n_kv + a.n_q;
    const long wgs = (total + KVC_WAVES - 1) / KVC_WAVES, cap = (long)ncu * KVC_WG_PER_CU;
    hipLaunchKernelGGL(k, dim3((unsigned)(wgs < cap ? wgs : cap)), dim3(KVC_THREADS), lds, st, a);
    return vq_check_launch();
}

template <int NP>
static int kvc_dispatch(const KvcArgs& a, int mode, hipStream_t st) {
    const bool kn = a.kn_w != nullptr;
    if (mode == VQ_KVC_CONV) {
        if (a.sr == 2) return kn ? kvc_launch<NP, 2, true, false, true>(a, st) : kvc_launch<NP, 2, true, false, false>(a, st);
        return kn ? kvc_launch<NP, 4, true, false, true>(a, st) : kvc_launch<NP, 4, true, false, false>(a, st);
    }
    if (mode == VQ_KVC_PICK) return kn ? kvc_launch<NP, 1, false, false, true>(a, st) : kvc_launch<NP, 1, false, false, false>(a, st);
    return kn ? kvc_launch<NP, 1, false, true, true>(a, st) : kvc_launch<NP, 1, false, true, false>(a, st);
}

static bool kvc_misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

extern "C" int vq_kv_compress(void* qkv, long ld, const float* sr_w, const float* sr_b, const float* norm_w,
                              const float* norm_b, float norm_eps, const float* kn_w, const float* kn_b, float kn_eps,
                              const float* qn_w, const float* qn_b, float qn_eps, void* k_out, void* v_out, int B, int H, int W,
                              int C, int sr, int mode, void* stream) {
    if (!qkv || !k_out || !v_out) return VQ_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || sr <= 0 || ld <= 0) return VQ_EINVAL;
    if ((kn_w != nullptr) != (kn_b != nullptr) || (qn_w != nullptr) != (qn_b != nullptr)) return VQ_EINVAL;
    if (mode == VQ_KVC_CONV && (!sr_w || !sr_b || !norm_w || !norm_b)) return VQ_EINVAL;
    const long N = (long)H * W;
    if ((long)B * N > 0x7fffffffL / 2) return VQ_EINVAL;      // items (output tokens + q rows) are counted in an int
    if (C % 8 != 0 || ld % 8 != 0 || ld < 3L * C) return VQ_ESHAPE;
    if (mode == VQ_KVC_PICK_FLAT ? N % sr != 0 : (H % sr != 0 || W % sr != 0)) return VQ_ESHAPE;
    if (kvc_misaligned(qkv) || kvc_misaligned(k_out) || kvc_misaligned(v_out) || kvc_misaligned(sr_w) || kvc_misaligned(sr_b) ||
        kvc_misaligned(norm_w) || kvc_misaligned(norm_b) || kvc_misaligned(kn_w) || kvc_misaligned(kn_b) ||
        kvc_misaligned(qn_w) || kvc_misaligned(qn_b))
        return VQ_ESHAPE;
    if (mode != VQ_KVC_CONV && mode != VQ_KVC_PICK && mode != VQ_KVC_PICK_FLAT) return VQ_EUNSUP;
    if ((sr != 2 && sr != 4) || C > KVC_MAX_C) return VQ_EUNSUP;
    KvcArgs a{};
    a.qkv = (half_t*)qkv, a.ld = ld;
    a.sr_w = sr_w, a.sr_b = sr_b, a.n_w = norm_w, a.n_b = norm_b, a.kn_w = kn_w, a.kn_b = kn_b, a.qn_w = qn_w, a.qn_b = qn_b;
    a.n_eps = norm_eps, a.kn_eps = kn_eps, a.qn_eps = qn_eps;
    a.k_out = (half_t*)k_out, a.v_out = (half_t*)v_out;
    a.N = (int)N, a.W = W, a.C = C, a.sr = sr;
    a.Wo = mode == VQ_KVC_PICK_FLAT ? 1 : W / sr;
    a.Lk = mode == VQ_KVC_PICK_FLAT ? (int)(N / sr) : (H / sr) * (W / sr);
    a.n_kv = B * a.Lk, a.n_q = qn_w ? (int)(B * N) : 0;
    hipStream_t st = (hipStream_t)stream;
    const int np = (C / 8 + 63) / 64;
    switch (np) {
        case 1: return kvc_dispatch<1>(a, mode, st);
        case 2: return kvc_dispatch<2>(a, mode, st);
        case 3: return kvc_dispatch<3>(a, mode, st);
        default: return kvc_dispatch<4>(a, mode, st);
    }
}

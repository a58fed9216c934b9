// final_layer.hip - T2IFinalLayer in ONE launch for gfx950: LayerNorm (no affine) + AdaLN modulate + Linear C -> N_out
// (blocks.py:393-397 with the t2i_modulate expression x * (1 + scale) + shift), STDiT's and PixArt's last layer.
//   out[r, n] = fp16( sum_k xm[r, k] * w[n, k] + bias[n] ),  xm[r, k] = fp16( LN(x[r, :])[k] * (1 + scale[b, k]) + shift[b, k] ),
//   b = r / rows_per_sample.
// It replaces vq_ln_modulate_rowquant used for its fp16 by-product (which also computes and writes int8 codes and three row
// terms nobody reads, and writes xm) followed by vq_linear_f16 (which reads xm back): x is read once, [M, N_out] is
// written, and nothing else moves - no quantizer arithmetic, no codes, no xm store.
//
// Work split.  A WAVE owns whole 16-row token tiles.  Its lane (lq = lane & 15, g4 = lane >> 4) holds, of row lq of the
// tile, the 8 channels 32 s + 8 g4 .. + 8 of every k-step s - exactly the token fragment of v_mfma_f32_16x16x32_f16 (roles
// as in fp_linear.hip: A = weight fragment, B = token fragment, a lane of D^T owns one token and 4 consecutive output
// channels).  The tile's rows are loaded ONCE, as 16-byte loads (64 contiguous bytes per row and instruction, C / 32
// loads in flight per lane), and stay in registers as raw fp16 (C / 8 VGPRs: 144 at C = 1152) through the three passes:
// mean, centred sum of squares - a row's four partial sums sit in lanes lq, lq + 16, lq + 32, lq + 48 and meet through two
// xor exchanges - and modulate, whose fp16 result of k-step s is fed to the MFMAs of that step straight from the
// registers it was made in.  rstd = 1 / sqrt(var + eps) correctly rounded, (x - mu) * rstd, then * (1 + scale) + shift in
// fp32 and ONE rounding to fp16: the rounding points of rq_ln_stats / rq_modulate (rowquant_shared.h), which the
// two-launch route takes.  The sums run in another order than there, so xm may differ from that route's in a last bit.
//
// Modulation.  1 + scale and shift are read per tile and k-step by the lane that needs them, for the sample of ITS row
// (a tile may straddle samples when rows_per_sample % 16 != 0; every row takes its own sample's vectors): the 16 lanes of
// one g4 read the same 32 bytes when they share a sample and the four g4 one 128-byte line, so a load instruction is one
// line of a table (9 KB per sample at C = 1152) that stays in the CU's vector cache - once per tile, never once per row.
//
// Weight.  The WHOLE weight is resident in LDS per workgroup ([32, 1152] fp16: 72 KiB; nothing else is kept there),
// staged once by all four waves with 16-byte copies BEHIND the first tile's row loads, one barrier, none afterwards.  Rows
// are C + 8 halves apart: the pitch in 4-byte banks is C / 2 + 4 = 4 * odd (C % 32 == 0), so the 16 lanes of one g4 - one
// quarter of a ds_read_b128 - reading 16 weight rows at the same k start 4 * odd banks apart and cover the 64 banks
// exactly once: conflict-free by construction (not measured).  A weight that does not fit the 160 KiB of a CU beside
// nothing (N_out = 64 with C > 1272) is read as fragments from global memory instead (RES = false): it is 144 - 192 KiB
// and stays in L2.
//
// Grid.  tiles = ceil(M / 16); workgroups = max(min(tiles, CUs), min(ceil(tiles / 4), CUs * per_cu)), per_cu = 2 while two
// weights fit one CU's LDS, else 1; wave v of workgroup g takes tiles g + G (v + 4 i).  16384 rows: 256 workgroups, every
// wave of the chip's first row of workgroups one tile; 1024 rows: 64 workgroups on 64 CUs with one tile each (the other
// three waves only help stage the weight); beyond 2 * 4 * CUs tiles waves walk, and the weight stage is amortised.
// Rows past M of the last tile are loaded from row M - 1 (in bounds) and never stored.
//
// Refusals of vq_final_layer_f16, in this order, all before any HIP call or dereference:
//   1. VQ_EINVAL  x, shift, scale, w or out null (bias may be null)
//   2. VQ_EINVAL  M, rows_per_sample, C, N_out, ldx or ldw not positive
//   3. VQ_EINVAL  M % rows_per_sample != 0
//   4. VQ_ESHAPE  C % 32 != 0, C > 1536, N_out % 16 != 0, N_out > 64
//   5. VQ_ESHAPE  ldx % 8 != 0, ldw % 8 != 0, ldx < C, ldw < C
//   6. VQ_ESHAPE  x, shift, scale, w, out or a non-null bias not 16-byte aligned
#include "vq_common.h"

#define FL_WAVES 4
#define FL_THREADS (64 * FL_WAVES)
#define FL_MAX_C 1536
#define FL_MAX_N 64
#define FL_PAD 8                         // halves between weight rows in LDS
#define FL_LDS_CU (160 * 1024)
#define FL_G 2                           // k-steps per modulation request

struct FlArgs {
    const half_t* x;
    const float *shift, *scale;
    const half_t *w, *bias;
    half_t* out;
    long ldx, ldw;
    float eps;
    int M, rps, C, N, tiles;
};

__device__ __forceinline__ float fl_row_sum(float v) {      // over the four lanes lq + 16 j that share a row
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// The tile stays RAW fp16 between the passes: without this fence the compiler keeps the fp32 copies of one pass for the
// next (C / 4 more registers per lane, spilled to scratch at C = 1152); a conversion is one instruction, a register is not
template <int KS>
__device__ __forceinline__ void fl_pin(half8 (&h)[KS]) {
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(h[s]));
}

// KS: k-steps held (C <= 32 KS); NT: 16-column output tiles held (N_out <= 16 NT); RES: weight resident in LDS.
// Up to C = 1152 with N_out <= 32 two workgroups share a CU (72 KiB of LDS each): the register budget is held to that.
template <int KS, int NT, bool RES>
__global__ __launch_bounds__(FL_THREADS, (KS <= 36 && NT <= 2) ? 2 : 1) void final_layer_kernel(const FlArgs a) {
    extern __shared__ half_t fl_w[];                        // [N][C + FL_PAD] (RES)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 15, g4 = lane >> 4;
    const int C = a.C, ns = C >> 5, nt = a.N >> 4;
    const int ldl = C + FL_PAD;
    const int stride = gridDim.x * FL_WAVES;
    int tile = blockIdx.x + gridDim.x * wave;
    half8 h[KS];

    auto load_tile = [&](int t) {
        const long m = (long)t * 16 + lq;
        const half_t* xr = a.x + (size_t)(m < a.M ? m : a.M - 1) * a.ldx + 8 * g4;
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (s < ns) h[s] = *reinterpret_cast<const half8*>(xr + 32 * s);
    };
    if (tile < a.tiles) load_tile(tile);
    if constexpr (RES) {
        const int per_row = C >> 3;
        for (int i = threadIdx.x; i < a.N * per_row; i += FL_THREADS) {
            const int r = i / per_row, c = (i - r * per_row) * 8;
            *reinterpret_cast<half8*>(fl_w + r * ldl + c) = *reinterpret_cast<const half8*>(a.w + (size_t)r * a.ldw + c);
        }
        __syncthreads();
    }
    const float invC = 1.0f / (float)C;
    while (tile < a.tiles) {
        const long m = (long)tile * 16 + lq;
        const int b = (int)(m < a.M ? m : a.M - 1) / a.rps;
        // ---- LayerNorm statistics, two-pass
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (s < ns)
#pragma unroll
                for (int e = 0; e < 8; ++e) sum += (float)h[s][e];
        const float mu = fl_row_sum(sum) * invC;
        fl_pin<KS>(h);
        float sq = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (s < ns)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = (float)h[s][e] - mu;
                    sq += d * d;
                }
        const float var = fl_row_sum(sq) * invC;
        fl_pin<KS>(h);
        const float rstd = __fdiv_rn(1.0f, __fsqrt_rn(var + a.eps));
        // ---- modulate k-step s, feed it to the MFMAs of every output tile
        const float* scp = a.scale + (size_t)b * C + 8 * g4;
        const float* shp = a.shift + (size_t)b * C + 8 * g4;
        float4v acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = float4v{0.f, 0.f, 0.f, 0.f};
        // (two k-steps of modulation vectors are requested while the two before them are used: FL_G steps x 16 floats
        // x 2 buffers = 64 VGPRs beside the tile; the fences keep the scheduler from requesting the whole table at once)
        float md[2][FL_G][16];
        auto load_mod = [&](int g, float (&d)[FL_G][16]) {
#pragma unroll
            for (int u = 0; u < FL_G; ++u)
                if (g * FL_G + u < ns) {
                    const int k = 32 * (g * FL_G + u);
                    *reinterpret_cast<float4v*>(d[u]) = *reinterpret_cast<const float4v*>(scp + k);
                    *reinterpret_cast<float4v*>(d[u] + 4) = *reinterpret_cast<const float4v*>(scp + k + 4);
                    *reinterpret_cast<float4v*>(d[u] + 8) = *reinterpret_cast<const float4v*>(shp + k);
                    *reinterpret_cast<float4v*>(d[u] + 12) = *reinterpret_cast<const float4v*>(shp + k + 4);
                }
        };
        load_mod(0, md[0]);
#pragma unroll
        for (int g = 0; g < KS / FL_G; ++g) {
            if (g + 1 < KS / FL_G) load_mod(g + 1, md[(g + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < FL_G; ++u) {
                const int s = g * FL_G + u;
                if (s < ns) {
                    const float(&d)[16] = md[g & 1][u];
                    half8 xm;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float y = ((float)h[s][e] - mu) * rstd;
                        const float v = y * (1.0f + d[e]) + d[8 + e];
                        xm[e] = (half_t)v;
                    }
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t < nt) {
                            half8 wa;
                            if constexpr (RES) wa = *reinterpret_cast<const half8*>(fl_w + (16 * t + lq) * ldl + 32 * s + 8 * g4);
                            else wa = *reinterpret_cast<const half8*>(a.w + (size_t)(16 * t + lq) * a.ldw + 32 * s + 8 * g4);
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, xm, acc[t], 0, 0, 0);
                        }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- the next tile's rows are requested before this one's results leave
        const int next = tile + stride;
        if (next < a.tiles) load_tile(next);
        if (m < a.M) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t < nt) {
                    const int n = 16 * t + 4 * g4;
                    half4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (half_t)(acc[t][r] + (a.bias ? (float)a.bias[n + r] : 0.f));
                    *reinterpret_cast<half4*>(a.out + (size_t)m * a.N + n) = o;
                }
        }
        tile = next;
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <int KS, int NT, bool RES>
static int fl_launch(const FlArgs& a, hipStream_t st) {
    constexpr auto k = final_layer_kernel<KS, NT, RES>;
    const int lds = RES ? a.N * (a.C + FL_PAD) * (int)sizeof(half_t) : 0;
    int ncu = 0;
    const int e = vq_prepare_kernel<k>(RES ? FL_LDS_CU : 1024, &ncu);
    if (e != VQ_OK) return e;
    const int per_cu = 2 * lds <= FL_LDS_CU ? 2 : 1;
    const int spread = a.tiles < ncu ? a.tiles : ncu;
    const int quads = (a.tiles + FL_WAVES - 1) / FL_WAVES, cap = ncu * per_cu;
    const int walk = quads < cap ? quads : cap;
    hipLaunchKernelGGL(k, dim3((unsigned)(spread > walk ? spread : walk)), dim3(FL_THREADS), lds, st, a);
    return vq_check_launch();
}

template <int KS>
static int fl_dispatch(const FlArgs& a, hipStream_t st) {
    const bool res = a.N * (a.C + FL_PAD) * (int)sizeof(half_t) <= FL_LDS_CU;
    if constexpr (KS == 48) {
        if (!res) return fl_launch<KS, 4, false>(a, st);
    }
    return a.N <= 32 ? fl_launch<KS, 2, true>(a, st) : fl_launch<KS, 4, true>(a, st);
}

static bool fl_misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

extern "C" int vq_final_layer_f16(const void* x, const float* shift, const float* scale, float eps, const void* w,
                                  const void* bias, void* out, int M, int rows_per_sample, int C, int N_out, long ldx,
                                  long ldw, void* stream) {
    if (!x || !shift || !scale || !w || !out) return VQ_EINVAL;
    if (M <= 0 || rows_per_sample <= 0 || C <= 0 || N_out <= 0 || ldx <= 0 || ldw <= 0) return VQ_EINVAL;
    if (M % rows_per_sample != 0) return VQ_EINVAL;
    if (C % 32 != 0 || C > FL_MAX_C || N_out % 16 != 0 || N_out > FL_MAX_N) return VQ_ESHAPE;
    if (ldx % 8 != 0 || ldw % 8 != 0 || ldx < C || ldw < C) return VQ_ESHAPE;
    if (fl_misaligned(x) || fl_misaligned(shift) || fl_misaligned(scale) || fl_misaligned(w) || fl_misaligned(bias) ||
        fl_misaligned(out))
        return VQ_ESHAPE;
    FlArgs a{};
    a.x = (const half_t*)x, a.shift = shift, a.scale = scale, a.w = (const half_t*)w, a.bias = (const half_t*)bias;
    a.out = (half_t*)out, a.ldx = ldx, a.ldw = ldw, a.eps = eps;
    a.M = M, a.rps = rows_per_sample, a.C = C, a.N = N_out, a.tiles = (int)(((long)M + 15) / 16);
    hipStream_t st = (hipStream_t)stream;
    if (C <= 32 * 12) return fl_dispatch<12>(a, st);
    if (C <= 32 * 36) return fl_dispatch<36>(a, st);
    return fl_dispatch<48>(a, st);
}

// final_layer_i8.hip - T2IFinalLayer with a QUANTIZED Linear in ONE launch for gfx950: LayerNorm (no affine) + AdaLN
// modulate + the Linear's dynamic per-token quantizer + int8 MFMA Linear C -> N_out (PixArt's final_layer.linear, which the
// t2i FP list leaves quantized).  Per row r, sample b = r / rows_per_sample, token n = r % rows_per_sample:
//   xm[r, k] = fp16( LN(x[r, :])[k] * (1 + scale[b, k]) + shift[b, k] ),  q[r, k] = xm[r, k] / s[k]  (s: the Linear's
//   smoothing vector, may be absent), (delta, zp) of token n from the min / max of q over its channels AND its B samples
//   (the reference shares a token's grid over the batch), codes = clamp(rint(q / delta) + zp, 0, 2^n_bits - 1),
//   out[r, j] = fp16( sx sw_j (acc - zw_j R - zx cs_j) + bias_j ),  acc = sum_k int8 codes x int8 weight (ring_dequant).
// It replaces vq_ln_modulate_rowquant taken for its fp16 by-product xm (its codes and row terms are thrown away),
// vq_rowquant (reads xm back, writes codes and row terms) and vq_gemm_i8 with N = 32 on tiles built for N = 1152: the
// [M, C] activation crossed HBM four times for an [M, 32] result; here x is read once, [M, N_out] is written, and no
// codes, row terms or xm exist in memory.
//
// Work split.  A WORKGROUP of four waves owns one 16-row tile, arranged as 16 / B tokens x B samples: tile row lq = lane &
// 15 is token n0 + (lq % TPT) of sample lq / TPT, TPT = 16 / B - the samples of one token sit in lanes whose lq differ in
// the HIGH bits only, so the grid shared over the batch is a ladder of __shfl_xor over those bits (no LDS exchange), and
// every token's B rows are in one tile: a last tile is padded with whole tokens (loaded from row M - 1, never stored,
// their grids their own).  The 64-channel k-steps are dealt ROUND-ROBIN to the four waves (wave w: steps w, w + 4, ..., as
// fp_linear.hip deals its SPLITK steps): lane (lq, g4 = lane >> 4) holds per owned step the 16 channels 64 s + 16 g4 ..
// + 16 of row lq - the token fragment of v_mfma_i32_16x16x64_i8 (roles of gemm_wide.h: A = weight fragment, B = token
// fragment; a lane of D owns token lq and output channels 4 g4 .. + 4 of a 16-channel tile).  Two 16-byte loads per step,
// kept as raw fp16 (8 VGPRs per step; 5 steps at C = 1152, 6 at 1536) and overwritten in place by xm, which both later
// passes (min / max, encode) widen and divide again - no fp32 copy of a row lives across a barrier.  Occupancy, not a
// software pipeline, hides the load latency.
//
// Exchanges.  The row sum, the centred sum of squares and the row min / max each meet across the four waves through one
// 256-byte LDS table [wave][row]: a wave reduces its lanes' partials over g4 (two xor steps), lane g4 = 0 writes, one
// barrier, EVERY wave reads the four partials and combines them in wave order 0, 1, 2, 3 - identical mu, rstd, delta,
// zp in all four.  A table is rewritten one tile later, three barriers behind its last read.  Each wave then encodes its
// own channels (rq_quant on vq_row_grid's grid: the shared row steps, rowquant_shared.h) and runs its own MFMAs against
// the weight in LDS; waves 1 - 3 park their int32 accumulators and all four their code sums in LDS, one barrier, and wave
// 0 adds them - exact in integers, so the split changes no bit - dequantises and stores 8 bytes per lane and tile.
//
// Weight.  Staged once per workgroup into LDS as int8 rows of the ceil(C / 64) * 64 columns that are used, a nibble-packed
// weight (w_bits <= 4, [N, Kp / 2]) unpacked WHILE it is staged (the loop has one form), behind the first tile's row
// loads; the first barrier of the first tile publishes it.  Rows are Kp + 16 bytes apart: Kp % 128 == 0, so the pitch is
// 16 * odd bytes = 4 * odd banks, and the 16 lanes of one g4 - one quarter of a ds_read_b128 - reading 16 weight rows at the
// same k start 4 * odd banks apart and cover the 64 banks exactly once: conflict-free by construction (not measured).  The
// per-channel terms sw, P = sw (-zw), Q = sw cs, bias are parked beside it as ring_park_col_params parks them.
//
// Grid.  tiles = ceil(rows_per_sample / TPT); workgroups = min(tiles, CUs * resident), resident = workgroups whose LDS fits
// one CU, at most 3 (168 VGPRs); a workgroup walks tiles with stride gridDim.x.  A masked tail (C % 64 == 32: the lanes
// g4 >= 2 of the last step) feeds zero token bytes and enters no sum, min or max; columns [C, Kp) are never read.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), no scratch in either instantiation:
//   KSW 5 (C <= 1280): 155 VGPRs, 0 AGPRs, 106 SGPRs, scratch 0, 3 waves / SIMD; KSW 6: 165 VGPRs, 106 SGPRs, scratch 0, 3.
//   LDS: 2304 bytes of tables + N (Kp + 16) + 3 (N / 16) 1024 bytes: 45.8 KB at C 1152 -> 32 (three workgroups per CU,
//   the same three the registers allow; held to 128 VGPRs the compiler spills 20 - 36 of them), 113.9 KB at 1536 -> 64.
//
// Refusals of vq_final_layer_i8, in this order, all before any HIP call or dereference:
//   1. VQ_EINVAL  x, shift, scale, wq, sw, zw, cs or out null; s_rcp without s (s, s_rcp, bias, status may be null)
//   2. VQ_EINVAL  M, rows_per_sample, C, Kp, N_out or ldx not positive
//   3. VQ_EINVAL  M % rows_per_sample != 0
//   4. VQ_ESHAPE  C % 32 != 0, C > 1536, Kp != pad128(C), N_out % 16 != 0, N_out > 64, M / rows_per_sample not in
//                 {1, 2, 4, 8, 16}
//   5. VQ_ESHAPE  ldx % 8 != 0, ldx < C
//   6. VQ_EUNSUP  n_bits or w_bits outside 2 .. 8
//   7. VQ_ESHAPE  a non-null pointer not 16-byte aligned
#include "vq_common.h"
#include "rowquant_shared.h"
#include "gemm_common.h"

#define FQ_WAVES 4
#define FQ_THREADS (64 * FQ_WAVES)
#define FQ_MAX_C 1536
#define FQ_MAX_N 64
#define FQ_NT (FQ_MAX_N / 16)            // 16-channel output tiles a wave holds accumulators for
#define FQ_WPAD 16                       // bytes between weight rows in LDS beyond Kp
#define FQ_LDS_CU (160 * 1024)
#define FQ_MAX_RESIDENT 3

struct FqArgs {
    const half_t* x;
    const float *shift, *scale, *s, *s_rcp;
    const uint8_t* wq;
    const float* sw;
    const int32_t *zw, *cs;
    const float* bias;
    half_t* out;
    int32_t* status;
    long ldx;
    float eps;
    int M, rps, C, Kp, N, tiles, tpt, n_bits, w4;
};

__device__ __forceinline__ float fq_sum4(float v) {          // over the four lanes lq + 16 j that share a row
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// one cross-wave exchange of a per-row partial: lane g4 = 0 parks, the caller's barrier publishes, fq_meet combines the four
// partials in wave order (the same order in every wave)
template <class T>
__device__ __forceinline__ void fq_park(T (&tab)[FQ_WAVES][16], int wave, int lq, int g4, T v) {
    if (g4 == 0) tab[wave][lq] = v;
}
template <class T, class OP>
__device__ __forceinline__ T fq_meet(const T (&tab)[FQ_WAVES][16], int lq, OP op) {
    return op(op(op(tab[0][lq], tab[1][lq]), tab[2][lq]), tab[3][lq]);
}

// The row stays PACKED fp16 between the passes: without this fence the compiler keeps one pass's fp32 values for the next
// (16 more registers per step, spilled by a 128-register wave), as final_layer.hip's fl_pin explains
template <int KSW>
__device__ __forceinline__ void fq_pin(half8 (&h)[KSW][2]) {
#pragma unroll
    for (int j = 0; j < KSW; ++j) asm volatile("" : "+v"(h[j][0]), "+v"(h[j][1]));
}

// 8 channels of xm at column c0 as the quantizer's input: xm / s in the form vq_rowquant's smooth arm takes
__device__ __forceinline__ void fq_quotient(const half8& h, const float* s, const float* r, int c0, float (&q)[8]) {
    rq_widen(h, q);
    if (!s) return;                                          // (kernel-uniform)
    float sv[8];
    rq_load_f<8>(s + c0, sv);
    if (r) {
        float rv[8];
        rq_load_f<8>(r + c0, rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = rq_div_rcp(q[e], sv[e], rv[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = __fdiv_rn(q[e], sv[e]);
    }
}

// KSW: k-steps a wave holds (ceil(C / 64) <= 4 KSW)
template <int KSW>
__global__ __launch_bounds__(FQ_THREADS, FQ_MAX_RESIDENT) void final_layer_i8_kernel(const FqArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fq_lds[];   // weight [N][Kp + 16] | accumulators [3][nt][64] int4v
    __shared__ float t_sum[FQ_WAVES][16], t_sq[FQ_WAVES][16], t_mn[FQ_WAVES][16], t_mx[FQ_WAVES][16];
    __shared__ int t_cs[FQ_WAVES][16];
    __shared__ __attribute__((aligned(16))) float colp[4][FQ_MAX_N];   // sw | P = sw (-zw) | Q = sw cs | bias
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 15, g4 = lane >> 4;
    const int C = a.C, ns = (C + 63) >> 6, nt = a.N >> 4;
    const int pitch = a.Kp + FQ_WPAD;
    int4v* accx = reinterpret_cast<int4v*>(fq_lds + a.N * pitch);
    const int tok_l = lq & (a.tpt - 1), b = lq / a.tpt;      // this lane's token of the tile and its sample
    const RqWidth wd = rq_width(a.n_bits);
    half8 h[KSW][2];

    // chunk j of this wave: k-step wave + 4 j, columns c0 .. c0 + 16; live when inside the row
    auto col = [&](int j) { return 64 * (wave + FQ_WAVES * j) + 16 * g4; };
    auto load_tile = [&](int t) {
        const int tok = t * a.tpt + tok_l;
        const long m = tok < a.rps ? (long)b * a.rps + tok : (long)a.M - 1;
        const half_t* xr = a.x + (size_t)m * a.ldx;
#pragma unroll
        for (int j = 0; j < KSW; ++j)
            if (col(j) < C) {
                h[j][0] = *reinterpret_cast<const half8*>(xr + col(j));
                h[j][1] = *reinterpret_cast<const half8*>(xr + col(j) + 8);
            }
    };
    int tile = blockIdx.x;
    load_tile(tile);
    {   // the weight, once: 16 codes per thread and step - 16 bytes of an int8 image, 8 bytes of a nibble image
        const int per_row = ns * 4;
        for (int i = threadIdx.x; i < a.N * per_row; i += FQ_THREADS) {
            const int r = i / per_row, c = i - r * per_row;
            int4v v;
            if (a.w4) {
                const int2v p = *reinterpret_cast<const int2v*>(a.wq + (size_t)r * (a.Kp >> 1) + 8 * c);
                v = int4v{p[0] & 0x0F0F0F0F, (int)(((uint32_t)p[0] >> 4) & 0x0F0F0F0Fu), p[1] & 0x0F0F0F0F,
                          (int)(((uint32_t)p[1] >> 4) & 0x0F0F0F0Fu)};
            } else {
                v = *reinterpret_cast<const int4v*>(a.wq + (size_t)r * a.Kp + 16 * c);
            }
            *reinterpret_cast<int4v*>(fq_lds + r * pitch + 16 * c) = v;
        }
        if (threadIdx.x < a.N) {
            const int n = threadIdx.x;
            const float sw = a.sw[n];
            colp[0][n] = sw;
            colp[1][n] = sw * (float)(-a.zw[n]);
            colp[2][n] = sw * (float)a.cs[n];
            colp[3][n] = a.bias ? a.bias[n] : 0.f;
        }
    }
    const float invC = 1.0f / (float)C;
    const float* scp0 = a.scale + (size_t)b * C;
    const float* shp0 = a.shift + (size_t)b * C;
    for (; tile < a.tiles; tile += gridDim.x) {
        const int tok = tile * a.tpt + tok_l;
        const bool live = tok < a.rps;
        // A lane meets the same sample and columns in every tile, so its modulation and smoothing vectors are loop
        // invariants the compiler would hoist and hold (up to 64 floats per k-step, spilled): the addresses are made new
        // values per tile, the vectors are re-read chunk by chunk from the CU's cache
        const float *scp = scp0, *shp = shp0, *sp = a.s, *rp = a.s_rcp;
        asm volatile("" : "+v"(scp), "+v"(shp), "+s"(sp), "+s"(rp));
        // ---- LayerNorm statistics, two-pass, the rounding points of rq_ln_stats (wave map)
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < KSW; ++j)
            if (col(j) < C)
#pragma unroll
                for (int e = 0; e < 16; ++e) sum += (float)h[j][e >> 3][e & 7];
        fq_park(t_sum, wave, lq, g4, fq_sum4(sum));
        fq_pin<KSW>(h);
        __syncthreads();
        const float mu = fq_meet(t_sum, lq, vq_addf) * invC;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < KSW; ++j)
            if (col(j) < C)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float d = (float)h[j][e >> 3][e & 7] - mu;
                    sq += d * d;
                }
        fq_park(t_sq, wave, lq, g4, fq_sum4(sq));
        fq_pin<KSW>(h);
        __syncthreads();
        const float var = fq_meet(t_sq, lq, vq_addf) * invC;
        const float rstd = __fdiv_rn(1.0f, __fsqrt_rn(var + a.eps));
        // ---- modulate (rq_modulate: one rounding to fp16), xm replaces x in its registers; min / max of xm / s
        float vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < KSW; ++j)
            if (col(j) < C) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {                // the chunk's two 16-byte halves
                    const int c0 = col(j) + 8 * u;
                    float v[8], sc1[8], sh[8], q[8];
                    rq_widen(h[j][u], v);
                    rq_load_mod<8>(scp + c0, shp + c0, sc1, sh);
                    h[j][u] = rq_modulate<8>(v, mu, rstd, sc1, sh, false, nullptr, 0);
                    fq_quotient(h[j][u], sp, rp, c0, q);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        vmin = fminf(vmin, q[e]);
                        vmax = fmaxf(vmax, q[e]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);           // one chunk's vectors in flight, not the whole table's
            }
        fq_pin<KSW>(h);
        vmin = fminf(vmin, __shfl_xor(vmin, 16, 64));
        vmin = fminf(vmin, __shfl_xor(vmin, 32, 64));
        vmax = fmaxf(vmax, __shfl_xor(vmax, 16, 64));
        vmax = fmaxf(vmax, __shfl_xor(vmax, 32, 64));
        fq_park(t_mn, wave, lq, g4, vmin);
        fq_park(t_mx, wave, lq, g4, vmax);
        __syncthreads();
        float mn = fq_meet(t_mn, lq, [](float p, float q) { return fminf(p, q); });
        float mx = fq_meet(t_mx, lq, [](float p, float q) { return fmaxf(p, q); });
        for (int o = a.tpt; o < 16; o <<= 1) {              // the token's B samples: the high bits of lq
            mn = fminf(mn, __shfl_xor(mn, o, 64));
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        }
        float delta, zp, inv;
        bool small;
        vq_row_grid(mn, mx, wd.qmax, delta, zp, small, inv);
        if (small && live && wave == 0 && lane == tok_l && a.status) atomicOr(a.status, VQ_ST_EPSFILL);   // once per token
        // ---- encode this wave's channels, multiply them with the weight
        int4v acc[FQ_NT];
#pragma unroll
        for (int t = 0; t < FQ_NT; ++t) acc[t] = int4v{0, 0, 0, 0};
        uint32_t csum = 0;
#pragma unroll
        for (int j = 0; j < KSW; ++j) {
            const int s = wave + FQ_WAVES * j;               // (wave-uniform)
            if (s < ns) {
                uint32_t pk[4] = {0u, 0u, 0u, 0u};           // a masked chunk of the tail step: zero token bytes
                if (col(j) < C) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        float q[8];
                        uint32_t p2[2];
                        fq_quotient(h[j][u], sp, rp, col(j) + 8 * u, q);
                        RQ_BY_WIDTH(wd.qmax, rq_quant<8, SAT8_>(q, inv, delta, zp, wd.qmax, p2);)
                        pk[2 * u] = p2[0], pk[2 * u + 1] = p2[1];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        csum = __builtin_amdgcn_sad_u8(pk[k], 0u, csum);
                        pk[k] ^= wd.flip;
                    }
                }
                const int4v xb = int4v{(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
                const uint8_t* wl = fq_lds + lq * pitch + 64 * s + 16 * g4;
#pragma unroll
                for (int t = 0; t < FQ_NT; ++t)
                    if (t < nt) {
                        const int4v wa = *reinterpret_cast<const int4v*>(wl + 16 * t * pitch);
                        acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa, xb, acc[t], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- the four partial accumulators and code sums meet in wave 0
        int cs_row = (int)csum;
        cs_row += __shfl_xor(cs_row, 16, 64);
        cs_row += __shfl_xor(cs_row, 32, 64);
        fq_park(t_cs, wave, lq, g4, cs_row);
        if (wave > 0) {
#pragma unroll
            for (int t = 0; t < FQ_NT; ++t)
                if (t < nt) accx[((wave - 1) * nt + t) * 64 + lane] = acc[t];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < FQ_NT; ++t)
                if (t < nt)
#pragma unroll
                    for (int w = 0; w < FQ_WAVES - 1; ++w) acc[t] += accx[(w * nt + t) * 64 + lane];
            // the row terms as rq_write_row forms them (QAct: sx, zx, R), never written
            const int code_sum = fq_meet(t_cs, lq, vq_addi);
            const int izx = (int)zp - wd.cx;
            const int R = code_sum - wd.cx * C - C * izx;
            const float sx = delta, V = sx * (float)(-izx), U = sx * (float)R;
            if (live) {
                half_t* orow = a.out + ((size_t)b * a.rps + tok) * a.N + 4 * g4;
#pragma unroll
                for (int t = 0; t < FQ_NT; ++t)
                    if (t < nt) {
                        const int n = 16 * t + 4 * g4;
                        const float4v fsw = *reinterpret_cast<const float4v*>(colp[0] + n);
                        const float4v fP = *reinterpret_cast<const float4v*>(colp[1] + n);
                        const float4v fQ = *reinterpret_cast<const float4v*>(colp[2] + n);
                        const float4v fb = *reinterpret_cast<const float4v*>(colp[3] + n);
                        half4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            o[e] = (half_t)ring_dequant(acc[t][e], sx, V, U, fsw[e], fP[e], fQ[e], fb[e]);
                        *reinterpret_cast<half4*>(orow + 16 * t) = o;
                    }
            }
        }
        if (tile + (int)gridDim.x < a.tiles) load_tile(tile + gridDim.x);
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
static int fq_lds_bytes(int N, int Kp) { return N * (Kp + FQ_WPAD) + (FQ_WAVES - 1) * (N / 16) * 64 * (int)sizeof(int4v); }

template <int KSW>
static int fq_launch(const FqArgs& a, hipStream_t st) {
    constexpr auto k = final_layer_i8_kernel<KSW>;
    const int lds = fq_lds_bytes(a.N, a.Kp);
    int ncu = 0;
    const int e = vq_prepare_kernel<k>(FQ_LDS_CU - 4096, &ncu);   // (the static tables take 2.3 KiB of the CU's 160)
    if (e != VQ_OK) return e;
    int resident = (FQ_LDS_CU - 4096) / (lds + 2560);
    resident = resident < 1 ? 1 : (resident > FQ_MAX_RESIDENT ? FQ_MAX_RESIDENT : resident);
    const long cap = (long)ncu * resident;
    hipLaunchKernelGGL(k, dim3((unsigned)(a.tiles < cap ? a.tiles : cap)), dim3(FQ_THREADS), lds, st, a);
    return vq_check_launch();
}

static int fq_pad128(int k) { return (k + 127) / 128 * 128; }

extern "C" int vq_final_layer_i8(const void* x, const float* shift, const float* scale, float eps, const float* s,
                                 const float* s_rcp, const void* wq, const float* sw, const int* zw, const int* cs,
                                 const float* bias, void* out, int* status, int M, int rows_per_sample, int C, int Kp,
                                 int N_out, long ldx, int n_bits, int w_bits, void* stream) {
    if (!x || !shift || !scale || !wq || !sw || !zw || !cs || !out || (s_rcp && !s)) return VQ_EINVAL;
    if (M <= 0 || rows_per_sample <= 0 || C <= 0 || Kp <= 0 || N_out <= 0 || ldx <= 0) return VQ_EINVAL;
    if (M % rows_per_sample != 0) return VQ_EINVAL;
    const int B = M / rows_per_sample;
    if (C % 32 != 0 || C > FQ_MAX_C || Kp != fq_pad128(C) || N_out % 16 != 0 || N_out > FQ_MAX_N) return VQ_ESHAPE;
    if (B > 16 || (B & (B - 1)) != 0) return VQ_ESHAPE;
    if (ldx % 8 != 0 || ldx < C) return VQ_ESHAPE;
    if (n_bits < 2 || n_bits > 8 || w_bits < 2 || w_bits > 8) return VQ_EUNSUP;
    if (rq_off16(x) || rq_off16(shift) || rq_off16(scale) || rq_off16(s) || rq_off16(s_rcp) || rq_off16(wq) || rq_off16(sw) ||
        rq_off16(zw) || rq_off16(cs) || rq_off16(bias) || rq_off16(out) || rq_off16(status))
        return VQ_ESHAPE;
    FqArgs a{};
    a.x = (const half_t*)x, a.shift = shift, a.scale = scale, a.s = s, a.s_rcp = s_rcp, a.wq = (const uint8_t*)wq;
    a.sw = sw, a.zw = zw, a.cs = cs, a.bias = bias, a.out = (half_t*)out, a.status = status, a.ldx = ldx, a.eps = eps;
    a.M = M, a.rps = rows_per_sample, a.C = C, a.Kp = Kp, a.N = N_out, a.tpt = 16 / B;
    a.tiles = (rows_per_sample + a.tpt - 1) / a.tpt, a.n_bits = n_bits, a.w4 = w_bits <= 4;
    hipStream_t st = (hipStream_t)stream;
    if (C <= 64 * FQ_WAVES * 5) return fq_launch<5>(a, st);
    return fq_launch<6>(a, st);
}

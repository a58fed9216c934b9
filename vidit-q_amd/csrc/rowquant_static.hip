// rowquant_static.hip - one-pass activation quantizers on STATIC (calibrated) grids for gfx950.
//
// Replaces: ActQuantizer.forward after init_done (qdiff/quantizer/base_quantizer.py:129-144) for up to three Linears
// that share an input, with what precedes them in a block - nn.LayerNorm + t2i_modulate (opensora/models/stdit/stdit.py:
// 103,124; layers/blocks.py:51), the temporal position embedding (stdit.py:112-114) and the smooth-quant division
// (qdiff/models/quant_layer.py:140) - in the same pass.
//
// A static grid needs no min / max, no exchange between the rows of a batch and no eps-fill status: a row is read
// once, (LayerNorm: normalised once,) and quantized n_out times on the grids (delta_j, zp_j), which are DEVICE arrays of
// 1 or n_tok entries read by the kernel.  Codes, steps, zero points and row terms are laid out as vq_rowquant writes
// them and are bit-identical to rowquant_kernel's static case (vq_code with the grid from delta_in / zp_in).
//
// Lane -> column maps.  The LayerNorm arm must reproduce the fp16 activation vq_ln_modulate_rowquant(n_out = 1,
// s = NULL, xm_out) stores today, bit for bit, so it keeps the summation order of the kernel that call runs:
//   one row per wave (lane * 8 + i * 512: ln_modulate_rowquant_fast_kernel and the generic kernel; B != 2, or a width
//   outside the block widths), or one row per half-wave (hl * 4 + i * 128: ln_modulate_rowquant_half_kernel<PAIR>;
//   B == 2 at a block width).  The two orders give different sums, hence both layouts exist here.
// The plain and added-rows arms take the half-wave layout at the block widths (every lane busy at C = 1152, as
// rowquant_half_kernel), rows of 4608 channels split over two partner waves (as rowquant_split_kernel) and one row per
// wave elsewhere; that last form is the chunk loop for every other C % 8 == 0 with Kp <= 4608 (1, 3 or 9 chunks).
// The maps fix the access width: 16-byte loads in the wave layouts, 8-byte loads in the half-wave layout, 8- and
// 4-byte code stores (a lane owns 8 or 4 consecutive codes), every access of a wave contiguous.
//
// round(x / delta) on a grid the row did not define: rqs_grid / rqs_quant of rowquant_shared.h (the product form with a
// window and a guard per (row, output); derivation there).  tests/test_static_quant_gpu.py runs exact ties, both clamps,
// values 300 steps outside and +-65504 through every layout.
#include "vq_common.h"
#include "rowquant_shared.h"

#define RQS_WAVES 4
#define RQS_THREADS (RQS_WAVES * 64)
#define RQS_MAX_KP 4608

enum { RQS_PLAIN = 0, RQS_ADD = 1, RQS_LN = 2 };

struct RqsArgs {
    const half_t* x;
    const half_t* add_rows;
    int add_div;
    const float* shift;
    const float* scale;
    float ln_eps;
    const float* s[3];       // smoothing vector of output j, or null
    const float* r[3];       // RN(1 / s) per channel, or null: IEEE division
    const float* delta[3];   // n_param entries
    const float* zp[3];
    int8_t* xq[3];
    float* sx[3];
    int32_t* zx[3];
    int32_t* R[3];
    half_t* xm;
    int n_param, rows, n_tok, C, Kp, n_bits;
};

// ---------------------------------------------------------------------------
// L: RqHalf<NIT> / RqWave<MAXCH>.  ARM: plain / + add_rows[(r % n_tok) / add_div] / LayerNorm + modulate.
// SPLIT (RqWave only, Kp == C, C % 16 == 0): waves 2k / 2k + 1 take the two halves of a row and add their code sums
// through LDS.  Dynamic LDS: [NOUT][s | 1/s][C] floats when any output is smoothed (staged once per workgroup).
// At most 128 VGPRs (4 waves per SIMD asked of the compiler) wherever the row fits: every wave of a 16384-row launch
// is resident at once; the LayerNorm arm of rows longer than 1536 channels holds 72 fp32 values per lane and is not bound.
// ---------------------------------------------------------------------------
template <class L, int ARM, int NOUT, bool SPLIT>
__global__ __launch_bounds__(RQS_THREADS, (ARM == RQS_LN && L::NCH * L::W > 40) ? 1 : 4) void rowquant_static_kernel(RqsArgs a) {
    static_assert(!SPLIT || (!L::HALF && ARM != RQS_LN), "split rows: one-row-per-wave map, no row statistics");
    constexpr int NCH = L::NCH, W = L::W;
    typedef typename L::hvec hvec;
    extern __shared__ __attribute__((aligned(16))) float rqs_lds[];
    __shared__ int ps[SPLIT ? NOUT : 1][RQS_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool hi = L::HALF && lane >= 32;
    const int C = a.C;
    bool any_s = false;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) any_s = any_s || a.s[j];
    if (any_s) {                                          // kernel-uniform
        for (int i = threadIdx.x; i < C / 4; i += RQS_THREADS) {
#pragma unroll
            for (int j = 0; j < NOUT; ++j) {
                if (a.s[j]) reinterpret_cast<float4v*>(rqs_lds + (2 * j) * C)[i] = reinterpret_cast<const float4v*>(a.s[j])[i];
                if (a.r[j]) reinterpret_cast<float4v*>(rqs_lds + (2 * j + 1) * C)[i] = reinterpret_cast<const float4v*>(a.r[j])[i];
            }
        }
        __syncthreads();
    }
    int row = L::HALF ? (blockIdx.x * RQS_WAVES + wv) * 2 + (hi ? 1 : 0)
                      : SPLIT ? blockIdx.x * (RQS_WAVES / 2) + (wv >> 1) : blockIdx.x * RQS_WAVES + wv;
    const bool live = row < a.rows;
    if (!live) {
        if constexpr (!L::HALF && !SPLIT) return;         // (no barrier below)
        row = a.rows - 1;                                 // re-does the last row, writes nothing
    }
    const int seg = SPLIT ? C / 2 : C;                    // this wave's channels [col0, col0 + seg), padded to segp
    const int segp = SPLIT ? C / 2 : a.Kp;
    const int col0 = (SPLIT && (wv & 1)) ? C / 2 : 0;
    const int lc = L::lane_col(lane);                     // + i * STEP: the lane's i-th chunk inside the segment
    const RqWidth wd = rq_width(a.n_bits);
    const float qmax = wd.qmax;
    const int tok = row % a.n_tok;
    const half_t* xrow = a.x + (size_t)row * C + col0;

    hvec h[NCH];
    rq_load_row<L>(xrow, lc, seg, h);

    RqsGrid g[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) g[j] = rqs_grid(a.delta[j], a.zp[j], a.n_param == 1 ? 0 : tok, qmax);

    // LayerNorm statistics in the order of the kernel whose xm this arm reproduces (file comment)
    float v[ARM == RQS_LN ? NCH : 1][W];
    float mu = 0.f, rstd = 0.f;
    const float *shp = nullptr, *scp = nullptr;
    if constexpr (ARM == RQS_LN) {
        rq_widen_row<L>(h, lc, C, v);
        rq_ln_stats<L>(v, lc, C, a.ln_eps, hi, mu, rstd);
        const size_t bo = (size_t)(row / a.n_tok) * C;    // modulation vectors of the row's sample
        shp = a.shift + bo;
        scp = a.scale + bo;
    }
    const half_t* addp = ARM == RQS_ADD ? a.add_rows + (size_t)(tok / a.add_div) * C + col0 : nullptr;

    uint32_t csum[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) csum[j] = 0;
    // one kernel-uniform branch on the code width around the whole loop (as RQ_BY_WIDTH)
    auto chunks = [&](auto sat8) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        constexpr bool SAT8_ = decltype(sat8)::value;
        const int c = lc + i * L::STEP;
        if (L::HALF || c < seg) {
            float u[W];
            if constexpr (ARM == RQS_LN) {
                float sc1[W], sh[W];
                rq_load_mod<W>(scp + c, shp + c, sc1, sh);
                const hvec hm = rq_modulate<W>(v[i], mu, rstd, sc1, sh, a.xm && live, a.xm, (size_t)row * C + c);
                rq_widen(hm, u);                           // the grid quantizes the STORED fp16 activation
            } else {
                rq_widen(h[i], u);
                if constexpr (ARM == RQS_ADD) {
                    const hvec ad = *reinterpret_cast<const hvec*>(addp + c);
#pragma unroll
                    for (int e = 0; e < W; ++e) u[e] += (float)ad[e];
                }
            }
#pragma unroll
            for (int j = 0; j < NOUT; ++j) {
                float w[W];
                if (a.s[j]) {                              // kernel-uniform
                    const float* ls = rqs_lds + (2 * j) * C + col0 + c;
                    float sv[W];
                    rq_load_f<W>(ls, sv);
                    if (a.r[j]) {
                        float rv[W];
                        rq_load_f<W>(ls + C, rv);
#pragma unroll
                        for (int e = 0; e < W; ++e) w[e] = rq_div_rcp(u[e], sv[e], rv[e]);
                    } else {
#pragma unroll
                        for (int e = 0; e < W; ++e) w[e] = __fdiv_rn(u[e], sv[e]);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < W; ++e) w[e] = u[e];
                }
                uint32_t pk[W / 4];
                rqs_quant<W, SAT8_>(w, g[j], qmax, pk);
#pragma unroll
                for (int k = 0; k < W / 4; ++k) {
                    csum[j] = __builtin_amdgcn_sad_u8(pk[k], 0u, csum[j]);
                    pk[k] ^= wd.flip;
                }
                if (live) rq_store_codes<W>(a.xq[j] + (size_t)row * a.Kp + col0 + c, pk);
            }
        } else if (c < segp) {                             // pad columns [C, Kp)
            const uint32_t zero[W / 4] = {};
#pragma unroll
            for (int j = 0; j < NOUT; ++j)
                if (live) rq_store_codes<W>(a.xq[j] + (size_t)row * a.Kp + col0 + c, zero);
        }
      }
    };
    if (qmax == 255.0f) chunks(std::true_type{});
    else chunks(std::false_type{});
    int rs[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        rs[j] = rq_sum_i<L::HALF>((int)csum[j], hi);
        if constexpr (SPLIT)
            if (lane == 0) ps[j][wv] = rs[j];
    }
    if constexpr (SPLIT) __syncthreads();
    const bool writer = (L::HALF ? (lane & 31) == 0 : lane == 0) && live && !(SPLIT && (wv & 1));
    if (writer) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            int sum = rs[j];
            if constexpr (SPLIT) sum += ps[j][wv ^ 1];
            rq_write_row(a.sx[j], a.zx[j], a.R[j], nullptr, row, g[j].delta, g[j].zp, sum, C, wd.cx);
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <class L, int ARM, bool SPLIT>
static int rqs_launch(const RqsArgs& a, int n_out, hipStream_t st) {
    int lds = 0;
    for (int j = 0; j < n_out; ++j)
        if (a.s[j]) lds = 2 * n_out * a.C * (int)sizeof(float);
    const int per = SPLIT ? RQS_WAVES / 2 : (L::HALF ? 2 : 1) * RQS_WAVES;   // rows per workgroup
    const dim3 grid((a.rows + per - 1) / per), block(RQS_THREADS);
    auto go = [&](auto nout) -> int {
        constexpr auto k = rowquant_static_kernel<L, ARM, nout(), SPLIT>;
        if (lds > 48 * 1024) {                             // three smoothed outputs of rows beyond 2048 channels
            const int e = vq_prepare_kernel<k>(2 * 3 * RQS_MAX_KP * (int)sizeof(float));
            if (e != VQ_OK) return e;
        }
        hipLaunchKernelGGL(k, grid, block, lds, st, a);
        return vq_check_launch();
    };
    if (n_out == 1) return go(std::integral_constant<int, 1>{});
    if (n_out == 2) return go(std::integral_constant<int, 2>{});
    return go(std::integral_constant<int, 3>{});
}

template <int ARM>
static int rqs_dispatch(const RqsArgs& a, int n_out, int B, hipStream_t st) {
    const bool block_w = rq_block_width(a.C) && a.Kp == a.C && a.rows >= 2;
    // LayerNorm: the layout whose summation order today's xm has (file comment); other arms: every lane busy
    const bool half_wave = block_w && (ARM != RQS_LN || B == 2);
    int rc = VQ_OK;
    if (half_wave) {
        vq_dispatch_nit(a.C, [&](auto nit) { rc = rqs_launch<RqHalf<nit()>, ARM, false>(a, n_out, st); });
        return rc;
    }
    if constexpr (ARM == RQS_PLAIN)
        if (a.C == RQS_MAX_KP && a.Kp == a.C && a.rows >= 2) return rqs_launch<RqWave<5>, ARM, true>(a, n_out, st);
    vq_dispatch_maxch(a.Kp, [&](auto m) { rc = rqs_launch<RqWave<m()>, ARM, false>(a, n_out, st); });
    return rc;
}

static bool rqs_misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

extern "C" int vq_rowquant_static(const void* x, const void* add_rows, int n_add, int add_div, const float* shift,
                                  const float* scale, float ln_eps, int n_out, const float* const* s,
                                  const float* const* s_rcp, const float* const* delta, const float* const* zp, int n_param,
                                  int8_t* const* xq, float* const* sx, int32_t* const* zx, int32_t* const* R, void* xm_out,
                                  int B, int n_tok, int C, int Kp, int n_bits, void* stream) {
    if (!x || !delta || !zp || !xq || !sx || !zx || !R) return VQ_EINVAL;
    if ((shift != nullptr) != (scale != nullptr)) return VQ_EINVAL;
    if (n_out < 1 || n_out > 3 || B <= 0 || n_tok <= 0 || C <= 0 || Kp <= 0) return VQ_EINVAL;
    if (n_param != 1 && n_param != n_tok) return VQ_EINVAL;
    if (add_rows && (add_div <= 0 || n_add <= 0 || (n_tok + add_div - 1) / add_div > n_add)) return VQ_EINVAL;
    if ((long)B * n_tok > 0x7fffffffL) return VQ_EINVAL;
    if (C % 8 != 0 || Kp % 128 != 0 || Kp < C) return VQ_ESHAPE;
    if (add_rows && shift) return VQ_EUNSUP;
    if (n_bits < 2 || n_bits > 8 || Kp > RQS_MAX_KP) return VQ_EUNSUP;
    if (xm_out && !shift) return VQ_EINVAL;                // the modulated activation exists behind LayerNorm only
    if (rqs_misaligned(x) || rqs_misaligned(add_rows) || rqs_misaligned(shift) || rqs_misaligned(scale) || rqs_misaligned(xm_out))
        return VQ_ESHAPE;
    RqsArgs a{};
    a.x = (const half_t*)x, a.add_rows = (const half_t*)add_rows, a.add_div = add_div > 0 ? add_div : 1;
    a.shift = shift, a.scale = scale, a.ln_eps = ln_eps, a.xm = (half_t*)xm_out;
    a.n_param = n_param, a.rows = B * n_tok, a.n_tok = n_tok, a.C = C, a.Kp = Kp, a.n_bits = n_bits;
    for (int j = 0; j < n_out; ++j) {                      // (host arrays of device pointers: nothing on the device is read)
        a.s[j] = s ? s[j] : nullptr;
        a.r[j] = (a.s[j] && s_rcp) ? s_rcp[j] : nullptr;
        a.delta[j] = delta[j], a.zp[j] = zp[j];
        a.xq[j] = xq[j], a.sx[j] = sx[j], a.zx[j] = zx[j], a.R[j] = R[j];
        if (!a.delta[j] || !a.zp[j] || !a.xq[j] || !a.sx[j] || !a.zx[j] || !a.R[j]) return VQ_EINVAL;
        if (rqs_misaligned(a.s[j]) || rqs_misaligned(a.r[j]) || rqs_misaligned(a.xq[j])) return VQ_ESHAPE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (shift) return rqs_dispatch<RQS_LN>(a, n_out, B, st);
    if (add_rows) return rqs_dispatch<RQS_ADD>(a, n_out, B, st);
    return rqs_dispatch<RQS_PLAIN>(a, n_out, B, st);
}

// vq_rowquant's static case (delta_in given) at a shape this file covers; false: the caller runs rowquant_kernel
bool vq_rowquant_static_one(const half_t* x, const half_t* add_rows, int n_add, int add_div, const float* s, const float* s_rcp,
                            int8_t* xq, float* sx, int32_t* zx, int32_t* R, const float* delta, const float* zp, int n_param,
                            int B, int n_tok, int C, int Kp, int n_bits, hipStream_t st, int* rc) {
    if (Kp > RQS_MAX_KP || (long)B * n_tok > 0x7fffffffL) return false;
    if (rqs_misaligned(x) || rqs_misaligned(add_rows) || rqs_misaligned(s) || rqs_misaligned(s_rcp) || rqs_misaligned(xq)) return false;
    *rc = vq_rowquant_static(x, add_rows, n_add, add_div, nullptr, nullptr, 0.f, 1, &s, &s_rcp, &delta, &zp, n_param, &xq, &sx,
                             &zx, &R, nullptr, B, n_tok, C, Kp, n_bits, st);
    return true;
}

// gemm_i8.hip - W8A8 / W4A8 Linear for gfx950: int8 MFMA contraction + fused dequant epilogue (product kernels only;
// the retired generations and ablations are tools/lab/gemm_lab.hip).
//
// Replaces F.linear(x_hat, W_hat, bias) on fake-quantized operands
// (qdiff/models/quant_layer.py:211; stdit_quant_layer.py:96,187,304; dit_quant_layer.py:29,76)
// with the equivalent integer form:
//   out[m,n] = sx[m]*sw[n] * (acc - zw[n]*R[m] - zx[m]*cs[n]) + bias[n],  acc = sum_k xs*ws  (int32)
// and, by epilogue, GELU-tanh (modules.py:57) and the gate/residual adds (stdit.py:109,118,121,128).
//
// Design (MI355X): one 512-thread workgroup (8 wave64) per BM x BN output tile, 1 workgroup / CU (gemm_wide.h).
//   - tile 256 tokens x 288 channels: 1152 = 4*288, 3456 = 12*288, 4608 = 16*288, so with
//     M = 16384 every Linear of the STDiT block is an exact multiple of 256 workgroups (no tail wave);
//     intensity 256*288/(256+288) = 135 MAC/B of L2->LDS traffic.
//   - operands are both K-contiguous ([M,Kp] and [N,Kp] int8), staged L2 -> LDS by LDS-DMA (buffer_load ... lds) in
//     whole 128-byte lines per row and stage, double-buffered, one barrier per stage; LDS rows XOR-swizzled at
//     16-byte granularity so every ds_read_b128 fragment read is conflict-free.
//   - MFMA v_mfma_i32_16x16x64_i8 with the WEIGHT fragment as the A operand and the TOKEN fragment as
//     the B operand, i.e. each wave computes D^T[n][m]: a lane then owns ONE token (column) and four
//     consecutive channels per accumulator quad -> per-token dequant terms are lane constants.
//   - blockIdx -> tile map is XCD-aware (8 XCDs, private L2s; xcd_tile in gemm_common.h).
//   - W4A8: nibble-packed weights travel as nibbles through LDS and are expanded to int8 operand words in registers
//     (layout in pack.hip).
//   - Launches whose 128-row tiles all fit ONE round of the 256 CUs (PixArt-Sigma's N = 1152 Linears at M = 8192: 128
//     tiles of 256 rows = half the chip idle; the batched prompt K/V of 120-300 rows) take the 128 x 288 form of the same
//     kernel (32 x 144 wave tiles): twice the workgroups, half the k-loop work each.  Same arithmetic per output
//     element, bit-identical results (tested).
//
// Roofline: MFMA-bound (int8 dense peak 5.03 POPS); algorithmic bytes M*K + N*K(/2) + 2*M*N (+2*M*N
// when a residual is read).
#include "gemm_wide.h"

// Tile height by shape.  A 128-row tile costs ~0.62 of a 256-row one (tools/gemm_half_tiles.py: 17.2 vs 23.1 us at
// K = 1152, 45.1 vs 60.2 us at K = 4608 for one round), so it wins when it brings idle CUs in - fewer than 5/8 as many
// rounds of the 256 CUs per 256-row round: every launch whose 128-row tiles fit ONE round (M = 8192, N = 1152: 128
// -> 256 workgroups), and 1.5-round launches such as N = 3456 at M = 8192 (384 -> 768 tiles: 45.3 vs 48.2 us).
static bool vq_half_tiles(int M, int N, int sets) {
    const long nt = (long)((N + 287) / 288) * sets;
    const long r128 = (((M + 127) / 128) * nt + 255) / 256, r256 = (((M + 255) / 256) * nt + 255) / 256;
    return r128 * 5 < r256 * 8;
}
// Launches made of interior tiles only (M % tile height == 0, N % 288 == 0) take the scalar-addressed form of the same
// kernel with asymmetric DMA issue (gemm_wide.h, INT 1: waves 0-3 issue every stage piece): `variant` 19, and the library's
// own choice for such shapes - every Linear of the benchmarked STDiT / PixArt-Sigma configurations.  Bit-identical to the
// general form (tested).
// The tile form of a launch.  ldo and gate_rows are what the interior form's EPILOGUE needs beyond interior tiles: 8-element
// aligned output rows, and - gate epilogue - rows_per_gate a multiple of the tile height, so that the gate folds into the
// staged scales for every tile; an epilogue without output rows / without a gate passes 0.  VQ_ESHAPE: `variant` 19 on a
// shape the interior form does not cover.
struct GemmForm {
    bool half, interior;
};
static int vq_gemm_form(int M, int N, int sets, int variant, int ldo, int gate_rows, GemmForm& f) {
    f.half = variant == 16 || (variant == VQ_GEMM_DEFAULT && vq_half_tiles(M, N, sets));
    const int bm = f.half ? 128 : 256;
    const bool interior = M % bm == 0 && N % 288 == 0 && (ldo & 7) == 0 && gate_rows % bm == 0;
    if (variant == 19 && !interior) return VQ_ESHAPE;          // (variant 19 is never a half tile)
    f.interior = variant == 19 || (variant == VQ_GEMM_DEFAULT && interior);
    return VQ_OK;
}
// go(tile height, INT) as integral constants
template <class F>
static int vq_gemm_dispatch_form(const GemmForm& f, F&& go) {
    using H = std::integral_constant<int, 128>;
    using T = std::integral_constant<int, 256>;
    if (f.interior) return f.half ? go(H{}, std::integral_constant<int, 1>{}) : go(T{}, std::integral_constant<int, 1>{});
    return f.half ? go(H{}, std::integral_constant<int, 0>{}) : go(T{}, std::integral_constant<int, 0>{});
}
template <bool W4>
static int launch_gemm_auto(const GemmArgs& a, hipStream_t st, int variant) {
    const int sets = a.nbatch > 1 ? a.nbatch : a.ngroups > 1 ? a.ngroups : 1;
    GemmForm f;
    if (const int rc = vq_gemm_form(a.M, a.N, sets, variant, a.ldo, a.epilogue == VQ_EPI_GATE_RESID ? a.rows_per_gate : 0, f))
        return rc;
    return vq_gemm_dispatch_form(f, [&](auto bm, auto interior) {
        return launch_gemm_wide<decltype(bm)::value, 288, 4, 2, W4, decltype(interior)::value>(a, st);
    });
}
extern "C" int vq_gemm_i8(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R, const void* wq,
                          const float* sw, const int32_t* zw, const int32_t* cs, const float* bias, void* out,
                          int ldo, const void* resid, const float* gate, int rows_per_gate, int M, int N, int K,
                          int Kp, int w_bits, int epilogue, int variant, void* stream) {
    if (!xq || !sx || !zx || !R || !wq || !sw || !zw || !cs || !out) return VQ_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0) return VQ_EINVAL;
    const int ops = vq_gemm_operand_check(M, N, K, Kp);
    if (ops == VQ_GEMM_OPS_KP || N % 4 != 0 || ldo % 4 != 0 || ldo < N) return VQ_ESHAPE;
    if (w_bits < 2 || w_bits > 8) return VQ_EUNSUP;
    if (epilogue < VQ_EPI_NONE || epilogue > VQ_EPI_RESID) return VQ_EUNSUP;
    if ((epilogue == VQ_EPI_GATE_RESID || epilogue == VQ_EPI_RESID) && !resid) return VQ_EINVAL;
    if (epilogue == VQ_EPI_GATE_RESID && (!gate || rows_per_gate <= 0)) return VQ_EINVAL;
    if (ops != VQ_GEMM_OPS_OK) return VQ_ESHAPE;
    GemmArgs a{xq, sx, zx, R, (const uint8_t*)wq, sw, zw, cs, bias, (half_t*)out, (const half_t*)resid, gate,
               ldo, rows_per_gate > 0 ? rows_per_gate : 1, M, N, K, Kp, epilogue, 0};
    hipStream_t st = (hipStream_t)stream;
    switch (variant) {
        case VQ_GEMM_DEFAULT:  // tile height by shape (vq_half_tiles)
        case 11:               // 256 x 288 tile: full-line double buffer, 128 bytes of k per row and stage, staggered DMA issue
        case 16:               // 128 x 288 tile of the same kernel
        case 19:               // 256 x 288 tile, interior form: scalar-addressed pieces, waves 0-3 issue (VQ_ESHAPE unless M % 256 == 0,
                               // N % 288 == 0, ldo % 8 == 0 and - gate epilogue - rows_per_gate % 256 == 0)
            if (w_bits <= 4) return launch_gemm_auto<true>(a, st, variant);
            return launch_gemm_auto<false>(a, st, variant);
        default:
            break;
    }
    return VQ_EUNSUP;
}

// One activation, nbatch stacked weight sets (e.g. the kv_linear of every transformer block applied to the same
// prompt tokens): out[b] [M, N] = dequant(xq . wq[b]^T) + bias[b].  Default kernel only, no fused epilogue.
extern "C" int vq_gemm_i8_batched(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R, const void* wq,
                                  const float* sw, const int32_t* zw, const int32_t* cs, const float* bias, void* out,
                                  int nbatch, int M, int N, int K, int Kp, int w_bits, void* stream) {
    if (!xq || !sx || !zx || !R || !wq || !sw || !zw || !cs || !out) return VQ_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || nbatch <= 0) return VQ_EINVAL;
    const int ops = vq_gemm_operand_check(M, N, K, Kp);
    if (ops == VQ_GEMM_OPS_KP || N % 4 != 0) return VQ_ESHAPE;
    if (w_bits <= 4 || w_bits > 8) return VQ_EUNSUP;
    if (ops != VQ_GEMM_OPS_OK) return VQ_ESHAPE;
    GemmArgs a{xq, sx, zx, R, (const uint8_t*)wq, sw, zw, cs, bias, (half_t*)out, nullptr, nullptr,
               N, 1, M, N, K, Kp, VQ_EPI_NONE, 0};
    a.nbatch = nbatch;
    a.bs_w = (long)N * Kp;
    a.bs_ch = N;
    a.bs_out = (long)M * N;
    return launch_gemm_auto<false>(a, (hipStream_t)stream, VQ_GEMM_DEFAULT);
}

// ngroups (2 or 3) independent Linears of one shape in one grid: out_g [M, N] = dequant(xq_g . wq_g^T) + bias_g, written
// to out + g * N with row pitch ldo (the q | k | v column blocks of one [M, 3N] buffer).  The plans that smooth every
// Linear against its own weight quantize the shared input three times (quant_layer.py:136-160), so q / k / v cannot be
// one N = 3C GEMM; as three launches each is a single round of 256 tiles whose prologue and store drain nothing
// overlaps.  Default kernel, no fused epilogue.
extern "C" int vq_gemm_i8_grouped(int ngroups, const int8_t* const* xq, const float* const* sx, const int32_t* const* zx,
                                  const int32_t* const* R, const void* const* wq, const float* const* sw,
                                  const int32_t* const* zw, const int32_t* const* cs, const float* const* bias, void* out,
                                  int ldo, int M, int N, int K, int Kp, int w_bits, void* stream) {
    if (ngroups < 1 || ngroups > 3 || !xq || !sx || !zx || !R || !wq || !sw || !zw || !cs || !out) return VQ_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0) return VQ_EINVAL;
    const int ops = vq_gemm_operand_check(M, N, K, Kp);
    if (ops == VQ_GEMM_OPS_KP || N % 4 != 0 || ldo % 4 != 0 || ldo < ngroups * N) return VQ_ESHAPE;
    if (w_bits < 2 || w_bits > 8) return VQ_EUNSUP;
    if (ops != VQ_GEMM_OPS_OK) return VQ_ESHAPE;
    for (int g = 0; g < ngroups; ++g)
        if (!xq[g] || !sx[g] || !zx[g] || !R[g] || !wq[g] || !sw[g] || !zw[g] || !cs[g]) return VQ_EINVAL;
    GemmArgs a{xq[0], sx[0], zx[0], R[0], (const uint8_t*)wq[0], sw[0], zw[0], cs[0], bias ? bias[0] : nullptr,
               (half_t*)out, nullptr, nullptr, ldo, 1, M, N, K, Kp, VQ_EPI_NONE, 0};
    a.ngroups = ngroups;
    for (int g = 1; g < ngroups; ++g)
        a.grp[g - 1] = GemmArgs::Group{xq[g], sx[g], zx[g], R[g], (const uint8_t*)wq[g], sw[g], zw[g], cs[g],
                                       bias ? bias[g] : nullptr, (half_t*)out + (size_t)g * N};
    hipStream_t st = (hipStream_t)stream;
    if (w_bits <= 4) return launch_gemm_auto<true>(a, st, VQ_GEMM_DEFAULT);
    return launch_gemm_auto<false>(a, st, VQ_GEMM_DEFAULT);
}

// cross_attn.q_linear + cross attention against the prompt's <= 128 keys in ONE launch of the 256 x 288 interior tile with
// the cross-attention epilogue (gemm_common.h, ring_epilogue_cross): q [M, N] is never written.  Replaces F.linear
// (quant_layer.py:211) + the xformers block-diagonal attention of MultiHeadCrossAttention (blocks.py:302-304); o is
// bit-identical to vq_gemm_i8(VQ_EPI_NONE) + vq_attn_fwd.  Every check comes before any HIP call or dereference.
extern "C" int vq_gemm_i8_cross_attn(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R, const void* wq,
                                     const float* sw, const int32_t* zw, const int32_t* cs, const float* bias, const void* k,
                                     const void* v, void* o, int M, int N, int K, int Kp, int w_bits, int n_seq, int Lq, int Lk,
                                     int H, int D, long kv_seq_stride, long kv_tok_stride, long o_seq_stride, long o_tok_stride,
                                     const int32_t* kv_off, float scale, void* stream) {
    if (!xq || !sx || !zx || !R || !wq || !sw || !zw || !cs || !k || !v || !o) return VQ_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || n_seq <= 0 || Lq <= 0 || H <= 0 || Lk <= 0) return VQ_EINVAL;
    // what vq_gemm_i8 refuses ...
    if (vq_gemm_operand_check(M, N, K, Kp) != VQ_GEMM_OPS_OK) return VQ_ESHAPE;
    if (w_bits < 2 || w_bits > 8) return VQ_EUNSUP;
    // ... the tile: interior 256 x 288 tiles of 4 whole heads, every tile inside one sample
    if (D != 72) return VQ_EUNSUP;
    if (M % 256 != 0 || N % 288 != 0 || (long)N != (long)H * D || (long)M != (long)n_seq * Lq || Lq % 256 != 0) return VQ_ESHAPE;
    // ... and the attention: resident images of <= 128 keys addressed with 32-bit byte offsets, 16-byte rows
    if (Lk > 128 || (long)Lk * kv_tok_stride * 2 >= (1L << 31)) return VQ_ESHAPE;
    if ((kv_tok_stride | kv_seq_stride | o_tok_stride | o_seq_stride) % 8 != 0 || kv_tok_stride < D || o_tok_stride < N) return VQ_ESHAPE;
    if (((uintptr_t)xq | (uintptr_t)wq | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 != 0) return VQ_ESHAPE;
    if (n_seq > 65535) return VQ_ESHAPE;
    GemmXArgs a{};
    static_cast<GemmArgs&>(a) = GemmArgs{xq, sx, zx, R, (const uint8_t*)wq, sw, zw, cs, bias, nullptr, nullptr, nullptr,
                                         N, 1, M, N, K, Kp, VQ_EPI_NONE, 0};
    a.at = AttnArgs{nullptr, (const half_t*)k, (const half_t*)v, (half_t*)o, 0, 0, kv_seq_stride, kv_tok_stride, o_seq_stride,
                    o_tok_stride, kv_off, n_seq, Lq, Lk, H, scale * ATT_LOG2E};
    hipStream_t st = (hipStream_t)stream;
    if (w_bits <= 4) return launch_gemm_tiles<gemm_i8_cross_attn_kernel<true>, 256, 288, 4, 2, true>(a, st);
    return launch_gemm_tiles<gemm_i8_cross_attn_kernel<false>, 256, 288, 4, 2, false>(a, st);
}

// R[0, n) = 0 in front of a quantizing launch (every wave adds its columns' part of a row's term).  A kernel, not
// hipMemsetAsync: a memset node captured into a graph took effect in no replay (attention.hip, attn_zero_rows_kernel).
__global__ void gemm_zero_rows_kernel(int32_t* R, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) R[i] = 0;
}

// mlp.fc1 + GELU(tanh) + fc2's STATIC tensor-wise activation quantizer: the GEMM of vq_gemm_i8(VQ_EPI_GELU) with the
// quantizing epilogue (gemm_common.h, ring_epilogue_quant) in the four forms launch_gemm_auto picks, 8-bit weights.
// Replaces F.linear (quant_layer.py:211) + nn.GELU(approximate="tanh") (blocks.py:27) + ActQuantizer.forward after init_done
// (base_quantizer.py:129-144) behind the smooth-quant division (quant_layer.py:140).  Every check comes before any HIP call
// or dereference.
extern "C" int vq_gemm_i8_rowquant_static(const int8_t* xq, const float* sx, const int32_t* zx, const int32_t* R,
                                          const void* wq, const float* sw, const int32_t* zw, const int32_t* cs,
                                          const float* bias, const float* s, const float* s_rcp, const float* delta,
                                          const float* zp, int8_t* xq_out, float* sx_out, int32_t* zx_out, int32_t* R_out,
                                          int M, int N, int K, int Kp, int Kp_out, int w_bits, int n_bits, int variant,
                                          void* stream) {
    if (!xq || !sx || !zx || !R || !wq || !sw || !zw || !cs || !delta || !zp || !xq_out || !sx_out || !zx_out || !R_out)
        return VQ_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || Kp <= 0 || Kp_out <= 0) return VQ_EINVAL;
    // what vq_gemm_i8 refuses (N % 8 covers its N % 4) ...
    if (vq_gemm_operand_check(M, N, K, Kp) != VQ_GEMM_OPS_OK) return VQ_ESHAPE;
    // ... and the quantizer's: whole 8-byte runs of codes, rows the int8 GEMM reads, 16-byte chunk stores and float4 reads
    if (N % 8 != 0 || Kp_out % 128 != 0 || Kp_out < N) return VQ_ESHAPE;
    if ((((uintptr_t)xq_out | (uintptr_t)s | (uintptr_t)s_rcp) & 15u) != 0) return VQ_ESHAPE;
    GemmForm f;                                                // (the quantizing epilogue: no output rows, no gate)
    if (const int rc = vq_gemm_form(M, N, 1, variant, 0, 0, f)) return rc;
    if (w_bits <= 4 || w_bits > 8) return VQ_EUNSUP;           // nibble weights: no quantizing form
    if (n_bits < 2 || n_bits > 8) return VQ_EUNSUP;
    if (s && !s_rcp) return VQ_EUNSUP;                         // the division exists in reciprocal form only
    if (variant != VQ_GEMM_DEFAULT && variant != 11 && variant != 16 && variant != 19) return VQ_EUNSUP;
    GemmQArgs a{};
    static_cast<GemmArgs&>(a) = GemmArgs{xq, sx, zx, R, (const uint8_t*)wq, sw, zw, cs, bias, nullptr, nullptr, nullptr,
                                         N, 1, M, N, K, Kp, VQ_EPI_GELU, 0};
    a.qs = s, a.qs_rcp = s ? s_rcp : nullptr, a.qdelta = delta, a.qzp = zp;
    a.qxq = xq_out, a.qsx = sx_out, a.qzx = zx_out, a.qR = R_out, a.Kp_out = Kp_out, a.n_bits = n_bits;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gemm_zero_rows_kernel, dim3((M + 255) / 256), dim3(256), 0, st, R_out, M);
    if (const int rc = vq_check_launch()) return rc;
    return vq_gemm_dispatch_form(f, [&](auto bm, auto interior) {
        constexpr int BM = decltype(bm)::value;
        return launch_gemm_tiles<gemm_i8_wide_quant_kernel<BM, 288, 4, 2, decltype(interior)::value>, BM, 288, 4, 2, false>(a, st);
    });
}

// attn_lab.hip - LAB ONLY: every attention arm that is not a product route, launched by an explicit kernel id (the form
// vq_lab_gemm_i8 has for the GEMM).  This translation unit includes csrc/attention.hip - the product's kernels, argument
// checks and launchers, unchanged - and adds the retired kernels (attn_phased.h, attn_stream.h) and the wider
// instantiations of attn_fwd32d / attn_fwd64d.  Every experiment behind these ids is concluded: profiles/r05_experiments.md,
// r06_attention_phases.md (the profiling ablations of attn_fwd8 / attn_fwd32d are gone with their template parameters; what
// they measured is in profiles/r04_experiments.md and r06_attention_phases.md).
// Part of libviditq_lab.so (tools/lab/build.py); the product library never sees this file.  (libviditq_lab.so therefore
// also carries a copy of attention.hip's own entry points; nothing in tools/ calls those.)
#include "attention.hip"
#include "attn_stream.h"
#include "attn_phased.h"

// Kernel ids of vq_lab_attn_fwd.  < 0: the product's own choice (the control arm, from the same build).
#define VQ_LAB_ATTN_K_FWD32D_NW4 4      // attn_fwd32d_kernel<72, 4, 64> (round 5; the id it had in include/viditq.h)
#define VQ_LAB_ATTN_K_64D_128 100       // attn_fwd64d_kernel<D, 8, 128>
#define VQ_LAB_ATTN_K_64D_NW4 101       // attn_fwd64d_kernel<D, 4, 64>
#define VQ_LAB_ATTN_K_64P 102           // attn_fwd64p_kernel, ring of 3 tile images (attn_phased.h)
#define VQ_LAB_ATTN_K_64S 103           // attn_fwd64s_kernel (attn_stream.h)
#define VQ_LAB_ATTN_K_64P_NB4 104       // attn_fwd64p_kernel, ring of 4

// The lab kernels share the tile images of attn_fwd32d_kernel and with them its preconditions: one key length for all
// sequences, more than two key tiles, K / V addressed with 32-bit byte offsets.  VQ_ESHAPE where a kernel cannot run the
// shape, VQ_EUNSUP for an id (or an id / head dim pair) without a kernel.
template <int D>
static int lab_launch_attn(int kernel, const AttnArgs& a, hipStream_t st) {
    if (kernel < 0) return launch_attn<D>(a, st);
    if (a.kv_off || a.Lk <= 128) return VQ_ESHAPE;
    if ((long)a.Lk * a.kv_tok_stride * 2 >= (1l << 31)) return VQ_ESHAPE;
    if (kernel == VQ_LAB_ATTN_K_FWD32D_NW4) {
        if (a.Lq < 192) return VQ_ESHAPE;
        if constexpr (D == 72) return launch_attn32d<D, 4>(a, st);
        return VQ_EUNSUP;
    }
    if (a.Lq < 512) return VQ_ESHAPE;
    switch (kernel) {
        case VQ_LAB_ATTN_K_64D_128: return launch_attn64d<D, 8, 128>(a, st);
        case VQ_LAB_ATTN_K_64D_NW4: return launch_attn64d<D, 4, 64>(a, st);
        case VQ_LAB_ATTN_K_64P: if constexpr (D >= 64) return launch_attn64p<D, 3>(a, st); break;
        case VQ_LAB_ATTN_K_64P_NB4: if constexpr (D >= 64) return launch_attn64p<D, 4>(a, st); break;
        case VQ_LAB_ATTN_K_64S:
            if constexpr (D % 8 == 0 && D >= 64) {
                // more than one query tile; >= 64 D / 512 key tiles (that many carry the parked O rows out); Q parked by
                // LDS-DMA with 32-bit byte offsets
                if (a.Lq <= 512 || a.Lk < 64 * (64 * D * 2 / 1024) || (long)a.Lq * a.q_tok_stride * 2 >= (1l << 31)) return VQ_ESHAPE;
                return launch_attn64s<D>(a, st);
            }
            break;
        default: break;
    }
    return VQ_EUNSUP;
}

// vq_attn_fwd with the kernel named by the caller
extern "C" int vq_lab_attn_fwd(int kernel, const void* q, const void* k, const void* v, void* o, int n_seq, int Lq, int Lk, int H,
                               int D, long q_seq_stride, long q_tok_stride, long kv_seq_stride, long kv_tok_stride,
                               long o_seq_stride, long o_tok_stride, const int32_t* kv_off, float scale, void* stream) {
    AttnArgs a;
    const int rc = attn_fwd_args(q, k, v, o, n_seq, Lq, Lk, H, q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride,
                                 o_seq_stride, o_tok_stride, kv_off, scale, &a);
    if (rc != VQ_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    return vq_dispatch_head_dim(D, [&](auto d) { return lab_launch_attn<d()>(kernel, a, st); });
}

// The phased kernel with cycle stamps (D = 72, ring of 3): stamps = uint32[workgroups][8 waves][16].  tools/attn_stamps.py
extern "C" int vq_lab_attn64p_stamped(const void* q, const void* k, const void* v, void* o, int n_seq, int Lq, int Lk, int H,
                                      long q_seq_stride, long q_tok_stride, long kv_seq_stride, long kv_tok_stride,
                                      long o_seq_stride, long o_tok_stride, float scale, void* stamps, void* stream) {
    AttnArgs a;
    const int rc = attn_fwd_args(q, k, v, o, n_seq, Lq, Lk, H, q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride,
                                 o_seq_stride, o_tok_stride, nullptr, scale, &a);
    if (rc != VQ_OK) return rc;
    if (!stamps) return VQ_EINVAL;
    if (Lk <= 128 || Lq < 512 || (long)Lk * kv_tok_stride * 2 >= (1l << 31)) return VQ_ESHAPE;
    constexpr int NB = 3;
    constexpr int LDS = NB * (Att8Cfg<72, 8>::KTILE + 64 * 192);
    constexpr auto kern = attn_fwd64p_kernel<72, NB, 1>;
    if (const int rc2 = vq_prepare_kernel<kern>(LDS)) return rc2;
    const int nqt = (Lq + 511) / 512, G = n_seq * H;
    hipLaunchKernelGGL(kern, dim3(8 * ((G + 7) / 8) * nqt), dim3(512), LDS, (hipStream_t)stream, a, (long long*)stamps);
    return vq_check_launch();
}

// vq_attn_temporal_rowquant on the round-3 kernel (attn_temporal_quant_kernel) where the product runs the trimmed
// attn_temporal_quant2_kernel: the control arm of that A/B
extern "C" int vq_lab_attn_temporal_rowquant_v1(const void* q, const void* k, const void* v, const float* s, const float* s_rcp,
                                                int8_t* xq, float* sx, int32_t* zx, int32_t* R, int32_t* status, void* o, int B,
                                                int T, int S, int H, int D, long ld_in, int Kp, float scale, void* stream) {
    TempQArgs a;
    if (const int rc = temporal_quant_args(q, k, v, s, s_rcp, xq, sx, zx, R, status, o, B, T, S, H, D, ld_in, Kp, scale, &a)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return vq_dispatch_head_dim(D, [&](auto d) { return launch_temporal_quant<d()>(a, st, false); });
}

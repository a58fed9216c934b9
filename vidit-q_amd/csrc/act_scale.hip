// act_scale.hip - the running smooth-quant act-scale statistic on the device, for gfx950.
//
// Replaces: QuantLayer's momentum statistic at inference (qdiff/models/quant_layer.py:118-126, :147-154 - the per-channel
// abs-max of the layer's input, averaged over the batch, folded into act_scale with a momentum) and the zero patch of the
// channel-wise scale (:128-133), which the reference evaluates with host-visible tests (`.abs().mean() == 0`,
// `(== 0).sum() != 0`).  Here nothing leaves the device: three launches on the caller's stream, capturable in a graph.
//
//   act_scale_zero_kernel     scratch[B*C] = 0 (a kernel, not hipMemsetAsync: see attn_zero_rows_kernel, attention.hip)
//   act_scale_colmax_kernel   scratch[b*C + c] = max over tok of (bits(x[b, tok, c]) & 0x7fff)
//   act_scale_finalize_kernel mean over b, all-zero test, momentum update, zero patch
//
// The column maximum is taken on the fp16 BIT PATTERNS with the sign cleared: for finite values the integer order of
// `bits & 0x7fff` is the order of |x|, and an integer maximum does not depend on the order in which rows, waves and
// workgroups arrive - the atomic exchange between workgroups is bit-reproducible.  (Precondition: finite inputs.  A NaN
// pattern is larger than every finite one and would win, as it does in torch's amax.)
//
// Column-max kernel: a pure HBM reader (PixArt-Sigma 1024^2, mlp.fc2: 8192 x 4608 fp16 = 75 MB).  A lane owns 8 consecutive
// columns (one 16-byte load per row), a wave 512 columns, the four waves of a workgroup take every fourth row of the
// workgroup's slab of rows and keep a packed 16-bit maximum (v_pk_max_u16) in four registers; they combine through 4 KiB of
// LDS and the workgroup issues ONE integer atomic per column.  A slab never mixes two samples b; the host sizes it so that
// the launch is about ACS_TARGET_WGS workgroups (16 waves per CU at 256 CUs) whatever the shape.
#include "vq_common.h"

#define ACS_WAVES 4
#define ACS_THREADS (ACS_WAVES * 64)
#define ACS_COLS (64 * 8)          // columns of a workgroup
#define ACS_UNROLL 4               // 16-byte loads in flight per lane
#define ACS_TARGET_WGS 1024

typedef unsigned short ushort8v __attribute__((ext_vector_type(8)));

__global__ void act_scale_zero_kernel(uint32_t* p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

__device__ __forceinline__ int4v acs_max(int4v acc, int4v v) {
    const int4v mask = {0x7fff7fff, 0x7fff7fff, 0x7fff7fff, 0x7fff7fff};
    v &= mask;
    return __builtin_bit_cast(int4v, __builtin_elementwise_max(__builtin_bit_cast(ushort8v, acc), __builtin_bit_cast(ushort8v, v)));
}

// grid (ceil(C / 512), slabs per sample, B); rows [t0, t1) of sample b
__global__ __launch_bounds__(ACS_THREADS) void act_scale_colmax_kernel(const half_t* __restrict__ x, uint32_t* scratch, int n_tok,
                                                                      int C, int slab) {
    __shared__ __attribute__((aligned(16))) int4v part[ACS_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = blockIdx.x * ACS_COLS + lane * 8;
    const int b = blockIdx.z;
    const int t0 = blockIdx.y * slab;
    const int t1 = min(t0 + slab, n_tok);
    int4v acc = {0, 0, 0, 0};
    if (col < C) {                                        // (C % 8 == 0: the lane's 8 columns are inside the row)
        const half_t* p = x + ((size_t)b * n_tok) * C + col;
        int t = t0 + wv;
        for (; t + (ACS_UNROLL - 1) * ACS_WAVES < t1; t += ACS_UNROLL * ACS_WAVES) {
            int4v v[ACS_UNROLL];
#pragma unroll
            for (int u = 0; u < ACS_UNROLL; ++u)
                v[u] = *reinterpret_cast<const int4v*>(p + (size_t)(t + u * ACS_WAVES) * C);
#pragma unroll
            for (int u = 0; u < ACS_UNROLL; ++u) acc = acs_max(acc, v[u]);
        }
        for (; t < t1; t += ACS_WAVES) acc = acs_max(acc, *reinterpret_cast<const int4v*>(p + (size_t)t * C));
    }
    part[wv][lane] = acc;
    __syncthreads();
    // thread i takes packed word i of the 256 of a row of `part`: columns 2 i and 2 i + 1 of the workgroup
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&part[0][0]);
    uint32_t lo = 0u, hi = 0u;
#pragma unroll
    for (int k = 0; k < ACS_WAVES; ++k) {
        const uint32_t v = w[k * 256 + threadIdx.x];
        lo = max(lo, v & 0xffffu);
        hi = max(hi, v >> 16);
    }
    const int c = blockIdx.x * ACS_COLS + 2 * (int)threadIdx.x;
    if (c < C) {                                          // (C even: c + 1 < C too)
        uint32_t* s = scratch + (size_t)b * C + c;
        atomicMax(s, lo);
        atomicMax(s + 1, hi);
    }
}

// One workgroup.  cur[c] = (m[0][c] + m[1][c] + ... in order) / B; all-zero statistic: act_scale = cur, else
// act_scale = RN(RN(act_scale * momentum) + RN(cur * one_minus_momentum)) - three roundings, no contraction; then the
// entries that are exactly zero become 1e-5.
__global__ __launch_bounds__(ACS_THREADS) void act_scale_finalize_kernel(const uint32_t* __restrict__ scratch, float* act_scale,
                                                                        float* cur_out, float momentum, float one_minus_momentum,
                                                                        int B, int C) {
    int nz = 0;
    for (int c = threadIdx.x; c < C; c += ACS_THREADS) nz |= act_scale[c] != 0.0f;   // (|a| mean == 0 <=> every entry +-0)
    const bool init = !__syncthreads_or(nz);              // (also orders the reads above before the writes below)
    for (int c = threadIdx.x; c < C; c += ACS_THREADS) {
        float sum = 0.0f;
        for (int b = 0; b < B; ++b)
            sum = __fadd_rn(sum, (float)__builtin_bit_cast(half_t, (uint16_t)scratch[(size_t)b * C + c]));
        const float cur = __fdiv_rn(sum, (float)B);
        float a = cur;
        if (!init) a = __fadd_rn(__fmul_rn(act_scale[c], momentum), __fmul_rn(cur, one_minus_momentum));
        if (a == 0.0f) a = 1.0e-5f;
        act_scale[c] = a;
        if (cur_out) cur_out[c] = cur;
    }
}

extern "C" int vq_act_scale_momentum(const void* x, float* act_scale, float* cur_out, uint32_t* scratch, float momentum,
                                     float one_minus_momentum, int B, int n_tok, int C, void* stream) {
    if (!x || !act_scale || !scratch) return VQ_EINVAL;
    if (B <= 0 || n_tok <= 0 || C <= 0) return VQ_EINVAL;
    if (!(momentum >= 0.0f && momentum <= 1.0f)) return VQ_EINVAL;
    if ((long)B * C > 0x7fffffffL || B > 65535) return VQ_EINVAL;
    if (C % 8 != 0 || ((uintptr_t)x & 15u) != 0) return VQ_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int n = B * C;
    hipLaunchKernelGGL(act_scale_zero_kernel, dim3((n + 255) / 256), dim3(256), 0, st, scratch, n);
    if (const int rc = vq_check_launch()) return rc;
    const int cgs = (C + ACS_COLS - 1) / ACS_COLS;
    // slabs per sample: about ACS_TARGET_WGS workgroups in all, at least one row per wave, at most 65535 (grid.y)
    long want = ACS_TARGET_WGS / ((long)B * cgs);
    const long most = (n_tok + ACS_WAVES - 1) / ACS_WAVES;
    if (want > most) want = most;
    if (want < 1) want = 1;
    int slab = (int)((n_tok + want - 1) / want);
    if ((n_tok + slab - 1) / slab > 65535) slab = (n_tok + 65534) / 65535;
    const int slabs = (n_tok + slab - 1) / slab;
    hipLaunchKernelGGL(act_scale_colmax_kernel, dim3(cgs, slabs, B), dim3(ACS_THREADS), 0, st, (const half_t*)x, scratch, n_tok,
                       C, slab);
    if (const int rc = vq_check_launch()) return rc;
    hipLaunchKernelGGL(act_scale_finalize_kernel, dim3(1), dim3(ACS_THREADS), 0, st, scratch, act_scale, cur_out, momentum,
                       one_minus_momentum, B, C);
    return vq_check_launch();
}

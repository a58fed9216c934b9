// patch_embed.hip - the patch embedding in ONE launch for gfx950: gather + Linear + position-embedding add, the front edge
// of STDiT's (PatchEmbed3D, blocks.py:66-105) and PixArt's (timm PatchEmbed) forward.  For token n = (t, i, j) of sample b
// (row-major over D / pt, H / ph, W / pw) and channel c:
//   a[b, n, c]   = fp16( sum_k fp16(x[b, ci, t pt + dt, i ph + dh, j pw + dw]) * w[c, k] + bias[c] ),
//                  k = ((ci pt + dt) ph + dh) pw + dw                      (the flatten order of the Conv weight)
//   out[b, n, c] = pos ? fp16( float(a) + float(pos[n % pos_rows, c]) ) : a
// It replaces a reshape / permute / reshape copy of the latent, its cast, vq_linear_f16 (K <= 32 form) and torch's
// "+ pos_embed", with the same operands, the same placement of k in v_mfma_f32_16x16x32_f16 and the same two roundings:
// the result is theirs bit for bit.
//
// The problem is output-bound (STDiT 16x64x64: latent 1 MB, weight 36 KB, output 37.7 MB per sample), so the kernel is
// built around the stores and around reading the weight once per workgroup.
//
// Work split.  A workgroup is four waves and walks 16-token tiles in a grid-stride loop; the grid is sized to the device
// (two workgroups per CU), not to the tile count.  The channels are dealt to the waves in GROUPS of 32: wave v owns groups
// v, v + 4, v + 8, ... (9 each at C = 1152, 12 at the cap 1536; 1, 1, 1, 0 at C = 96; a wave without a group leaves).  A
// wave loads the weight fragments (A operand: lane lq = lane & 15 one weight row, its 8 consecutive k from 8 g4, g4 = lane
// >> 4; zero where 8 g4 >= K) and the bias of ITS groups once, before the loop, and keeps them in registers: two 16-row
// tiles x 4 VGPRs + 4 VGPRs of bias per group.
//
// Store pattern.  A lane of the MFMA's D^T owns one token and rows 4 g4 .. 4 g4 + 3 of the A operand - and WHICH channel
// sits in an A row is free.  The two tiles of a group are loaded with their rows interleaved in fours: row i of tile 0 is
// channel c0 + 8 (i / 4) + i % 4, row i of tile 1 the channel 4 further.  A lane then holds channels c0 + 8 g4 .. + 7 of its
// token in order - no exchange between lanes, no LDS - and writes them with ONE 16-byte store; a wave store instruction
// covers 16 rows x 64 contiguous bytes, and the four waves of the workgroup, which run in step, cover 256 contiguous bytes
// of each row.  The position row is read with the same addressing (16 bytes per lane from an L2-resident table) and the
// bias the same way (once).  A last group of 16 channels (C % 32 == 16) keeps the plain row order and 8-byte stores.
//
// Gather.  The token fragment (B operand: lane lq one token, 8 consecutive k) is read straight from the latent: a lane
// works out the 8 element offsets of ITS k once (they depend on g4 only), a tile adds the token's origin.  k and k + 1 are
// neighbours in W when pw is even: four 2-element loads (PAIR), else eight.  Neighbouring tokens of a row are neighbouring
// pw-element pieces, so the 16 lanes of one g4 read one contiguous run.  No patchified copy exists.  The token coordinates
// (b, t, i, j) and n % pos_rows are decoded once before the loop and CARRIED from tile to tile by the decoded stride with one
// conditional subtraction per digit: no integer division in the loop.  The next tile's fragment is requested before this
// tile's results leave.  fp32 latents are rounded to fp16 as they arrive.
//
// Ragged edges.  A tile may straddle samples (every lane carries its own coordinates).  Lanes of the last tile past row
// B N gather from element 0 of x, read position row (their own) n % pos_rows < pos_rows, and store nothing.
// No LDS, no barrier.
//
// Refusals of vq_patch_embed_f16, in this order, all before any HIP call or dereference:
//   1. VQ_EINVAL  x, w or out null (bias and pos may be null)
//   2. VQ_EINVAL  B, Cin, D, H, W, pt, ph, pw, C or ldw not positive; pos given with pos_rows not positive
//   3. VQ_ESHAPE  D % pt, H % ph or W % pw != 0; K = Cin pt ph pw with K % 8 != 0 or K > 32; C % 16 != 0 or C > 1536;
//                 pos given with N % pos_rows != 0; B Cin D H W >= 2^31
//   4. VQ_ESHAPE  ldw % 8 != 0 or ldw < K
//   5. VQ_ESHAPE  x, w, out, a non-null bias or a non-null pos not 16-byte aligned
//   6. VQ_EUNSUP  x_f32 neither 0 (fp16 latent) nor 1 (fp32 latent)
#include "vq_common.h"

#define PE_WAVES 4
#define PE_THREADS (64 * PE_WAVES)
#define PE_MAX_C 1536
#define PE_MAX_K 32
#define PE_PER_CU 2

typedef __attribute__((ext_vector_type(2))) _Float16 half2v;

struct PeArgs {
    const void* x;
    const half_t *w, *bias, *pos;
    half_t* out;
    long ldw;
    int M, tiles;                        // token rows B * N, 16-row tiles
    int C, K, pos_rows;                  // pos_rows = 1 without pos
    int pt, ph, pw, Dp, Hp, Wp;          // patch, token grid
    int W, HW, DHW, CDHW;                // latent pitches in elements: row, frame, channel, sample
};

// mixed-radix token coordinates of one lane, and the step that carries them
struct PeTok {
    int j, i, t, b, pr;
};

__device__ __forceinline__ PeTok pe_decode(int m, const PeArgs& a) {
    PeTok c;
    c.pr = m % a.pos_rows;
    c.j = m % a.Wp, m /= a.Wp;
    c.i = m % a.Hp, m /= a.Hp;
    c.t = m % a.Dp, c.b = m / a.Dp;
    return c;
}

__device__ __forceinline__ void pe_advance(PeTok& c, const PeTok& s, const PeArgs& a) {
    c.pr += s.pr;
    c.pr -= c.pr >= a.pos_rows ? a.pos_rows : 0;
    c.j += s.j;
    int carry = c.j >= a.Wp;
    c.j -= carry ? a.Wp : 0;
    c.i += s.i + carry;
    carry = c.i >= a.Hp;
    c.i -= carry ? a.Hp : 0;
    c.t += s.t + carry;
    carry = c.t >= a.Dp;
    c.t -= carry ? a.Dp : 0;
    c.b += s.b + carry;
}

// the token fragment of one lane: its 8 k of the token whose origin is element xo of the latent
template <typename T, bool PAIR>
__device__ __forceinline__ half8 pe_gather(const T* __restrict__ x, long xo, const int (&koff)[8], bool live) {
    half8 f = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
    if (live) {
        if constexpr (PAIR) {
            typedef __attribute__((ext_vector_type(2))) T pair_t;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const pair_t v = *reinterpret_cast<const pair_t*>(x + xo + koff[2 * p]);
                f[2 * p] = (half_t)v[0], f[2 * p + 1] = (half_t)v[1];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (half_t)x[xo + koff[e]];
        }
    }
    return f;
}

// T: the latent's type; PAIR: pw even; NG: channel groups a wave holds (C <= 128 NG)
template <typename T, bool PAIR, int NG>
__global__ __launch_bounds__(PE_THREADS, PE_PER_CU) void patch_embed_kernel(const PeArgs a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane & 15, g4 = lane >> 4;
    const int C = a.C, ngroups = (C + 31) >> 5;
    if (wave >= ngroups) return;                              // C = 16 .. 96: fewer groups than waves
    const bool live = 8 * g4 < a.K;                           // K % 8 == 0: a lane's 8 k are all there or all padding
    const bool has_pos = a.pos != nullptr;
    const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
    const half8 z8 = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};

    // ---- once: this wave's weight fragments and bias
    half8 wa[NG][2], bs[NG];
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        const int c0 = 32 * (wave + PE_WAVES * u);
        wa[u][0] = wa[u][1] = bs[u] = z8;
        if (c0 < C) {
            const bool full = c0 + 32 <= C;
            const int r0 = full ? c0 + 8 * (lq >> 2) + (lq & 3) : c0 + lq;
            if (live) {
                wa[u][0] = *reinterpret_cast<const half8*>(a.w + (size_t)r0 * a.ldw + 8 * g4);
                if (full) wa[u][1] = *reinterpret_cast<const half8*>(a.w + (size_t)(r0 + 4) * a.ldw + 8 * g4);
            }
            if (a.bias) {
                if (full) {
                    bs[u] = *reinterpret_cast<const half8*>(a.bias + c0 + 8 * g4);
                } else {
                    const half4 b4 = *reinterpret_cast<const half4*>(a.bias + c0 + 4 * g4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) bs[u][r] = b4[r];
                }
            }
        }
    }

    // ---- once: the element offsets of this lane's k, its token's coordinates and the stride's
    int koff[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        int k = live ? 8 * g4 + e : 0;
        const int dw = k % a.pw;
        k /= a.pw;
        const int dh = k % a.ph;
        k /= a.ph;
        koff[e] = (k / a.pt) * a.DHW + (k % a.pt) * a.HW + dh * a.W + dw;
    }
    int m = blockIdx.x * 16 + lq;
    PeTok tok = pe_decode(m, a);
    const PeTok step = pe_decode((int)gridDim.x * 16, a);
    auto origin = [&](int mm, const PeTok& c) -> long {
        return mm < a.M ? (long)c.b * a.CDHW + (long)(c.t * a.pt) * a.HW + (c.i * a.ph) * a.W + c.j * a.pw : 0;
    };
    half8 nxt = pe_gather<T, PAIR>(x, origin(m, tok), koff, live);

    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const half8 xb = nxt;
        const bool valid = m < a.M;
        half_t* orow = a.out + (size_t)m * C + 8 * g4;
        const half_t* prow = has_pos ? a.pos + (size_t)tok.pr * C + 8 * g4 : nullptr;
        // the next tile's fragment is requested before this one's results leave
        m += (int)gridDim.x * 16;
        pe_advance(tok, step, a);
        if (tile + (int)gridDim.x < a.tiles) nxt = pe_gather<T, PAIR>(x, origin(m, tok), koff, live);
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int c0 = 32 * (wave + PE_WAVES * u);
            if (c0 < C) {
                const float4v zero = {0.f, 0.f, 0.f, 0.f};
                const float4v acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[u][0], xb, zero, 0, 0, 0);
                if (c0 + 32 <= C) {
                    const float4v acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[u][1], xb, zero, 0, 0, 0);
                    half8 p8 = z8, o;
                    if (has_pos) p8 = *reinterpret_cast<const half8*>(prow + c0);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        o[e] = (half_t)((e < 4 ? acc0[e & 3] : acc1[e & 3]) + (float)bs[u][e]);
                        if (has_pos) o[e] = (half_t)((float)o[e] + (float)p8[e]);
                    }
                    if (valid) *reinterpret_cast<half8*>(orow + c0) = o;
                } else {                                      // the last 16 channels of a C % 32 == 16: plain row order
                    half4 p4 = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f}, o;
                    if (has_pos) p4 = *reinterpret_cast<const half4*>(prow - 4 * g4 + c0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        o[r] = (half_t)(acc0[r] + (float)bs[u][r]);
                        if (has_pos) o[r] = (half_t)((float)o[r] + (float)p4[r]);
                    }
                    if (valid) *reinterpret_cast<half4*>(orow - 4 * g4 + c0) = o;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
template <typename T, bool PAIR, int NG>
static int pe_launch(const PeArgs& a, hipStream_t st) {
    constexpr auto k = patch_embed_kernel<T, PAIR, NG>;
    int ncu = 0;
    const int e = vq_prepare_kernel<k>(1024, &ncu);
    if (e != VQ_OK) return e;
    const int cap = ncu * PE_PER_CU;
    hipLaunchKernelGGL(k, dim3((unsigned)(a.tiles < cap ? a.tiles : cap)), dim3(PE_THREADS), 0, st, a);
    return vq_check_launch();
}

template <typename T, bool PAIR>
static int pe_dispatch(const PeArgs& a, hipStream_t st) {
    if (a.C <= 128 * 3) return pe_launch<T, PAIR, 3>(a, st);
    if (a.C <= 128 * 9) return pe_launch<T, PAIR, 9>(a, st);
    return pe_launch<T, PAIR, 12>(a, st);
}

static bool pe_misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

extern "C" int vq_patch_embed_f16(const void* x, int x_f32, const void* w, const void* bias, const void* pos, void* out,
                                  int B, int Cin, int D, int H, int W, int pt, int ph, int pw, int C, int pos_rows, long ldw,
                                  void* stream) {
    if (!x || !w || !out) return VQ_EINVAL;
    if (B <= 0 || Cin <= 0 || D <= 0 || H <= 0 || W <= 0 || pt <= 0 || ph <= 0 || pw <= 0 || C <= 0 || ldw <= 0)
        return VQ_EINVAL;
    if (pos && pos_rows <= 0) return VQ_EINVAL;
    if (D % pt != 0 || H % ph != 0 || W % pw != 0) return VQ_ESHAPE;
    if (Cin > PE_MAX_K || pt > PE_MAX_K || ph > PE_MAX_K || pw > PE_MAX_K) return VQ_ESHAPE;
    const int K = Cin * pt * ph * pw;                         // each factor <= 32: no overflow
    if (K % 8 != 0 || K > PE_MAX_K || C % 16 != 0 || C > PE_MAX_C) return VQ_ESHAPE;
    const long cap = 1L << 31;
    long n = (long)(D / pt) * (H / ph);                       // < 2^62
    n = n < cap ? n * (W / pw) : cap;
    long elems = (long)D * H;
    elems = elems < cap ? elems * W : cap;
    elems = elems < cap ? elems * Cin : cap;
    elems = elems < cap ? elems * B : cap;
    if (elems >= cap) return VQ_ESHAPE;                       // (then N and B N are below 2^31 too)
    if (pos && n % pos_rows != 0) return VQ_ESHAPE;
    if (ldw % 8 != 0 || ldw < K) return VQ_ESHAPE;
    if (pe_misaligned(x) || pe_misaligned(w) || pe_misaligned(out) || pe_misaligned(bias) || pe_misaligned(pos))
        return VQ_ESHAPE;
    if (x_f32 != 0 && x_f32 != 1) return VQ_EUNSUP;
    PeArgs a{};
    a.x = x, a.w = (const half_t*)w, a.bias = (const half_t*)bias, a.pos = (const half_t*)pos, a.out = (half_t*)out;
    a.ldw = ldw, a.M = (int)(B * n), a.tiles = (a.M + 15) / 16;
    a.C = C, a.K = K, a.pos_rows = pos ? pos_rows : 1;
    a.pt = pt, a.ph = ph, a.pw = pw, a.Dp = D / pt, a.Hp = H / ph, a.Wp = W / pw;
    a.W = W, a.HW = H * W, a.DHW = D * H * W, a.CDHW = Cin * D * H * W;
    hipStream_t st = (hipStream_t)stream;
    const bool pair = pw % 2 == 0;
    if (x_f32) return pair ? pe_dispatch<float, true>(a, st) : pe_dispatch<float, false>(a, st);
    return pair ? pe_dispatch<half_t, true>(a, st) : pe_dispatch<half_t, false>(a, st);
}

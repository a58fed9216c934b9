// attn_tile.h - the steps the flash-style kernels behind vq_attn_fwd share (attn_fwd_kernel, attn_fwd8_kernel,
// attn_fwd32d_kernel, attn_fwd64d_kernel, attn_cross32_kernel of attention.hip; the lab's attn_stream.h / attn_phased.h).
//
// The layout all of them use: v_mfma_f32_32x32x16_f16 with lane = (l31 = lane & 31, g = lane >> 5).  S^T = K Q^T leaves
// lane (l31, g) with 16 keys of query l31 (attn_key), O^T = V^T P^T with dims 32 dt + 8 rg + 4 g .. + 3 of query l31; column
// D of every V image is 1.0, so row D of O^T is the softmax row sum.  A kernel body is its SCHEDULE - issue, QK^T chain,
// decide, exp, P.V, barrier, with its sched_barriers and pins; each step is written once, here, with the hazard and
// compiler-quirk notes that belong to it.
#pragma once
#include "vq_common.h"
#include "attn_rowquant.h"

#define ATT_LOG2E 1.4426950408889634f

// The argument block of every vq_attn_fwd kernel (filled by attn_fwd_args of attention.hip); it lives here because the
// geometry steps below take it.
struct AttnArgs {
    const half_t* q;
    const half_t* k;
    const half_t* v;
    half_t* o;
    long q_seq_stride, q_tok_stride, kv_seq_stride, kv_tok_stride, o_seq_stride, o_tok_stride;
    const int32_t* kv_off;
    int n_seq, Lq, Lk, H;
    float c;  // scale * log2(e)
};

// The static-grid forms (the kernels instantiated on AttnQSArgs; vq_attn_fwd_rowquant_static) add the consuming Linear's
// calibrated tensor-wise quantizer - its grid one fp32 value each, read by the kernel - the code width and the quantizer's
// outputs; `o` is optional there.  The plain forms keep their argument block as it was.
struct AttnQSArgs : AttnArgs {
    const float* s;                                // nullable [H*D]: smooth-quant channel scale of the consuming Linear
    const float* s_rcp;                            //                 and its reciprocal (vq_smooth_reciprocal)
    const float* delta;
    const float* zp;
    int8_t* xq;                                    // [n_seq*Lq, Kp] codes, dense rows (row = seq * Lq + query)
    float* sx;
    int32_t* zx;
    int32_t* R;                                    // zero when the kernel starts: every head ADDS its part of a row's term
    int Kp, n_bits;                                // n_bits 2 .. 8
};

// ---- geometry ----------------------------------------------------------------------------------------------------------
// Workgroup -> (sequence, head, query tile of `wg_rows` queries).  Workgroups are dealt round-robin to the 8 XCDs; XCD x
// takes a CONTIGUOUS range of the (sequence, head) pairs and runs the query tiles of a pair back to back, so a pair's
// K/V panel is fetched into that XCD's L2 once for all its query tiles, and neighbouring heads (whose 2*D-byte row
// segments share cache lines) sit in the same L2.  With the plain (qt, h, seq) grid the 4 query tiles of a pair ran on 4
// different XCDs: 341 MB read for 113 MB of q/k/v (profiles/r01_hbm_traffic.md), and re-staging K/V cost 50 of 188 us.
// false: a padded grid slot (the whole workgroup leaves: no barrier reached yet).
__device__ __forceinline__ bool attn_xcd_map(const AttnArgs& a, int wg_rows, int& qt, int& h, int& seq) {
    const int nqt = (a.Lq + wg_rows - 1) / wg_rows;
    const int G = a.n_seq * a.H;
    const int bid = blockIdx.x, xcd = bid & 7, idx = bid >> 3;
    const int q8 = G / 8, r8 = G % 8;
    const int gbase = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
    const int gcount = xcd < r8 ? q8 + 1 : q8;
    const int pl = idx / nqt;
    if (pl >= gcount) return false;
    const int pair = gbase + pl;
    qt = idx - pl * nqt;
    seq = pair / a.H;
    h = pair - seq * a.H;
    return true;
}

// K / V rows of (seq, h) and their number: packed by a.kv_off, or a.Lk rows per sequence.  `cap` > 0: the kernels with
// resident K / V images take at most that many keys (the host guarantees no more).
template <int D>
__device__ __forceinline__ int attn_kv_base(const AttnArgs& a, int seq, int h, const half_t*& kbase, const half_t*& vbase, int cap = 0) {
    int kv_len = a.Lk;
    if (a.kv_off) {
        const int o0 = a.kv_off[seq];
        kv_len = a.kv_off[seq + 1] - o0;
        kbase = a.k + (long)o0 * a.kv_tok_stride + h * D;
        vbase = a.v + (long)o0 * a.kv_tok_stride + h * D;
    } else {
        kbase = a.k + (long)seq * a.kv_seq_stride + h * D;
        vbase = a.v + (long)seq * a.kv_seq_stride + h * D;
    }
    return cap > 0 && kv_len > cap ? cap : kv_len;
}

// key (row of S^T; key0: the first key of the 32-key half tile) that accumulator register r of half-wave g holds
__device__ __forceinline__ constexpr int attn_key(int r, int g, int key0 = 0) { return key0 + (r & 3) + 8 * (r >> 2) + 4 * g; }

// ---- operands ----------------------------------------------------------------------------------------------------------
// MFMA operand fragment ks of a row of D halves: 8 dims at ks * 16 + 8 g, zero for d0 >= D (head_dim 72 is contracted as
// 5 k-steps of 16 with a zero tail).  ZT = false: the tail is read as it lies (the other operand's zero tail covers it).
template <int D, bool ZT = true>
__device__ __forceinline__ half8 attn_frag(const void* row, int ks, int g) {
    const int d0 = ks * 16 + 8 * g;
    half8 f = *reinterpret_cast<const half8*>(reinterpret_cast<const uint8_t*>(row) + (d0 < D ? d0 : 0) * 2);
    if (ZT && d0 >= D)
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (half_t)0.f;
    return f;
}
// Q fragments (B operand: lane = query) straight from a global row: the tail is not read at all
template <int D, int KS>
__device__ __forceinline__ void attn_q_frags(const half_t* qrow, int g, half8 (&qf)[KS]) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int d0 = ks * 16 + 8 * g;
        if (d0 < D) qf[ks] = *reinterpret_cast<const half8*>(qrow + d0);
        else
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[ks][e] = (half_t)0.f;
    }
}
template <int DT>
__device__ __forceinline__ void attn_zero(float16v (&oacc)[DT]) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
}
// V^T fragments (A operand: lane = output dim, 8 keys) of a ROW-major V image by LDS transpose reads.  attn_vtr0: the
// lane's byte offset inside a 16-key step; attn_vt_frag: fragment idx = k2 * DT + dt of the 32-key half tile at `vhalf`
// (= image + first key row * VRB + attn_vtr0).
union AttnVF {
    half8 v;
    h4_t h[2];
};
template <int VRB>
__device__ __forceinline__ int attn_vtr0(int lane, int g) {
    return (4 * g + ((lane & 15) >> 2)) * VRB + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
}
template <int DT, int VRB>
__device__ __forceinline__ void attn_vt_frag(const uint8_t* vhalf, int idx, AttnVF& vf) {
    const uint8_t* vp = vhalf + 16 * (idx / DT) * VRB + (idx % DT) * 64;
    vf.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4_t*)(vp));
    vf.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4_t*)(vp + 8 * VRB));
}
// Fragment n of a 32-key half tile in the order its MFMAs consume them: K fragments 0 .. KS-1 (`krow`: row l31 of the half
// in the K image), then V^T fragments 0 .. 2 DT - 1; past the end: nothing.  The kernels call it a fixed distance ahead of
// the MFMAs.
template <int D, int VRB, int KS, int DT2>
__device__ __forceinline__ void attn_read_frag(int n, const uint8_t* krow, const uint8_t* vhalf, int g, half8 (&kf)[KS], AttnVF (&vf)[DT2]) {
    if (n < KS) kf[n] = attn_frag<D, false>(krow, n, g);
    else if (n - KS < DT2) attn_vt_frag<DT2 / 2, VRB>(vhalf, n - KS, vf[n - KS]);
}

// ---- tile delivery by LDS-DMA (buffer_load_dwordx4 ... lds) -----------------------------------------------------------
// A wave-instruction fills 64 consecutive 16-byte slots of a [rows][SL slots] image; slot -> (row, piece) is the ordinary
// padded row-major layout, lanes whose slot is padding (piece >= CHD) are masked off, rows past `nrec` bytes are out of the
// buffer's range and land as zeros.
__device__ __forceinline__ unsigned attn_lds_addr(const void* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const uint8_t*)p;
}
struct AttnDmaSlot {
    bool ok;
    int voff;
};
template <int SL, int CHD, int ROWS = 0>                   // ROWS > 0: an image of that many rows that ends inside an instruction
__device__ __forceinline__ AttnDmaSlot attn_dma_slot(int instr, int lane, int strideB) {   // instruction `instr` of one image
    const int slot = instr * 64 + lane, row = slot / SL, piece = slot - row * SL;
    return {(ROWS == 0 || row < ROWS) && piece < CHD, row * strideB + piece * 16};
}
// One wave-instruction: 64 slots from `base` (+ the lane's voff, num_records nrec) to LDS byte address dst.
// Issued through asm: the builtin makes the compiler order every later ds_read behind the DMA (vmcnt(0) before the first
// MFMAs of the tile); the only consumer-side wait needed is the one in attn_wg_barrier().  Hazards the recognizer would
// handle for its own instructions are spelled out: s_nop 4 covers the M0 write -> LDS-DMA rule (1 wait state) and a
// VALU-written (v_readfirstlane) resource SGPR -> VMEM read (5).
__device__ __forceinline__ void attn_dma_instr(const void* base, unsigned nrec, unsigned dst, const AttnDmaSlot& sl) {
    const unsigned long ba = (unsigned long)base;
    const int4v rs = {(int)__builtin_amdgcn_readfirstlane((unsigned)ba), (int)__builtin_amdgcn_readfirstlane((unsigned)(ba >> 32) & 0xffffu),
                      (int)__builtin_amdgcn_readfirstlane(nrec), 0x00020000};
    if (sl.ok)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(dst), "v"(sl.voff), "s"(rs)
                     : "memory", "m0");
}
// The K tile and the V tile of KT keys (K rows KROW bytes, V rows VRB bytes with the pad columns behind the data) as one
// sequence of wave-instructions j = wave + NW * i, K first.
template <int D, int NW, int KT, int KROW, int VRB>
struct AttnKvDma {
    static constexpr int CHD = D / 8, KSL = KROW / 16, VSL = VRB / 16;   // 16-byte pieces per head row, slots per image row
    static constexpr int NKI = KSL * (KT / 64), NVI = VSL * (KT / 64);   // wave-instructions (64 slots) per K / V tile
    static constexpr int NI = NKI + NVI, IPW = (NI + NW - 1) / NW;
    AttnDmaSlot sl[IPW];
    __device__ __forceinline__ void init(int wave, int lane, int strideB) {
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int j = wave + NW * i;                   // wave-uniform
            sl[i] = j < NKI ? attn_dma_slot<KSL, CHD>(j, lane, strideB) : attn_dma_slot<VSL, CHD>(j - NKI, lane, strideB);
            sl[i].ok = sl[i].ok && j < NI;
        }
    }
    // The tile at byte offset t0 of kbase / vbase (nrec: num_records of the whole K / V panel) -> the images at LDS byte
    // addresses kdst / vdst.  part 0: round i == 0 only, 1: the other rounds, -1: all.  CLAMP: tiles wholly past nrec are
    // issued too (a resident image is filled with zeros).
    template <bool CLAMP = false>
    __device__ __forceinline__ void issue(const half_t* kbase, const half_t* vbase, unsigned t0, unsigned nrec, unsigned kdst,
                                          unsigned vdst, int wave, int part = -1) const {
        const unsigned left = CLAMP ? (nrec > t0 ? nrec - t0 : 0u) : nrec - t0;
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int j = wave + NW * i;
            if (j < NI && (part < 0 || (part == 0) == (i == 0))) {
                const bool isk = j < NKI;
                const unsigned dst = __builtin_amdgcn_readfirstlane(isk ? kdst + j * 1024 : vdst + (j - NKI) * 1024);
                attn_dma_instr(reinterpret_cast<const uint8_t*>(isk ? kbase : vbase) + t0, left, dst, sl[i]);
            }
        }
    }
};
// DMA landed and visible to every wave (and every wave done with the buffer that is overwritten next)
__device__ __forceinline__ void attn_wg_barrier() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// pad columns of `rows` contiguous V image rows (never written by the DMA): column D = 1.0, the rest 0
template <int D, int VRB>
__device__ __forceinline__ void attn_fill_pad(uint8_t* vimg, int rows, int tid, int nthr) {
    for (int i = tid; i < rows * 3; i += nthr) {
        const int r = i / 3, ch = i % 3;
        *reinterpret_cast<int4v*>(vimg + r * VRB + D * 2 + ch * 16) = int4v{ch == 0 ? 0x00003c00 : 0, 0, 0, 0};
    }
}

// ---- softmax -----------------------------------------------------------------------------------------------------------
// ragged tile: keys at or past kv_len leave the softmax (key0: the first key of this 32-key half tile).  Masked in a local
// copy: written on the referenced accumulator element by element, a kernel with two query blocks per wave came out with
// the 16 lane masks of each combined through chains of scalar ORs (82 more instructions and 25 more SGPRs per ragged tile).
__device__ __forceinline__ void attn_mask(float16v& s, int key0, int g, int kv_len) {
    float16v t = s;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (attn_key(r, g, key0) >= kv_len) t[r] = -INFINITY;
    s = t;
}
// Row maximum of a query over the keys of the tile: the lane's registers, then the other half-wave.  Three spellings that
// generate different code, each where it was measured.
// (1) attn_fwd32d (attn_fwd64d has the same chain written out in its softmax block) - v_max3 chain in asm: fmaxf() would canonicalise every MFMA result first (one extra v_max
// each).  The hazard recognizer does not look at asm operands: an asm VALU read of an accumulator the matrix core is still
// writing gets NO wait states and sees the previous contents (with one k-step, D = 16: the last tile's exponentials - a
// garbage running max, rows of zeros / NaN).  So the first read of the fresh accumulator is a compiler-visible VALU
// instruction (x + 0.0f is not foldable); the asm chain depends on it.  ONE statement for the whole chain: between two
// dependent asm statements the compiler pads a wait state (an asm producer may write with dst_sel:
// DstSelForwardingHazard) - 8 s_nop per 32-key half otherwise.
__device__ __forceinline__ float attn_rowmax_max3(const float16v& s) {
    float mx, mloc;
    const float s0 = s[0] + 0.0f;
    asm("v_max3_f32 %0, %1, %2, %3\n\tv_max3_f32 %0, %0, %4, %5\n\tv_max3_f32 %0, %0, %6, %7\n\t"
        "v_max3_f32 %0, %0, %8, %9\n\tv_max3_f32 %0, %0, %10, %11\n\tv_max3_f32 %0, %0, %12, %13\n\t"
        "v_max3_f32 %0, %0, %14, %15\n\tv_max_f32 %0, %0, %16"
        : "=&v"(mx)
        : "v"(s0), "v"(s[1]), "v"(s[2]), "v"(s[3]), "v"(s[4]), "v"(s[5]), "v"(s[6]), "v"(s[7]), "v"(s[8]), "v"(s[9]),
          "v"(s[10]), "v"(s[11]), "v"(s[12]), "v"(s[13]), "v"(s[14]), "v"(s[15]));
    const unsigned mb = __builtin_bit_cast(unsigned, mx);
    const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
    asm("v_max_f32 %0, %1, %2" : "=v"(mloc) : "v"(sw[0]), "v"(sw[1]));
    return mloc;
}
// (2) attn_cross32 - fmaxf and the lane swap.  The two halves are copied out of the vector FIRST: hipcc of ROCm 7.2 reads
// element 0 for BOTH operands of __builtin_bit_cast(float, sw[i]) written on the vector elements directly - rounds 4-5
// shipped the kernel with the maximum over only half of the keys of a 32-key tile: still an exact softmax, the reference
// point just was not the row maximum, so P could exceed the 2^8 the lazy rescale assumes; found in round 6.
__device__ __forceinline__ float attn_rowmax_swap(const float16v& s) {
    float mx = fmaxf(fmaxf(s[0], s[1]), s[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, s[r]), s[r + 1]);
    mx = fmaxf(mx, s[15]);
    const unsigned mb = __builtin_bit_cast(unsigned, mx);
    const auto sw = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
    const unsigned sw0 = sw[0], sw1 = sw[1];
    return fmaxf(__builtin_bit_cast(float, sw0), __builtin_bit_cast(float, sw1));
}
// (3) attn_fwd / attn_fwd8 - fmaxf over both 32-key halves of a 64-key tile and __shfl_xor
__device__ __forceinline__ float attn_rowmax_shfl(const float16v (&s)[2]) {
    float mloc = s[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, s[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[1][r]);
    return fmaxf(mloc, __shfl_xor(mloc, 32));
}
// Deferred rescale: the running max (and O) moves only when some lane's tile max leads it by more than 8 in the exp2
// domain, so P <= 2^8 in between (fp16-safe) and the DT x 16-register rescale of O^T runs on the first tiles only.
// Returns the exponent offset mc = running max * c.
template <int DT>
__device__ __forceinline__ float attn_lazy_rescale(float mloc, float& m_run, float16v (&oacc)[DT], float c) {
    if (__any((mloc - m_run) * c > 8.0f)) {
        const float m_new = fmaxf(m_run, mloc);
        const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * c);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
        m_run = m_new;
    }
    return ((m_run == -INFINITY) ? 0.f : m_run) * c;
}
// P^T = exp2(s * c - mc) as the two B operands of the P.V MFMAs (16 fma + 16 v_exp + 8 cvt, straight-line).
// Two plain v_fma_f32, NOT one v_pk_fma_f32: beside the partner waves' MFMAs the packed form costs more than the issue slot
// it saves (and a forwarding wait state in front of v_exp) - round 6, one box, alternating x 3: 115.4 -> 111.0 us at
// 16 x 1024 x 1024, 187.3 -> 177.6 us at 2 x 4096 x 4096 (profiles/r06_experiments.md 1); attn_cross32: 30.0-31.2 vs
// 31.2-32.4 us (profiles/r06_experiments.md 8).
__device__ __forceinline__ void attn_exp_pack(const float16v& s, float c, float mc, half8 (&pf)[2]) {
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const float t0 = __builtin_fmaf(s[r], c, -mc), t1 = __builtin_fmaf(s[r + 1], c, -mc);
        pf[r >> 3][r & 7] = (half_t)__builtin_amdgcn_exp2f(t0);
        pf[r >> 3][(r & 7) + 1] = (half_t)__builtin_amdgcn_exp2f(t1);
    }
}

// ---- epilogue ----------------------------------------------------------------------------------------------------------
// 1 / row sum of query l31.  Row D of O^T = sum_k P: it lives in tile D / 32, register (D % 32 -> attn_key) of ONE half-wave.
template <int D, int DT>
__device__ __forceinline__ float attn_inv_row_sum(const float16v (&oacc)[DT], int l31) {
    constexpr int LD_T = D / 32, LD_R = D % 32;
    constexpr int LD_G = (LD_R >> 2) & 1, LD_REG = (LD_R & 3) + 4 * (LD_R >> 3);
    static_assert(DT * 32 > D && attn_key(LD_REG, LD_G) == LD_R, "needs a spare O^T row for the row sums");
    float l_run = oacc[LD_T][LD_REG];
    l_run = __shfl(l_run, l31 + 32 * LD_G);
    return l_run > 0.f ? __fdiv_rn(1.0f, l_run) : 0.f;
}
// normalise and store a query's row, 8-byte stores: accumulator quads = 4 consecutive dims.  The caller masks the row.
template <int D, int DT>
__device__ __forceinline__ void attn_store_rows_h4(const float16v (&oacc)[DT], float inv, half_t* orow, int g) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int d = dt * 32 + 8 * rg + 4 * g;
            if (d < D) {
                half4 ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = (half_t)(oacc[dt][rg * 4 + e] * inv);
                *reinterpret_cast<half4*>(orow + d) = ov;
            }
        }
}
// 16-byte stores (D % 8 == 0).  O^T leaves the 32 x 32 matrix core with 4 consecutive dims per lane and (dt, rg) group, the
// partner lane (g ^ 1) holding the other half of each 8-dim group: one v_permlane32_swap per dword turns two groups into 8
// consecutive dims per lane - 32 contiguous bytes per row and instruction instead of 16 (the store tail of a row-per-lane
// epilogue is bound by store INSTRUCTIONS, not bytes: 9 -> 5 per lane at D = 72).  Every lane of the wave must call this
// (the swaps are wave-wide); `row_ok` masks the stores only.  Round 4: cross attention; round 6: the self-attention kernels.
template <int D, int DT>
__device__ __forceinline__ void attn_store_rows(const float16v (&oacc)[DT], float inv, half_t* orow, int g, bool row_ok) {
    static_assert(D % 8 == 0 && D >= 16, "16-byte store epilogue");
    constexpr int NG = D / 8;                           // 8-dim groups: dt = grp / 4, rg = grp % 4
#pragma unroll
    for (int p2 = 0; p2 < NG / 2; ++p2) {
        const int ga = 2 * p2, gb = 2 * p2 + 1;
        uint32_t A[2], B[2];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
            const h2_t ha = {(half_t)(oacc[ga / 4][(ga % 4) * 4 + 2 * w] * inv), (half_t)(oacc[ga / 4][(ga % 4) * 4 + 2 * w + 1] * inv)};
            const h2_t hb = {(half_t)(oacc[gb / 4][(gb % 4) * 4 + 2 * w] * inv), (half_t)(oacc[gb / 4][(gb % 4) * 4 + 2 * w + 1] * inv)};
            A[w] = __builtin_bit_cast(uint32_t, ha);
            B[w] = __builtin_bit_cast(uint32_t, hb);
        }
        // swap(A, B): first result = {low lanes: A of g = 0, high lanes: B of g = 0}, second = {A of g = 1, B of g = 1}
        const auto s0 = __builtin_amdgcn_permlane32_swap(A[0], B[0], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(A[1], B[1], false, false);
        const int4v ov = {(int)s0[0], (int)s1[0], (int)s0[1], (int)s1[1]};
        if (row_ok) *reinterpret_cast<int4v*>(orow + 16 * p2 + 8 * g) = ov;
    }
    if constexpr (NG % 2 == 1) {                        // the odd last group: 8-byte stores
        constexpr int gl = NG - 1;
        half4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = (half_t)(oacc[gl / 4][(gl % 4) * 4 + e] * inv);
        if (row_ok) *reinterpret_cast<half4*>(orow + 8 * gl + 4 * g) = ov;
    }
}

// ---- epilogue of the static-grid forms: the consuming Linear's quantizer on the row the steps above store ----------------
// Codes of the lane's 8-dim groups (dims 8 grp + 4 g .. + 3 of query l31, as attn_store_rows numbers them) on the grid `sq`,
// from the value those steps store - float(half(oacc * inv)) - divided by the smoothing vector `s` (of this head; null: none)
// in reciprocal form.  One dword of codes per group; one v_permlane32_swap turns the dwords of two groups into 8
// consecutive codes per lane (8-byte stores; the odd last group: 4-byte stores).  Every lane of the wave must call this
// (the swaps are wave-wide); `row_ok` masks the stores only.  Returns the sum of the lane's raw codes (v_sad_u8).
// (the swap builtin returns a 2-vector: its elements are copied into scalars before they are used - attn_rowquant.h)
template <int D, int DT, bool SAT8>
__device__ __forceinline__ uint32_t attn_quant_codes(const float16v (&oacc)[DT], float inv, const float* s, const float* s_rcp,
                                                     const TqGrid& sq, int8_t* xrow, int g, bool row_ok) {
    static_assert(D % 8 == 0 && D >= 16, "8-dim groups, 8-byte code stores");
    constexpr int NG = D / 8;                           // 8-dim groups: dt = grp / 4, rg = grp % 4
    uint32_t csum = 0;
    auto codes = [&](int grp) __attribute__((always_inline)) {
        float x4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x4[e] = (float)(half_t)(oacc[grp / 4][(grp % 4) * 4 + e] * inv);
        if (s) {                                        // kernel-uniform
            const float4v s4 = *reinterpret_cast<const float4v*>(s + 8 * grp + 4 * g);
            const float4v r4 = *reinterpret_cast<const float4v*>(s_rcp + 8 * grp + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) x4[e] = rq_div_rcp(x4[e], s4[e], r4[e]);
        }
        return tq_static_codes<SAT8>(x4, sq, csum);
    };
#pragma unroll
    for (int p2 = 0; p2 < NG / 2; ++p2) {
        const uint32_t A = codes(2 * p2), B = codes(2 * p2 + 1);
        // swap(A, B): first result = {low lanes: A of g = 0, high lanes: B of g = 0}, second = {A of g = 1, B of g = 1}
        const auto sw = __builtin_amdgcn_permlane32_swap(A, B, false, false);
        const uint32_t c0 = sw[0], c1 = sw[1];
        if (row_ok) *reinterpret_cast<uint2*>(xrow + 16 * p2 + 8 * g) = make_uint2(c0, c1);
    }
    if constexpr (NG % 2 == 1) {
        const uint32_t pk = codes(NG - 1);
        if (row_ok) *reinterpret_cast<uint32_t*>(xrow + 8 * (NG - 1) + 4 * g) = pk;
    }
    return csum;
}
// Quantizer outputs of query row `row` (= seq * Lq + query; lane l31 of both half-waves) for head h.  Codes: above.  The
// row term R = sum(raw codes) - C * (int)zp crosses the heads, which sit in different workgroups: every head adds
// sum(raw codes of its D dims) - D * (int)zp to R[row] - zeroed by the entry point on the same stream - with ONE relaxed
// agent-scope integer atomic per row, issued by the g = 0 lanes: 32 consecutive rows = one 128-byte segment per
// wave-instruction.  Integer adds commute, so R is bit-reproducible.  sx / zx: the head-0 workgroups; the pad columns
// [H * D, Kp): the last head's.  Rows with !row_ok (clamped duplicates of row Lq - 1) write and add nothing.
template <int D, int DT>
__device__ __forceinline__ void attn_quant_rows(const float16v (&oacc)[DT], float inv, const AttnQSArgs& a, const TqGrid& sq,
                                                int row, int h, int g, bool row_ok) {
    // (the addresses below are derived HERE: inside attn_cross32_kernel's walk the compiler otherwise computes every one of
    //  them once in front of the loop and keeps them - ~30 VGPRs of lane pointers, spilled - for its whole length)
    asm volatile("" : "+v"(g));
    int8_t* xrow = a.xq + (long)row * a.Kp + h * D;
    const float* s = a.s ? a.s + h * D : nullptr;
    const float* s_rcp = a.s ? a.s_rcp + h * D : nullptr;
    uint32_t csum;
    if (sq.wd.qmax == 255.0f) csum = attn_quant_codes<D, DT, true>(oacc, inv, s, s_rcp, sq, xrow, g, row_ok);   // kernel-uniform
    else csum = attn_quant_codes<D, DT, false>(oacc, inv, s, s_rcp, sq, xrow, g, row_ok);
    const auto sw = __builtin_amdgcn_permlane32_swap(csum, csum, false, false);     // the two halves of the row's dims
    const int c0 = (int)sw[0], c1 = (int)sw[1];
    const int izp = (int)sq.g.zp;
    if (row_ok && g == 0) {
        __hip_atomic_fetch_add(a.R + row, c0 + c1 - D * izp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (h == 0) {
            a.sx[row] = sq.g.delta;
            a.zx[row] = izp - sq.wd.cx;
        }
    }
    if (h == a.H - 1 && row_ok) {                       // pad columns zeroed like the row quantizers do
        int8_t* prow = a.xq + (long)row * a.Kp + a.H * D;
        for (int c = 8 * g; c < a.Kp - a.H * D; c += 16) *reinterpret_cast<uint2*>(prow + c) = make_uint2(0u, 0u);
    }
}

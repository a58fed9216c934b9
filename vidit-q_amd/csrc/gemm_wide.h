// gemm_wide.h - the full-line ring kernel (256 x 288 tile, 8 waves of 64 x 144; 128 x 288 with 32 x 144 wave tiles for
// launches that would otherwise leave half the CUs without a workgroup); see csrc/gemm_i8.hip for the design notes.
// Product forms only (round 6): the measurement arms of rounds 1-5 (main-loop ablations, issuer / prefetch-distance / slab
// switches, the twelve-wave tile) live in tools/lab/gemm_wide_lab.h and are compiled into tools/lab/libviditq_lab.so.
#pragma once
#include "gemm_common.h"

// ---------------------------------------------------------------------------
// Full-line ring kernel.  tools/dma_depth.py: the L2 -> LDS fill rate of a CU is bound by cache-line REQUESTS, not bytes:
// 64-byte row chunks stream at 65 GB/s per CU, 128-byte chunks (one whole line per row) at 127 GB/s.  A 256 x 288 tile at
// full MFMA rate consumes 63 GB/s.  A stage holds 128 bytes of k per row (two MFMA k-steps), every DMA lane group fetches
// whole lines, and the ring is a plain double buffer (2 x 68 KiB):
//   tile kt:  step h=0 | step h=1 ... [j = TN-2: vmcnt(0) + barrier -> DMA(kt+1) landed, stage kt free]
// LDS rows are 128 B with the 16-byte chunk index XOR-ed by (row >> 1) & 7 (W4: 64 B rows, (row >> 2) & 3): every
// ds_read_b128 fragment read is conflict-free for the instruction's real lane groups ({0-3, 12-15, 20-27}, ... - checked in
// profiles/r06_gemm_lds_conflicts.md; the conflicts the counters show belong to the epilogue's slab transposition).
//
// INT 0: general form - any M, N; one clamped VGPR offset per stage piece; every wave issues its share of a stage, waves
//        NW/2.. a few MFMA groups late (an LDS-DMA issue blocks the issuing wave ~60-100 cycles; staggering keeps one SIMD
//        partner on the matrix pipe).
// INT 1: launches made of INTERIOR tiles only (M % BM == 0, N % BN == 0; the launcher checks).  A stage piece is addressed
//        as ONE lane offset per wave (row lane >> 3 of the piece, swizzled 16-byte chunk; it depends on the piece only
//        through its parity, and with an even number of issuing waves all pieces of a wave share one parity) + a SCALAR row
//        / k offset in the buffer instruction's soffset - 2 VGPRs instead of 9; waves 0 .. NW/2-1 (one per SIMD) issue
//        EVERY piece of a stage right behind the stage barrier, their SIMD partners none; the kernel carries only the
//        interior epilogue (197 VGPRs for every epilogue kind).  Bit-identical to INT 0 (tested).
// (Round 6 measured the interior form as PERSISTENT workgroups with the next tile's first stage requested before the epilogue:
//  bit-identical, the saved prologues are paid back by the half-slab epilogue it needs - tools/lab/gemm_wide_r6.h,
//  profiles/r06_experiments.md 5.)
// STAMP: cycle-counter stamps of every wave -> a.gate reinterpreted as long long[tiles][waves][10] (0-6 shader cycles,
//        7/8 100 MHz wall clock at start/end, 9 arrival at the stage barrier of k-tile 1) - bench telemetry (clock_probe.hip: vq_gemm_i8_stamped).
// ---------------------------------------------------------------------------
template <int BM, int BN, int WAVES_M, int WAVES_N, bool W4>
struct WideCfg {
    using Epi = EpiGeom<BM, BN, WAVES_M, WAVES_N>;             // epilogue slabs + parked terms (gemm_common.h)
    static constexpr int NW = Epi::NW, WTM = Epi::WTM, WTN = Epi::WTN;
    static constexpr int WROW = W4 ? 64 : 128;                 // bytes per weight row and stage
    static constexpr int STAGE = BM * 128 + BN * WROW;
    static constexpr int LDS = 2 * STAGE > Epi::BYTES ? 2 * STAGE : Epi::BYTES;
    static_assert(LDS <= 163840, "LDS budget of one CU");
    // The terms are parked behind the epilogue slabs.  For the 256-row tile (and for W4 stages) that is past the end of the
    // ring; for the 128-row tile with 128-byte weight rows the block lies INSIDE stage 1 (gemm_i8_wide_tile, behind its loop).
    static constexpr bool PAR_IN_RING = Epi::PAR_OFF < 2 * STAGE;
    static_assert(PAR_IN_RING || Epi::QS_OFF >= 2 * STAGE, "smoothing vector outside the live ring");
};

// Args: GemmArgs, or GemmQArgs with EPI = VQ_EPI_GELU_QUANT (the quantizing epilogue, ring_epilogue_quant), or GemmXArgs with
// EPI = VQ_EPI_CROSS_ATTN (the cross-attention epilogue, ring_epilogue_cross: interior form of the 256 x 288 tile only)
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, bool W4, bool STAMP = false, int INT = 0, class Args = GemmArgs>
__device__ __forceinline__ void gemm_i8_wide_tile(const Args a0, const int vb, const int tid_) {
    constexpr bool QUANT = EPI == VQ_EPI_GELU_QUANT;
    static_assert(QUANT == std::is_same<Args, GemmQArgs>::value && !(QUANT && (W4 || STAMP)), "the quantizing epilogue: 8-bit weights");
    constexpr bool CROSS = EPI == VQ_EPI_CROSS_ATTN;
    static_assert(CROSS == std::is_same<Args, GemmXArgs>::value && !(CROSS && (STAMP || INT == 0)), "the cross-attention epilogue: interior tiles");
    using Cfg = WideCfg<BM, BN, WAVES_M, WAVES_N, W4>;
    constexpr int NW = Cfg::NW;
    constexpr bool ASYM = INT != 0;                   // one issuing wave per SIMD
    constexpr int NI = ASYM ? NW / 2 : NW;            // issuing waves
    constexpr int WTM = Cfg::WTM, WTN = Cfg::WTN;
    constexpr int TM = WTM / 16, TN = WTN / 16;
    constexpr int WROW = Cfg::WROW;
    constexpr int XP = BM / 8, WP = BN * WROW / 1024; // 1 KiB DMA pieces
    constexpr int STAGE = Cfg::STAGE;
    constexpr int PIECES = XP + WP;
    constexpr int PPW = (PIECES + NI - 1) / NI;
    constexpr int PLAST = PIECES - (PPW - 1) * NI;
    static_assert(INT == 0 || (NI % 2 == 0 && XP % 2 == 0), "one piece parity per issuing wave");
    // weight-fragment ring of three: reads run two channel groups ahead of their MFMAs (3 / 4 / 5 ahead measured flat, round 5)
    constexpr int WPF = 2, WR = 3;
    static_assert((2 * TN) % WR == 0 && WPF < TN, "ring index must repeat per stage");
    constexpr int BARJ = TN - WPF;                    // after the last fragment read of the current stage
    constexpr int DMA_B = TN >= 6 ? 3 : 0;            // late DMA issue point of the staggered half (general form)
    static_assert((TM == 8 || TM == 4 || TM == 2) && TN >= 3 && TN % 3 == 0, "fragment rings below");
    static_assert(BN * WROW % 1024 == 0 && STAGE % 128 == 0, "whole pieces, 128-byte aligned stages");
    static_assert(WTM % 16 == 0 && WTN % 16 == 0, "swizzle phase is taken from the fragment row");

    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    long long* ts = nullptr;
    if constexpr (STAMP) {
        ts = reinterpret_cast<long long*>(const_cast<float*>(a0.gate)) + ((size_t)vb * NW + (tid_ >> 6)) * 10;
        ts[7] = wall_clock64();
        ts[0] = __builtin_readcyclecounter();
    }

    const int tid = tid_, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const bool full_wave = (PIECES % NI == 0) || (wave < PLAST);
    const bool issuer = wave < NI;                                // wave-uniform (INT 0: every wave)
    const bool late = !ASYM && wave >= NW / 2;                    // wave-uniform
    const int MT_ = (a0.M + BM - 1) / BM, NT_ = (a0.N + BN - 1) / BN;
    const int ntiles = MT_ * NT_ * (a0.nbatch > 1 ? a0.nbatch : a0.ngroups > 1 ? a0.ngroups : 1);

    // what a tile's DMA needs: operand bases (as buffer resources) and its first token / channel row
    struct TileSrc {
        int4v rs_x, rs_w;
        int m0, n0;
    };
    auto mk_rsrc = [&](const void* base) {
        const unsigned long ba = (unsigned long)base;
        return int4v{(int)__builtin_amdgcn_readfirstlane((unsigned)ba),
                     (int)__builtin_amdgcn_readfirstlane((unsigned)(ba >> 32) & 0xffffu), (int)0xffffffffu, 0x00020000};
    };
    // virtual block id -> the arguments of its problem (batched / grouped launches) and its tile
    auto select = [&](GemmArgs& a, int vb, TileSrc& t) {
        // (the cross-attention form is one problem per launch: with the arms below compiled in, its larger argument block
        //  stayed in scratch behind the groups' indexed selects and every DMA offset became a vector value)
        if (!CROSS && a.nbatch > 1) {                  // batch-major grid: weight set = vb / tiles
            const int bt = vb / (MT_ * NT_);
            vb -= bt * (MT_ * NT_);
            a.wq += (size_t)bt * a.bs_w;
            a.sw += (size_t)bt * a.bs_ch;
            a.zw += (size_t)bt * a.bs_ch;
            a.cs += (size_t)bt * a.bs_ch;
            if (a.bias) a.bias += (size_t)bt * a.bs_ch;
            a.out += (size_t)bt * a.bs_out;
        } else if (!CROSS && a.ngroups > 1) {          // group-major grid; uniform selects, no indexed copy of the args
            const int g = vb / (MT_ * NT_);
            vb -= g * (MT_ * NT_);
            if (g > 0) {
                const bool g1 = g == 1;
                a.xq = g1 ? a.grp[0].xq : a.grp[1].xq;
                a.sx = g1 ? a.grp[0].sx : a.grp[1].sx;
                a.zx = g1 ? a.grp[0].zx : a.grp[1].zx;
                a.R = g1 ? a.grp[0].R : a.grp[1].R;
                a.wq = g1 ? a.grp[0].wq : a.grp[1].wq;
                a.sw = g1 ? a.grp[0].sw : a.grp[1].sw;
                a.zw = g1 ? a.grp[0].zw : a.grp[1].zw;
                a.cs = g1 ? a.grp[0].cs : a.grp[1].cs;
                a.bias = g1 ? a.grp[0].bias : a.grp[1].bias;
                a.out = g1 ? a.grp[0].out : a.grp[1].out;
            }
        }
        int mt, nt;
        xcd_tile(vb, MT_, NT_, mt, nt);
        t.m0 = mt * BM;
        t.n0 = nt * BN;
        t.rs_x = mk_rsrc(a.xq);
        t.rs_w = mk_rsrc(a.wq);
    };

    uint32_t soff[INT ? 2 : PPW];
    if constexpr (INT != 0) {
        // [0]: token rows (128-byte stage rows), [1]: weight rows (W4: 64-byte rows, 16 per piece - its swizzle phase
        // (row >> 2) & 3 = (lane >> 4) & 3 does not depend on the piece at all)
        soff[0] = (uint32_t)(lane >> 3) * (uint32_t)a0.Kp + (uint32_t)(((lane & 7) ^ (((wave & 1) * 4 + (lane >> 4)) & 7)) * 16);
        soff[1] = W4 ? (uint32_t)(lane >> 2) * (uint32_t)(a0.Kp >> 1) + (uint32_t)(((lane & 3) ^ ((lane >> 4) & 3)) * 16) : soff[0];
    }
    // LDS-DMA through buffer loads: SGPR resource (token or weight base), one VGPR byte offset per piece (constant over
    // k), the k offset in an SGPR - no 64-bit address arithmetic per piece and stage.  Issued through asm with
    // M0 = LDS destination; every wait on these transfers in this kernel is an explicit s_waitcnt vmcnt.  The hazard
    // recognizer does not look inside inline asm: s_nop 4 covers both the M0 write and a resource SGPR that the
    // compiler may have re-materialised with v_readlane right before the asm (VALU-written SGPR -> VMEM: 5 wait states).
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) uint8_t*)smem);
    auto issue = [&](const TileSrc& t, int stage, int kt) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int p = wave + i * NI;
            if (PIECES % NI == 0 || p < PIECES) {
                const unsigned dst = lds0 + stage * STAGE + p * 1024;
                if constexpr (INT != 0) {
                    if (p < XP) {
                        const unsigned so = (unsigned)(t.m0 + p * 8) * (unsigned)a0.Kp + kt * 128;
                        asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(dst), "v"(soff[0]), "s"(t.rs_x), "s"(so)
                                     : "memory", "m0");
                    } else {
                        const unsigned so = W4 ? (unsigned)(t.n0 + (p - XP) * 16) * (unsigned)(a0.Kp >> 1) + kt * 64
                                               : (unsigned)(t.n0 + (p - XP) * 8) * (unsigned)a0.Kp + kt * 128;
                        asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(dst), "v"(soff[1]), "s"(t.rs_w), "s"(so)
                                     : "memory", "m0");
                    }
                } else {
                    const int koff = kt * (p < XP ? 128 : WROW);
                    if (p < XP)
                        asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(dst), "v"(soff[i]), "s"(t.rs_x), "s"(koff)
                                     : "memory", "m0");
                    else
                        asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(dst), "v"(soff[i]), "s"(t.rs_w), "s"(koff)
                                     : "memory", "m0");
                }
            }
        }
    };

    const int frow = lane & 15, fc = lane >> 4;
    // k-step h (0/1) of a stage = chunks 4h..4h+3 of the 128-byte row: the swizzled address of step 1 is
    // the address of step 0 with bit 6 flipped (W4: 8-byte reads of a 64-byte row, bit 5)
    const int xf0 = (wm * WTM + frow) * 128 + ((fc ^ ((frow >> 1) & 7)) * 16);
    const int wf0 = W4 ? BM * 128 + (wn * WTN + frow) * 64 + (((fc >> 1) ^ ((frow >> 2) & 3)) * 16) + (fc & 1) * 8
                       : BM * 128 + (wn * WTN + frow) * 128 + ((fc ^ ((frow >> 1) & 7)) * 16);
    const int xf1 = xf0 ^ 64, wf1 = wf0 ^ (W4 ? 32 : 64);
    using WRaw = typename std::conditional<W4, int2v, int4v>::type;
    auto ldx = [&](int stage, int h, int i) {
        return *reinterpret_cast<const int4v*>(smem + stage * STAGE + (h ? xf1 : xf0) + i * 16 * 128);
    };
    auto ldw = [&](int stage, int h, int j) {
        return *reinterpret_cast<const WRaw*>(smem + stage * STAGE + (h ? wf1 : wf0) + j * 16 * WROW);
    };
    auto wop = [&](const WRaw& r) -> int4v {
        if constexpr (W4) {
            return int4v{r[0] & 0x0F0F0F0F, (int)(((uint32_t)r[0] >> 4) & 0x0F0F0F0Fu), r[1] & 0x0F0F0F0F,
                         (int)(((uint32_t)r[1] >> 4) & 0x0F0F0F0Fu)};
        } else {
            return r;
        }
    };
    const int nkt = a0.Kp / 128;

    // (the cross-attention form keeps its attention block in the kernel arguments: only the GEMM's part is a tile's own copy)
    typename std::conditional<CROSS, GemmArgs, Args>::type a = a0;
    TileSrc src;
    select(a, vb, src);
    if constexpr (INT == 0) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int p = wave + i * NW;
            if (p < XP) {
                const int r = p * 8 + (lane >> 3);
                const int c = (lane & 7) ^ ((r >> 1) & 7);
                int gm = src.m0 + r;
                gm = gm < a.M ? gm : a.M - 1;
                soff[i] = (uint32_t)gm * (uint32_t)a.Kp + c * 16;
            } else if (!W4) {
                const int r = (p - XP) * 8 + (lane >> 3);
                const int c = (lane & 7) ^ ((r >> 1) & 7);
                int gn = src.n0 + r;
                gn = gn < a.N ? gn : a.N - 1;
                soff[i] = (uint32_t)gn * (uint32_t)a.Kp + c * 16;
            } else {
                const int r = (p - XP) * 16 + (lane >> 2);
                const int c = (lane & 3) ^ ((r >> 2) & 3);
                int gn = src.n0 + r;
                gn = gn < a.N ? gn : a.N - 1;
                soff[i] = (uint32_t)gn * (uint32_t)(a.Kp >> 1) + c * 16;
            }
        }
    }

    // Prologue.  Interior forms: the issuing waves request only stage 0 before the first barrier and stage 1 right behind
    // it - the 17 pieces of stage 1 (~950 cycles of issue per wave) leave the prologue, where nothing covers them, for the
    // head of the main loop, where the partner wave owns the matrix pipe meanwhile (+0.5 % steps/s, round 5); stage 1 is
    // first read a whole k-tile later (behind the vmcnt(0) + barrier of tile 0).
    if (issuer) {
        issue(src, 0, 0);
        if (nkt > 1 && !ASYM) {
            issue(src, 1, 1);
            if (full_wave) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PPW - 1) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __builtin_amdgcn_s_barrier();
    if (ASYM && issuer && nkt > 1) issue(src, 1, 1);
    if (ts) ts[1] = __builtin_readcyclecounter();

    int4v acc[TN][TM];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[j][i] = int4v{0, 0, 0, 0};
    int4v xa[TM], xb[TM];
    WRaw w[WR];
#pragma unroll
    for (int i = 0; i < TM; ++i) xa[i] = ldx(0, 0, i);
#pragma unroll
    for (int k = 0; k < WPF; ++k) w[k % WR] = ldw(0, 0, k);

#define VQ_WIDE_STEP(X, XN, H)                                                                             \
    {                                                                                                      \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                   \
            if (H == 1 && j == BARJ && more) {                                                             \
                __builtin_amdgcn_sched_barrier(0);                                                         \
                if (STAMP && ts && kt == 1) ts[9] = __builtin_readcyclecounter(); /* arrival at the second stage barrier */ \
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                           \
                __builtin_amdgcn_s_barrier();                                                              \
                if (!late && issuer && kt + 2 < nkt) issue(src, cur, kt + 2);                              \
                __builtin_amdgcn_sched_barrier(0);                                                         \
            }                                                                                              \
            if (H == 0 && j == DMA_B && late && kt >= 1 && more) {                                         \
                __builtin_amdgcn_sched_barrier(0);                                                         \
                issue(src, nxt, kt + 1);                                                                   \
                __builtin_amdgcn_sched_barrier(0);                                                         \
            }                                                                                              \
            if (j + WPF < TN) w[(H * TN + j + WPF) % WR] = ldw(cur, H, j + WPF);                           \
            else if (H == 0) w[(H * TN + j + WPF) % WR] = ldw(cur, 1, j + WPF - TN);                       \
            else if (more) w[(H * TN + j + WPF) % WR] = ldw(nxt, 0, j + WPF - TN);                         \
            if (H == 0 || more) {                                                                          \
                if (j == TN - 2) { _Pragma("unroll") for (int i = 0; i < TM / 2; ++i) XN[i] = ldx(H == 0 ? cur : nxt, 1 - H, i); } \
                if (j == TN - 1) { _Pragma("unroll") for (int i = TM / 2; i < TM; ++i) XN[i] = ldx(H == 0 ? cur : nxt, 1 - H, i); } \
            }                                                                                              \
            const int4v wv_ = wop(w[(H * TN + j) % WR]);                                                   \
            _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                 \
                acc[j][i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv_, X[i], acc[j][i], 0, 0, 0);          \
            if (j >= TN - 2) __builtin_amdgcn_sched_group_barrier(0x100, 1 + TM / 2, 0);                   \
            else __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                        \
            __builtin_amdgcn_sched_group_barrier(0x008, TM, 0);                                            \
        }                                                                                                  \
    }
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1, nxt = cur ^ 1;
        const bool more = kt + 1 < nkt;
        VQ_WIDE_STEP(xa, xb, 0)
        VQ_WIDE_STEP(xb, xa, 1)
    }
#undef VQ_WIDE_STEP
    if (ts) ts[2] = __builtin_readcyclecounter();
    const float* gate_row = EPI == VQ_EPI_GATE_RESID ? ring_tile_gate_row<BM>(a, src.m0) : nullptr;
    // The dequantisation parameters are parked behind the epilogue slabs.  For the 256-row tile (and for W4 stages) that
    // is past the end of the ring, so they can be written while slower waves still read fragments; for the 128-row tile
    // with 128-byte weight rows the block lies INSIDE stage 1 - the stage the last k-tile occupies when their number is
    // even (K = 256, 4608): parked before every wave had left the loop it overwrote weight rows under the last MFMAs
    // (found by test_gemm_low_bit_weights).  There the global loads are issued first and the LDS writes wait for a
    // workgroup barrier.
    constexpr bool PAR_IN_RING = Cfg::PAR_IN_RING;
    const ColParams colp = ring_load_col_params<BN>(a, src.n0, tid, gate_row);
    const RowParams rowp = ring_load_row_params<BM>(a, src.m0, tid);
    if constexpr (QUANT) {
        // the consuming Linear's smoothing vector, parked in front of the parameter block: past the ring, or behind the
        // barrier that frees it (WideCfg asserts it)
        const SmoothParams smp = ring_load_smooth<BN>(a, src.n0, tid);
        if constexpr (PAR_IN_RING) __syncthreads();
        ring_park_smooth<BM, BN, WAVES_M, WAVES_N>(a, smp, smem, tid);
    } else {
        if constexpr (PAR_IN_RING) __syncthreads();
    }
    ring_park_col_params<BM, BN, WAVES_M, WAVES_N>(colp, smem, tid);
    ring_park_row_params<BM, BN, WAVES_M, WAVES_N>(rowp, smem, tid);
    __syncthreads();
    if constexpr (QUANT) {
        ring_epilogue_quant<BM, BN, WAVES_M, WAVES_N, INT != 0>(a, smem, acc, src.m0, src.n0, tid);
    } else if constexpr (CROSS) {
        ring_epilogue_cross<BM, BN, WAVES_M, WAVES_N>(a, a0.at, smem, acc, src.m0, src.n0, tid);
    } else {
        // (INT != 0: the launcher has checked what the interior epilogue needs for every tile - vq_gemm_form)
        ring_epilogue<BM, BN, WAVES_M, WAVES_N, EPI, INT != 0 && !STAMP>(a, smem, acc, src.m0, src.n0, ts, tid, gate_row != nullptr);
    }
}

template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, bool W4, bool STAMP = false, int INT = 0>
__global__ __launch_bounds__(64 * WAVES_M* WAVES_N) void gemm_i8_wide_kernel(GemmArgs a) {
    gemm_i8_wide_tile<BM, BN, WAVES_M, WAVES_N, EPI, W4, STAMP, INT>(a, blockIdx.x, threadIdx.x);
}

// the same tile with the quantizing epilogue (vq_gemm_i8_rowquant_static): 8-bit weights, general and interior form
template <int BM, int BN, int WAVES_M, int WAVES_N, int INT>
__global__ __launch_bounds__(64 * WAVES_M* WAVES_N) void gemm_i8_wide_quant_kernel(GemmQArgs a) {
    gemm_i8_wide_tile<BM, BN, WAVES_M, WAVES_N, VQ_EPI_GELU_QUANT, false, false, INT>(a, blockIdx.x, threadIdx.x);
}

// the 256 x 288 interior tile with the cross-attention epilogue (vq_gemm_i8_cross_attn): 8-bit and nibble weights
template <bool W4>
__global__ __launch_bounds__(512) void gemm_i8_cross_attn_kernel(GemmXArgs a) {
    gemm_i8_wide_tile<256, 288, 4, 2, VQ_EPI_CROSS_ATTN, W4, false, 1>(a, blockIdx.x, threadIdx.x);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// What every GEMM entry point requires of its operand images; each failing clause is a VQ_ESHAPE of the entry point.  The two
// groups are told apart because three entry points check a code width between them (and must keep refusing in that order):
//   VQ_GEMM_OPS_KP:    whole 128-byte k-lines that cover K (a stage is 128 bytes of k per row);
//   VQ_GEMM_OPS_RANGE: K <= 2^14 (|R| < 2^23: the row terms convert to fp32 exactly), and both images below 2^32 bytes -
//                      LDS-DMA offsets are 32-bit (buffer addressing).
enum { VQ_GEMM_OPS_OK = 0, VQ_GEMM_OPS_KP = 1, VQ_GEMM_OPS_RANGE = 2 };
static inline int vq_gemm_operand_check(int M, int N, int K, int Kp) {
    if (Kp % 128 != 0 || Kp < K) return VQ_GEMM_OPS_KP;
    if (K > 16384 || (long)M * Kp >= (1L << 32) || (long)N * Kp >= (1L << 32)) return VQ_GEMM_OPS_RANGE;
    return VQ_GEMM_OPS_OK;
}

// One launch of a tile kernel K: its dynamic LDS limit raised once per device, one workgroup per tile and weight set / group.
template <auto K, int BM, int BN, int WAVES_M, int WAVES_N, bool W4, class Args>
static int launch_gemm_tiles(const Args& a, hipStream_t st) {
    constexpr size_t LDS = WideCfg<BM, BN, WAVES_M, WAVES_N, W4>::LDS;
    const int MT = (a.M + BM - 1) / BM, NTl = (a.N + BN - 1) / BN;
    const int tiles = MT * NTl * (a.nbatch > 1 ? a.nbatch : a.ngroups > 1 ? a.ngroups : 1);
    if (const int rc = vq_prepare_kernel<K>((int)LDS)) return rc;
    hipLaunchKernelGGL(K, dim3(tiles), dim3(64 * WAVES_M * WAVES_N), LDS, st, a);
    return vq_check_launch();
}

// the plain kernel by epilogue kind (INT != 0: the caller has checked what the interior form needs - vq_gemm_form)
template <int BM, int BN, int WAVES_M, int WAVES_N, bool W4, int INT>
static int launch_gemm_wide(const GemmArgs& a, hipStream_t st) {
    auto go = [&](auto epi) {
        constexpr int EPI = decltype(epi)::value;
        return launch_gemm_tiles<gemm_i8_wide_kernel<BM, BN, WAVES_M, WAVES_N, EPI, W4, false, INT>, BM, BN, WAVES_M, WAVES_N, W4>(a, st);
    };
    switch (a.epilogue) {
        case VQ_EPI_NONE: return go(std::integral_constant<int, VQ_EPI_NONE>{});
        case VQ_EPI_GELU: return go(std::integral_constant<int, VQ_EPI_GELU>{});
        case VQ_EPI_GATE_RESID: return go(std::integral_constant<int, VQ_EPI_GATE_RESID>{});
        default: return go(std::integral_constant<int, VQ_EPI_RESID>{});
    }
}

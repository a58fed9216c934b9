// rowquant_shared.h - what the quantizer sources (rowquant_fast.hip, rowquant_static.hip) share: the width dispatch of
// the register-resident kernels and the half-wave reduction.
#pragma once
#include "vq_common.h"

// ---- host side: the dispatch the register-resident quantizers share -----------------
// The half-wave kernels are compiled for rows of C = 128 * NIT channels, NIT in {6, 8, 9, 10}: the hidden sizes 768, 1024,
// 1152 and 1280.  (The sources used to spell this set in two ways; the second, C % 128 == 0 && 768 <= C <= 1280, also let
// 896 through to a width switch that had no kernel for it and fell back - the assert below pins exactly that.)
constexpr bool rq_block_width(int C) { return C % 128 == 0 && (C / 128 == 6 || C / 128 == 8 || C / 128 == 9 || C / 128 == 10); }
constexpr bool rq_block_width_is_both_spellings() {
    for (int C = 0; C <= 8192; ++C) {
        const bool named = C == 1152 || C == 1024 || C == 1280 || C == 768;
        const bool range = C % 128 == 0 && C >= 768 && C <= 1280;
        if (rq_block_width(C) != named || rq_block_width(C) != (range && C != 896)) return false;
    }
    return true;
}
static_assert(rq_block_width_is_both_spellings(), "one predicate for the widths of the half-wave kernels");

// f(std::integral_constant<int, NIT>) and true at a block width, false (nothing launched) at any other C
template <class F>
static bool vq_dispatch_nit(int C, F&& f) {
    const int nit = rq_block_width(C) ? C / 128 : 0;
    switch (nit) {
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 9: f(std::integral_constant<int, 9>{}); break;
        case 10: f(std::integral_constant<int, 10>{}); break;
        default: return false;
    }
    return true;
}

// f(std::integral_constant<int, MAXCH>): the 16-byte chunks per lane the one-row-per-wave kernels hold for a padded row of Kp
template <class F>
static void vq_dispatch_maxch(int Kp, F&& f) {
    if (Kp <= 512) f(std::integral_constant<int, 1>{});
    else if (Kp <= 1536) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 9>{});
}

template <class F>
static void vq_dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// reduction over the 32 lanes of a half-wave (two rows per wave; ``hi`` = this lane is in the upper half): DPP inside
// each row of 16 lanes, then the two rows of the half through v_readlane
#define RQH_REDUCE2(T_, OP_, v_)                                                                        \
    {                                                                                                   \
        VQ_DPP_STEP(T_, OP_, v_, 0xB1);                                                                 \
        VQ_DPP_STEP(T_, OP_, v_, 0x4E);                                                                 \
        VQ_DPP_STEP(T_, OP_, v_, 0x141);                                                                \
        VQ_DPP_STEP(T_, OP_, v_, 0x140);                                                                \
        const int b_ = __builtin_bit_cast(int, v_);                                                     \
        const T_ r0_ = __builtin_bit_cast(T_, __builtin_amdgcn_readlane(b_, 0));                        \
        const T_ r1_ = __builtin_bit_cast(T_, __builtin_amdgcn_readlane(b_, 16));                       \
        const T_ r2_ = __builtin_bit_cast(T_, __builtin_amdgcn_readlane(b_, 32));                       \
        const T_ r3_ = __builtin_bit_cast(T_, __builtin_amdgcn_readlane(b_, 48));                       \
        v_ = hi ? OP_(r2_, r3_) : OP_(r0_, r1_);                                                        \
    }

// one kernel-uniform branch on the code width around a whole store loop: SAT8_ (8-bit codes) = v_cvt_pk_u8_f32 saturates to
// [0, 255] by itself, other widths clamp first (as a per-element select it cost a v_med3 + v_cndmask per code)
#define RQ_BY_WIDTH(qmax_, ...)                                       \
    if ((qmax_) == 255.0f) {                                          \
        constexpr bool SAT8_ = true;                                  \
        __VA_ARGS__                                                   \
    } else {                                                          \
        constexpr bool SAT8_ = false;                                 \
        __VA_ARGS__                                                   \
    }

// Copyright (c) Flashy-AMD authors.
// Shared host side of the 8-wave deep-pipeline conv family for gfx950:
// k_conv_fwd8 / k_conv1x1_mloop (conv_fwd8.hip), k_conv_dedup
// (conv_dedup.hip) and k_conv_dgrad8 with its SCAT2, PAR2 and split-K variants
// (conv_dgrad8.hip): the out-of-range sentinel, the family's off switch,
// the BN choice, the runtime -> template dispatch helper and the prototypes
// of every plan and launcher.
//
// The device bodies stay in their kernel files on purpose.  Moving the tile
// loop and the epilogues into shared __device__ helpers was tried and gave
// bitwise-equal results but not the same machine code (register allocation
// and the order of address ops in the MFMA loop shifted, and the 14x14 3x3
// layer measured about 1% slower), so the kernels keep their own text until
// a form is found that compiles to the same code.
#pragma once

#include <cstdlib>
#include <type_traits>

#include "conv_common.h"

// Out-of-range sentinel: a buffer-load voffset far past any real tensor
// (tensors routed to this family are < 2^31 - 2^28 bytes); the buffer
// descriptor's bounds check then returns hardware zeros, so im2col padding
// and tile tails need no branch in the loops.
constexpr unsigned kOobSentinel = 0xF0000000u;

// --- host side ---------------------------------------------------------------

// FLASHY_NO_FWD8=1 switches the whole family off (A/B against the 4-wave
// kernels).
inline bool conv8_disabled() {
    static const bool disabled = [] {
        const char* e = getenv("FLASHY_NO_FWD8");
        return e && e[0] == '1';
    }();
    return disabled;
}

// BN=128 when the channel count allows it and the grid still has
// `threshold` blocks, else BN=64 under the same floor, else no 8-wave tile.
inline bool pick_bn8(int tiles_m, int channels, int threshold, int* bn) {
    if (channels % 128 == 0 &&
        (int64_t)tiles_m * (channels / 128) >= threshold) {
        *bn = 128;
        return true;
    }
    if ((int64_t)tiles_m * (channels / 64) >= threshold) {
        *bn = 64;
        return true;
    }
    return false;
}

// Runtime (bn, flag) -> template arguments: f(BN, FLAG) receives two
// integral_constants, e.g. k<decltype(BN)::value, decltype(FLAG)::value>.
template <class F>
inline void dispatch8(int bn, bool flag, F&& f) {
    using B128 = std::integral_constant<int, 128>;
    using B64 = std::integral_constant<int, 64>;
    if (bn == 128) {
        if (flag) f(B128(), std::true_type());
        else f(B128(), std::false_type());
    } else {
        if (flag) f(B64(), std::true_type());
        else f(B64(), std::false_type());
    }
}

// Stride-2 dgrad forms (conv_dgrad_s2_plan; conv_dgrad.hip): 8-wave parity
// classes (k_conv_dgrad8 PAR2, tile = BN), 4-wave parity classes
// (k_conv_dgrad_s2, tile = BM), 1x1 quarter GEMM + sibling zeros (SCAT2,
// tile = BN), or none of them (generic zero-filled kernel, split-K allowed).
enum DgradS2Form {
    DGRAD_S2_NONE = 0,
    DGRAD_S2_PAR8 = 1,
    DGRAD_S2_PAR4 = 2,
    DGRAD_S2_SCAT2 = 3,
};
// Block floor of the 8-wave parity form, all four classes counted
// (profiles/r05a_dgrad_s2_sweep.txt: it wins from 208 blocks up, the 4-wave
// 32-row tile below)
constexpr int kPar8Floor = 208;

// Plans return grid.x (0 = not eligible) and are decided purely from the
// dims; launchers take what the plan returned.
extern "C" {
int conv_fwd8_plan(ConvDims d, int* bn_out);
void launch_conv_fwd8(const void* x, const void* w, void* y, ConvDims d,
                      int relu, void* bn_ws, int bn, int mtiles,
                      hipStream_t stream);
void launch_conv_fwd8_splitk(const void* x, const void* w, void* ws,
                             ConvDims d, int bn, int mtiles, int spz,
                             int zeff, hipStream_t stream);
int conv1x1_mloop_plan(ConvDims d, int* bn_out, int* gridx_out);
void launch_conv1x1_mloop(const void* x, const void* w, void* y, ConvDims d,
                          int relu, void* bn_ws, int bn, int gridx,
                          int mtiles, hipStream_t stream);
int conv_dedup_plan(ConvDims d, int* bn_out, int* tpi_out, int* rows_out,
                    int* elems_out);
void launch_conv_dedup(const void* x, const void* w, void* y, ConvDims d,
                       int relu, void* bn_ws, int bn, int tpi, int rows,
                       int lds_elems, hipStream_t stream);
int conv_dgrad8_plan(ConvDims d, int* bn_out);
void launch_conv_dgrad8(const void* dout, const void* w_rsck, void* dx,
                        ConvDims d, int bn, int mtiles, hipStream_t stream);
int conv_dgrad8_s2_plan(ConvDims d, int* bn_out);
int conv_dgrad8_s2_mtiles(ConvDims d);
int conv_dgrad8_par2_mtiles(ConvDims d);
void launch_conv_dgrad8_par2(const void* dout, const void* w_rsck, void* dx,
                             ConvDims d, int bn, int mtiles,
                             hipStream_t stream);
int conv_dgrad_s2_plan(ConvDims d, int* tile_out);
int launch_conv_dgrad_s2_form(const void* dout, const void* w_rsck, void* dx,
                              ConvDims d, int form, int tile,
                              hipStream_t stream);
void launch_conv_dgrad8_s2(const void* dout, const void* w_rsck, void* dx,
                           ConvDims d, int bn, int mtiles,
                           hipStream_t stream);
void launch_conv_dgrad8_splitk(const void* dout, const void* w_rsck,
                               void* ws, ConvDims d, int bn, int mtiles,
                               int spz, int zeff, hipStream_t stream);
}

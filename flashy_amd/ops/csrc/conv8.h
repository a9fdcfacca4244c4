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

// --- the tile plan -------------------------------------------------------------
// The family has two row tiles: BM=256 (8 m-fragments per wave) and BM=128
// (4 per wave, half the A stage, 4 LDS buffers at either BN).  Every plan,
// eligibility query and launcher takes its (bm, bn) from the two functions
// below, and Python asks them through the bindings.
struct Tile8 {
    int bm, bn;
};

inline int64_t blocks8(int64_t rows, int channels, Tile8 t) {
    return (rows + t.bm - 1) / t.bm * (channels / t.bn);
}

// Block floors: single pass, and slices counted (split-K launchers).
constexpr int kFloor8 = 160;
constexpr int kSplitkFloor8 = 120;

// Single pass: 256 rows wherever the grid (x `classes` for the parity form)
// keeps `floor` blocks, BN=128 before BN=64; else no 8-wave tile.  The
// 128-row tile has no single-pass route: it measured faster on the short
// stride-2 / 1x1 forwards (profiles/README.md, r08a), but those convs feed
// BatchNorm from the split-K combine's statistics of the rounded values
// today, and the epilogue's unrounded ones moved a training step's results
// well past rounding (r08a: loss 6.8e-4), so the route was withdrawn.
inline bool pick_tile8(int64_t rows, int channels, int floor, Tile8* t,
                       int classes = 1) {
    for (int bn : {128, 64}) {
        const Tile8 c = {256, bn};
        if (channels % bn == 0 &&
            blocks8(rows, channels, c) * classes >= floor) {
            *t = c;
            return true;
        }
    }
    return false;
}

// Split-K (one fp32 slab per slice).  BN is the widest the channel count
// allows.  256 rows from kRows128Below blocks up; below that the grid is so
// short of the 256 CUs that 128-row tiles win at the same split (r08a: 19.5
// against 32.8 us at 16 blocks, 23.1 against 30.1 at 32; at 52 the two tie
// and nothing moves): twice the blocks per slice.
constexpr int kRows128Below = 33;
inline Tile8 splitk_tile8(int64_t rows, int channels) {
    Tile8 t = {256, channels % 128 == 0 ? 128 : 64};
    if (blocks8(rows, channels, t) < kRows128Below) t.bm = 128;
    return t;
}
// Rows per block that ops._underfill_zn counts when it sizes the split.  It
// stays 256 whatever tile runs: fewer slices for the 128-row tile measured
// 1.5 us faster (8x8x256 3x3, 3 slices against 4) but regroup the fp32 sums,
// which moved a training step's weights by up to 1.4e-3 (r08a) where earlier
// reorderings moved them 1.7e-4.  With the split kept, every slice sums the
// same stages in the same order and the results are the parent's.
constexpr int kSplitSizingRows = 256;

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

// The same with the row tile in front: f(BM, BN, FLAG).
template <class F>
inline void dispatch8(Tile8 t, bool flag, F&& f) {
    using M256 = std::integral_constant<int, 256>;
    using M128 = std::integral_constant<int, 128>;
    dispatch8(t.bn, flag, [&](auto BN, auto FLAG) {
        if (t.bm == 128) f(M128(), BN, FLAG);
        else f(M256(), BN, FLAG);
    });
}

// Stride-2 dgrad forms (conv_dgrad_s2_plan; conv_dgrad.hip): 8-wave parity
// classes (k_conv_dgrad8 PAR2, tile = BN; PAR8 has 256-row tiles, PAR8_M128
// 128-row ones), 4-wave parity classes (k_conv_dgrad_s2, tile = BM), 1x1
// quarter GEMM + sibling zeros (SCAT2, tile = BN), or none of them (generic
// zero-filled kernel, split-K allowed).
enum DgradS2Form {
    DGRAD_S2_NONE = 0,
    DGRAD_S2_PAR8 = 1,
    DGRAD_S2_PAR4 = 2,
    DGRAD_S2_SCAT2 = 3,
    DGRAD_S2_PAR8_M128 = 4,
};
// Block floor of the 8-wave parity form, all four classes counted
// (profiles/r05a_dgrad_s2_sweep.txt: it wins from 208 blocks up, the 4-wave
// 32-row tile below)
constexpr int kPar8Floor = 208;

// Plans return grid.x (0 = not eligible) and are decided purely from the
// dims; launchers take what the plan returned.
extern "C" {
int conv_fwd8_plan(ConvDims d, Tile8* tile_out);
void launch_conv_fwd8(const void* x, const void* w, void* y, ConvDims d,
                      int relu, void* bn_ws, Tile8 tile, int mtiles,
                      hipStream_t stream);
void launch_conv_fwd8_splitk(const void* x, const void* w, void* ws,
                             ConvDims d, Tile8 tile, int mtiles, int spz,
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
int conv_dgrad8_plan(ConvDims d, Tile8* tile_out);
void launch_conv_dgrad8(const void* dout, const void* w_rsck, void* dx,
                        ConvDims d, Tile8 tile, int mtiles,
                        hipStream_t stream);
int conv_dgrad8_s2_plan(ConvDims d, int* bn_out);
int conv_dgrad8_s2_mtiles(ConvDims d);
int conv_dgrad8_par2_mtiles(ConvDims d, int bm);
void launch_conv_dgrad8_par2(const void* dout, const void* w_rsck, void* dx,
                             ConvDims d, Tile8 tile, int mtiles,
                             hipStream_t stream);
int conv_dgrad_s2_plan(ConvDims d, int* tile_out);
int launch_conv_dgrad_s2_form(const void* dout, const void* w_rsck, void* dx,
                              ConvDims d, int form, int tile,
                              hipStream_t stream);
void launch_conv_dgrad8_s2(const void* dout, const void* w_rsck, void* dx,
                           ConvDims d, int bn, int mtiles,
                           hipStream_t stream);
void launch_conv_dgrad8_splitk(const void* dout, const void* w_rsck,
                               void* ws, ConvDims d, Tile8 tile, int mtiles,
                               int spz, int zeff, hipStream_t stream);
// One 8-wave kernel named by the caller (tests, scripts/splitk_sweep.py):
// fwd8 or stride-1/-2 generic dgrad8 at tile (bm, bn); spz == 0 is a single
// pass into the bf16 `out` (forward: BN partials to `bn_ws` unless null),
// spz > 0 writes split-K slices of spz stages into the fp32 slab `out`.
// Returns the partials' msplit (forward single pass), else 1; 0 when the
// shape or tile cannot run.
int launch_conv8_form(int dgrad, const void* a, const void* w, void* out,
                      void* bn_ws, ConvDims d, Tile8 tile, int spz,
                      hipStream_t stream);
}

// Copyright (c) Flashy-AMD authors.
// NHWC bf16 DEPTHWISE k x k convolution (k in {3, 5, 7}, pad k / 2, stride 1
// or 2, channel multiplier 1) for gfx950: forward, backward-data and
// backward-weights for any C % 8 == 0.  Weights are [C][k][k][1].
// dwconv_plan() below is the only place that decides.
//
// There is no reduction over input channels, so there is nothing to feed a
// matrix instruction: per output element the work is k*k fp32 FMAs against 4
// bytes of traffic.  The kernels are built around traffic and LDS reuse: a
// block owns a rectangle of TR x TW output pixels of one image by a SLAB of up
// to 64 channels (the last slab of a width that is no multiple of 64 is
// partial; its surplus lanes stage zeros and compute nothing).  The input slab
// with its halo is staged ONCE in 16-byte lanes, zeros outside the image, and
// every tap is served from LDS.  There is no operand-preparation launch: the
// block gathers its slab's weights (at most 64 ch x 49 taps) strided from the
// [C][k*k] bf16 tensor and parks them tap-major, as fp32, behind the slab, so
// a lane's 8 channels of one tap are 32 contiguous bytes.
//
// Thread layout (256 threads): lane & 7 is the channel OCTET (8 channels, 16
// bytes), so 8 neighbouring lanes cover a pixel's 128 contiguous bytes in
// global memory and in LDS; tid >> 3 is one of 32 SLOTS.
//
// Forward (dw_body): a slot is an output column of the tile (TW <= 16) and a
// row group (RG = 32 / TW of them, RPG rows each).  A thread walks DOWN its
// column with a sliding window of NA = ceil(KR / stride) output-row
// accumulators (8 fp32 each): every staged input row is read once per tap
// column (one ds_read_b128), unpacked once, and fed to all the output rows in
// flight; after each input-row group the oldest accumulator is complete, is
// rounded once to bf16 and stored as 16 bytes, and the window shifts.  With at
// most 9 taps the weights sit in registers (72 VGPRs at 3x3); above that they
// are read from LDS, 32 bytes per lane and tap, the same address in every
// lane of equal octet (a broadcast).  The window costs 8 * (NA - 1) register
// moves per row group; against 8 * KR * KC FMAs that was accepted.
//
// LDS slab: one 128-byte row per input pixel, NO padding between pixels.  A
// 16-lane group of a ds_read_b128 is two neighbouring slots x 8 octets: at
// stride 1 two adjacent pixels of one tap, 256 contiguous bytes = all 64
// banks once.  At stride 2 neighbouring output columns are two input columns
// apart (64 dwords: the same banks, a 2-way conflict), so the slab keeps the
// even and the odd staged columns in two halves of each row (the layout of
// conv_group.hip) and a tap reads adjacent entries again.  A group that
// straddles two row groups breaks the sequence once.  Unmeasured: that b128
// reads are resolved per 16 lanes (the family's working assumption,
// conv_common.h), the cost of the straddle, and the cost of the broadcast
// weight reads.
//
// Backward-data at stride 1 is the forward kernel on dy with the taps
// flipped (only the gather of the weights changes).  At stride 2 it is split
// by the parity of (h, w) as conv_dgrad8.hip documents: dx[2i+ph][2j+pw] only
// meets taps r = (ph + pad) % 2 + 2a, likewise s, so a class is a stride-1
// correlation of dy with an NR x NS sub-kernel (1/2, 3/2, 3/4 rows at k = 3,
// 5, 7 for ph = 0/1) and runs the same dw_body<NR, NS, 1>.  No multiply meets
// a structural zero, no zero-filled dy exists, every dx element is written by
// exactly one class.  grid.z is the class; odd H / W shorten the odd classes,
// whose surplus blocks leave before the first barrier.
//
// Backward-weights: dw[c][r][s] = sum_m dy[m][c] * x[m @ (r, s)][c].  A block
// owns a slab and a range of tiles; per tile it stages the x slab (forward's
// layout) and the dy tile.  A slot is a TAP ROW r and one of CW = 32 / k
// column lanes, so a thread keeps only k x 8 accumulators (56 at 7x7, where
// 49 x 8 would spill) and walks the tile's pixels in column lanes.  Pixels
// outside the image are skipped, so padding never multiplies.  At the end the
// threads fold through LDS in column-lane order and the block writes one fp32
// [slab][k*k] slice of a workspace; k_dwconv_wgrad_combine sums the slices in
// split order and adds into dw.  The split count comes from the dims alone:
// no atomics, no spin-wait, no last-block fan-in, bitwise repeatable.

#include "conv_common.h"

#define DW_THREADS 256
#define DW_SLOTS 32                  // DW_THREADS / 8 octets
#define DW_MAXTW 16                  // output columns per tile
#define DW_SLAB_BYTES (40 * 1024)    // forward slab budget (weights come on top)
#define DW_WG_BYTES (48 * 1024)      // wgrad: x slab + dy tile

struct DTile {
    int TR, TW;     // output rows / columns per tile
    int RG, RPG;    // forward: row groups per tile, rows per group
    int rt, ct;     // tiles per image along rows / columns
};

static inline int dw_sr(int S, int KR, int TR) { return S * (TR - 1) + KR; }
static inline int dw_sw(int S, int KC, int TW) {
    const int swc = S * (TW - 1) + KC;
    return S == 2 ? 2 * ((swc + 1) / 2) : swc;
}

// Tile of an Hc x Wc output grid read through a KR x KC window at stride S.
static DTile dw_tile(int S, int KR, int KC, int Hc, int Wc, bool with_dy,
                     int budget) {
    DTile g;
    const int parts = (Wc + DW_MAXTW - 1) / DW_MAXTW;
    g.TW = (Wc + parts - 1) / parts;
    g.TR = Hc;
    while (g.TR > 1 &&
           (dw_sr(S, KR, g.TR) * dw_sw(S, KC, g.TW) +
            (with_dy ? g.TR * g.TW : 0)) * 128 > budget)
        --g.TR;
    g.RG = DW_SLOTS / g.TW;
    if (g.RG > g.TR) g.RG = g.TR;
    g.RPG = (g.TR + g.RG - 1) / g.RG;
    g.rt = (Hc + g.TR - 1) / g.TR;
    g.ct = (Wc + g.TW - 1) / g.TW;
    return g;
}

static bool dw_ok(const ConvDims& d) {
    if (d.C != d.K || d.C < 8 || d.C % 8 != 0) return false;
    if (d.R != d.S || (d.R != 3 && d.R != 5 && d.R != 7)) return false;
    if (d.pad != d.R / 2) return false;
    if (d.stride != 1 && d.stride != 2) return false;
    if (d.N < 1 || d.H < 1 || d.W < 1) return false;
    return d.Ho == (d.H - 1) / d.stride + 1 && d.Wo == (d.W - 1) / d.stride + 1;
}

static void dw_wgrad_split(const ConvDims& d, DTile* g, int* ntiles, int* tps,
                           int* nsplit) {
    *g = dw_tile(d.stride, d.R, d.R, d.Ho, d.Wo, true, DW_WG_BYTES);
    *ntiles = d.N * g->rt * g->ct;
    const int slabs = (d.C + 63) / 64;
    int want = (512 + slabs - 1) / slabs;    // two blocks per CU of 256
    if (want > *ntiles) want = *ntiles;
    *tps = (*ntiles + want - 1) / want;
    *nsplit = (*ntiles + *tps - 1) / *tps;
}

// Dims-only plan: 1 where the depthwise path serves `d` (d.C == d.K is the
// channel count, groups == d.C is implied), else 0; *wgrad_splits is the
// number of fp32 slices dwconv_wgrad writes.
extern "C" int dwconv_plan(ConvDims d, int* wgrad_splits) {
    *wgrad_splits = 0;
    if (!dw_ok(d)) return 0;
    DTile g; int ntiles, tps;
    dw_wgrad_split(d, &g, &ntiles, &tps, wgrad_splits);
    return 1;
}

// Everything up to the matching pop is compiled without packed fp32 math (see
// fused_optim.hip for why); a function under this attribute can only inline
// always_inline callees, hence dw_barrier and the plain helpers below.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// what __syncthreads expands to
__device__ __forceinline__ void dw_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int dw_min(int a, int b) { return a < b ? a : b; }

// LDS pixel index of staged row sr, staged column sc
template <int S>
__device__ __forceinline__ int dw_pos(int sr, int sc, int SW, int HALF) {
    if (S == 2) return sr * SW + (sc & 1) * HALF + (sc >> 1);
    return sr * SW + sc;
}

// Stage rows [ih0, ih0+SR) x columns [iw0, iw0+SWc) of the slab at ch0 of
// image n, zeros outside the image and in the octets a partial slab lacks.
template <int S>
__device__ __forceinline__ void dw_stage(const uint16_t* __restrict__ in,
                                         uint16_t* lds, int n, int Hin,
                                         int Win, int C, int ch0, int noct,
                                         int ih0, int iw0, int SR, int SWc,
                                         int SW, int HALF) {
    const int oct = threadIdx.x & 7;
    const int count = SR * SWc;
    for (int pix = threadIdx.x >> 3; pix < count; pix += DW_SLOTS) {
        const int sr = pix / SWc, sc = pix - sr * SWc;
        const int ih = ih0 + sr, iw = iw0 + sc;
        short8 v = {};
        if (oct < noct && ih >= 0 && ih < Hin && iw >= 0 && iw < Win)
            v = *reinterpret_cast<const short8*>(
                in + (((int64_t)n * Hin + ih) * Win + iw) * C + ch0 + oct * 8);
        *reinterpret_cast<short8*>(
            &lds[dw_pos<S>(sr, sc, SW, HALF) * 64 + oct * 8]) = v;
    }
}

// One tile of a KR x KC correlation at stride S: out[omul*(r0+j)+hadd]
// [omul*(c0+t)+wadd] = sum_{a,b} in[ih0 + S*j + a][iw0 + S*t + b] * wl[a][b],
// where wl[a][b] is tap (rb + rstep*a, sb + sstep*b) of the KS x KS kernel.
template <int KR, int KC, int S>
__device__ __forceinline__ void dw_body(
    const uint16_t* __restrict__ in, const uint16_t* __restrict__ w16,
    uint16_t* __restrict__ out, uint16_t* lds, int n, int Hin, int Win,
    int Hout, int Wout, int C, int Hc, int Wc, int r0, int c0, int ih0,
    int iw0, int omul, int hadd, int wadd, int KS, int rb, int rstep, int sb,
    int sstep, const DTile& g) {
    constexpr int NA = (KR + S - 1) / S;      // output rows in flight
    constexpr bool WREG = KR * KC <= 9;       // weights in registers
    const int SR = S * (g.TR - 1) + KR;
    const int SWc = S * (g.TW - 1) + KC;
    const int HALF = S == 2 ? (SWc + 1) / 2 : 0;
    const int SW = S == 2 ? 2 * HALF : SWc;
    const int ch0 = blockIdx.y * 64;
    const int noct = dw_min(8, (C - ch0) >> 3);
    const int tid = threadIdx.x, oct = tid & 7, slot = tid >> 3;

    dw_stage<S>(in, lds, n, Hin, Win, C, ch0, noct, ih0, iw0, SR, SWc, SW, HALF);
    // the slab's weights, tap-major fp32 [KR*KC][64] behind the slab: the
    // global reads are strided by k*k elements, the LDS writes are not
    float* const wl = reinterpret_cast<float*>(lds + SR * SW * 64);
    for (int idx = tid; idx < KR * KC * 64; idx += DW_THREADS) {
        const int t = idx >> 6, ch = idx & 63;
        const int a = t / KC, b = t - a * KC;
        float v = 0.f;
        if (ch0 + ch < C)
            v = bf16_to_f32(w16[(int64_t)(ch0 + ch) * KS * KS +
                                (rb + rstep * a) * KS + sb + sstep * b]);
        wl[idx] = v;
    }
    dw_barrier();

    const int rg = slot / g.TW, tc = slot - rg * g.TW;
    const int jlo = rg * g.RPG;
    const int jhi = dw_min(dw_min(jlo + g.RPG, g.TR), Hc - r0);
    if (rg >= g.RG || oct >= noct || c0 + tc >= Wc || jlo >= jhi) return;

    float wr[WREG ? KR * KC : 1][8];
    if (WREG) {
#pragma unroll
        for (int t = 0; t < KR * KC; ++t) {
            const floatx4 w0 = *reinterpret_cast<const floatx4*>(&wl[t * 64 + oct * 8]);
            const floatx4 w1 = *reinterpret_cast<const floatx4*>(&wl[t * 64 + oct * 8 + 4]);
#pragma unroll
            for (int c = 0; c < 4; ++c) { wr[t][c] = w0[c]; wr[t][4 + c] = w1[c]; }
        }
    }
    float acc[NA][8];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[i][c] = 0.f;

    const int wout = omul * (c0 + tc) + wadd;
    // group q holds staged rows S*q .. S*q+S-1; acc[i] is output row
    // q - (NA-1) + i and meets tap row S*(NA-1-i) + u of staged row S*q + u
    for (int q = jlo; q <= jhi - 1 + NA - 1; ++q) {
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int lr = S * q + u;
            if (lr >= SR) continue;   // stride 2: one row past the last tap
#pragma unroll
            for (int s = 0; s < KC; ++s) {
                const short8 v = *reinterpret_cast<const short8*>(
                    &lds[dw_pos<S>(lr, S * tc + s, SW, HALF) * 64 + oct * 8]);
                float f[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) f[c] = bf16_to_f32((uint16_t)v[c]);
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const int r = S * (NA - 1 - i) + u;
                    const int j = q - (NA - 1) + i;
                    if (r < KR && j >= jlo && j < jhi) {
                        if (WREG) {
#pragma unroll
                            for (int c = 0; c < 8; ++c)
                                acc[i][c] = __fmaf_rn(f[c], wr[WREG ? r * KC + s : 0][c],
                                                      acc[i][c]);
                        } else {
                            const float* wp = &wl[(r * KC + s) * 64 + oct * 8];
                            const floatx4 w0 = *reinterpret_cast<const floatx4*>(wp);
                            const floatx4 w1 = *reinterpret_cast<const floatx4*>(wp + 4);
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                acc[i][c] = __fmaf_rn(f[c], w0[c], acc[i][c]);
                                acc[i][4 + c] = __fmaf_rn(f[4 + c], w1[c], acc[i][4 + c]);
                            }
                        }
                    }
                }
            }
        }
        const int j = q - (NA - 1);
        if (j >= jlo) {       // its last tap row was in this group
            short8 o;
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] = (short)f32_to_bf16(acc[0][c]);
            const int hout = omul * (r0 + j) + hadd;
            *reinterpret_cast<short8*>(
                out + (((int64_t)n * Hout + hout) * Wout + wout) * C + ch0 +
                oct * 8) = o;
        }
#pragma unroll
        for (int i = 0; i + 1 < NA; ++i)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[i][c] = acc[i + 1][c];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[NA - 1][c] = 0.f;
    }
}

// in: [N][Hin][Win][C], out: [N][Hout][Wout][C].  Forward, and with `flip`
// the stride-1 backward-data (in = dy, out = dx).
template <int KS, int STRIDE>
__global__ void __launch_bounds__(DW_THREADS)
k_dwconv_fwd(const uint16_t* __restrict__ in, const uint16_t* __restrict__ w16,
             uint16_t* __restrict__ out, int Hin, int Win, int Hout, int Wout,
             int C, int flip, DTile g) {
    extern __shared__ __attribute__((aligned(16))) uint16_t dw_lds[];
    int tile = blockIdx.x;
    const int c0 = (tile % g.ct) * g.TW; tile /= g.ct;
    const int r0 = (tile % g.rt) * g.TR;
    const int n = tile / g.rt;
    dw_body<KS, KS, STRIDE>(in, w16, out, dw_lds, n, Hin, Win, Hout, Wout, C,
                            Hout, Wout, r0, c0, STRIDE * r0 - KS / 2,
                            STRIDE * c0 - KS / 2, 1, 0, 0, KS,
                            flip ? KS - 1 : 0, flip ? -1 : 1,
                            flip ? KS - 1 : 0, flip ? -1 : 1, g);
}

// Stride-2 backward-data: in = dy [N][Ho][Wo][C], out = dx [N][H][W][C],
// blockIdx.z = parity class (ph, pw); the tile grid is that of the largest
// class.  Class rows i of parity ph read dy rows i + bh - (NR-1) + a with tap
// row par + 2*(NR-1-a), par = (ph + pad) & 1, bh = (ph + pad - par) / 2.
template <int KS>
__global__ void __launch_bounds__(DW_THREADS)
k_dwconv_dgrad_s2(const uint16_t* __restrict__ dy,
                  const uint16_t* __restrict__ w16, uint16_t* __restrict__ dx,
                  int Ho, int Wo, int H, int W, int C, DTile g) {
    extern __shared__ __attribute__((aligned(16))) uint16_t dw_lds[];
    constexpr int P = KS / 2;
    constexpr int PAR0 = P & 1, PAR1 = (P + 1) & 1;         // ph = 0 / 1
    constexpr int N0 = (KS - PAR0 + 1) / 2, N1 = (KS - PAR1 + 1) / 2;
    constexpr int B0 = (P - PAR0) / 2, B1 = (1 + P - PAR1) / 2;
    const int ph = blockIdx.z >> 1, pw = blockIdx.z & 1;
    const int Hc = (H - ph + 1) >> 1, Wc = (W - pw + 1) >> 1;
    int tile = blockIdx.x;
    const int c0 = (tile % g.ct) * g.TW; tile /= g.ct;
    const int r0 = (tile % g.rt) * g.TR;
    const int n = tile / g.rt;
    if (r0 >= Hc || c0 >= Wc) return;   // block-uniform: a shorter odd class
    const int nr = ph ? N1 : N0, ns = pw ? N1 : N0;
    const int ih0 = r0 + (ph ? B1 : B0) - (nr - 1);
    const int iw0 = c0 + (pw ? B1 : B0) - (ns - 1);
    const int rb = (ph ? PAR1 : PAR0) + 2 * (nr - 1);
    const int sb = (pw ? PAR1 : PAR0) + 2 * (ns - 1);
#define DW_CLASS(NR, NS)                                                      \
    dw_body<NR, NS, 1>(dy, w16, dx, dw_lds, n, Ho, Wo, H, W, C, Hc, Wc, r0,   \
                       c0, ih0, iw0, 2, ph, pw, KS, rb, -2, sb, -2, g)
    if (ph && pw) DW_CLASS(N1, N1);
    else if (ph) DW_CLASS(N1, N0);
    else if (pw) DW_CLASS(N0, N1);
    else DW_CLASS(N0, N0);
#undef DW_CLASS
}

// ws: fp32 [nsplit][C][KS*KS]; block (x = m-split, y = slab) writes its slice
template <int KS, int S>
__global__ void __launch_bounds__(DW_THREADS)
k_dwconv_wgrad(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy,
               float* __restrict__ ws, int H, int W, int Ho, int Wo, int C,
               DTile g, int ntiles, int tps) {
    extern __shared__ __attribute__((aligned(16))) uint16_t dw_lds[];
    constexpr int KK = KS * KS;
    constexpr int CW = DW_SLOTS / KS;         // column lanes per tap row
    const int SR = S * (g.TR - 1) + KS;
    const int SWc = S * (g.TW - 1) + KS;
    const int HALF = S == 2 ? (SWc + 1) / 2 : 0;
    const int SW = S == 2 ? 2 * HALF : SWc;
    uint16_t* const xs = dw_lds;
    uint16_t* const dys = dw_lds + SR * SW * 64;
    const int ch0 = blockIdx.y * 64;
    const int noct = dw_min(8, (C - ch0) >> 3);
    const int tid = threadIdx.x, oct = tid & 7, slot = tid >> 3;
    const int r = slot / CW, cs = slot - r * CW;
    const bool active = r < KS && oct < noct;
    float acc[KS][8];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[s][c] = 0.f;

    const int t_end = dw_min(ntiles, ((int)blockIdx.x + 1) * tps);
    for (int tile = blockIdx.x * tps; tile < t_end; ++tile) {
        int tt = tile;
        const int c0 = (tt % g.ct) * g.TW; tt /= g.ct;
        const int r0 = (tt % g.rt) * g.TR;
        const int n = tt / g.rt;
        dw_barrier();    // the previous tile's reads are done
        dw_stage<S>(x, xs, n, H, W, C, ch0, noct, S * r0 - KS / 2,
                    S * c0 - KS / 2, SR, SWc, SW, HALF);
        dw_stage<1>(dy, dys, n, Ho, Wo, C, ch0, noct, r0, c0, g.TR, g.TW,
                    g.TW, 0);
        dw_barrier();
        if (!active) continue;
        const int jn = dw_min(g.TR, Ho - r0), tn = dw_min(g.TW, Wo - c0);
        for (int j = 0; j < jn; ++j)
            for (int tc = cs; tc < tn; tc += CW) {
                const short8 dv = *reinterpret_cast<const short8*>(
                    &dys[(j * g.TW + tc) * 64 + oct * 8]);
                float df[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) df[c] = bf16_to_f32((uint16_t)dv[c]);
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const short8 v = *reinterpret_cast<const short8*>(
                        &xs[dw_pos<S>(S * j + r, S * tc + s, SW, HALF) * 64 +
                            oct * 8]);
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        acc[s][c] = __fmaf_rn(df[c], bf16_to_f32((uint16_t)v[c]),
                                              acc[s][c]);
                }
            }
    }
    // fold the CW column lanes of each (tap, channel) in lane order
    float* const red = reinterpret_cast<float*>(dw_lds);   // [CW][KK][64]
    dw_barrier();
    if (r < KS) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int c = 0; c < 8; ++c)
                red[(cs * KK + r * KS + s) * 64 + oct * 8 + c] = acc[s][c];
    }
    dw_barrier();
    float* const slice = ws + (int64_t)blockIdx.x * C * KK;
    for (int idx = tid; idx < KK * 64; idx += DW_THREADS) {
        const int t = idx >> 6, ch = idx & 63;
        float sum = red[idx];
        for (int l = 1; l < CW; ++l) sum += red[l * KK * 64 + idx];
        if (ch0 + ch < C) slice[(int64_t)(ch0 + ch) * KK + t] = sum;
    }
}

// dw[i] += ws[0][i] + ws[1][i] + ..., summed in split order
__global__ void k_dwconv_wgrad_combine(const float* __restrict__ ws,
                                       float* __restrict__ dw, int n,
                                       int splits) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * blockDim.x) {
        float s = ws[i];
        for (int z = 1; z < splits; ++z) s += ws[(int64_t)z * n + i];
        dw[i] += s;
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
static size_t dw_fwd_lds(int S, int KR, int KC, const DTile& g) {
    return (size_t)dw_sr(S, KR, g.TR) * dw_sw(S, KC, g.TW) * 128 +
           (size_t)KR * KC * 64 * 4;
}

template <int KS>
static void dw_launch_conv(const void* in, const void* w16, void* out, int N,
                           int Hin, int Win, int Hout, int Wout, int C,
                           int stride, int flip, hipStream_t stream) {
    const DTile g = dw_tile(stride, KS, KS, Hout, Wout, false, DW_SLAB_BYTES);
    const dim3 grid(N * g.rt * g.ct, (C + 63) / 64);
    const size_t lds = dw_fwd_lds(stride, KS, KS, g);
    if (stride == 1)
        k_dwconv_fwd<KS, 1><<<grid, DW_THREADS, lds, stream>>>(
            (const uint16_t*)in, (const uint16_t*)w16, (uint16_t*)out, Hin,
            Win, Hout, Wout, C, flip, g);
    else
        k_dwconv_fwd<KS, 2><<<grid, DW_THREADS, lds, stream>>>(
            (const uint16_t*)in, (const uint16_t*)w16, (uint16_t*)out, Hin,
            Win, Hout, Wout, C, flip, g);
}

template <int KS>
static void dw_launch_dgrad_s2(const void* dy, const void* w16, void* dx,
                               const ConvDims& d, hipStream_t stream) {
    // tiles the largest class (even rows, even columns) with the widest
    // sub-kernel, so every class fits the slab
    constexpr int NMAX = (KS + 1) / 2;
    const DTile g = dw_tile(1, NMAX, NMAX, (d.H + 1) / 2, (d.W + 1) / 2, false,
                            DW_SLAB_BYTES);
    const dim3 grid(d.N * g.rt * g.ct, (d.C + 63) / 64, 4);
    k_dwconv_dgrad_s2<KS><<<grid, DW_THREADS, dw_fwd_lds(1, NMAX, NMAX, g),
                            stream>>>(
        (const uint16_t*)dy, (const uint16_t*)w16, (uint16_t*)dx, d.Ho, d.Wo,
        d.H, d.W, d.C, g);
}

template <int KS>
static void dw_launch_wgrad(const void* x, const void* dy, void* ws, void* dw,
                            const ConvDims& d, hipStream_t stream) {
    DTile g; int ntiles, tps, nsplit;
    dw_wgrad_split(d, &g, &ntiles, &tps, &nsplit);
    const dim3 grid(nsplit, (d.C + 63) / 64);
    size_t lds = ((size_t)dw_sr(d.stride, KS, g.TR) * dw_sw(d.stride, KS, g.TW) +
                  (size_t)g.TR * g.TW) * 128;
    const size_t red = (size_t)(DW_SLOTS / KS) * KS * KS * 64 * 4;
    if (lds < red) lds = red;
    if (d.stride == 1)
        k_dwconv_wgrad<KS, 1><<<grid, DW_THREADS, lds, stream>>>(
            (const uint16_t*)x, (const uint16_t*)dy, (float*)ws, d.H, d.W,
            d.Ho, d.Wo, d.C, g, ntiles, tps);
    else
        k_dwconv_wgrad<KS, 2><<<grid, DW_THREADS, lds, stream>>>(
            (const uint16_t*)x, (const uint16_t*)dy, (float*)ws, d.H, d.W,
            d.Ho, d.Wo, d.C, g, ntiles, tps);
    const int n = d.C * KS * KS;
    k_dwconv_wgrad_combine<<<ew_grid(n, 256, 1), 256, 0, stream>>>(
        (const float*)ws, (float*)dw, n, nsplit);
}

// w16: bf16 [C][k][k][1].  Each launcher returns 0 (nothing launched) where
// dwconv_plan declines the shape.
extern "C" int launch_dwconv_fwd(const void* x, const void* w16, void* y,
                                 ConvDims d, hipStream_t stream) {
    if (!dw_ok(d)) return 0;
    if (d.R == 3)
        dw_launch_conv<3>(x, w16, y, d.N, d.H, d.W, d.Ho, d.Wo, d.C, d.stride, 0, stream);
    else if (d.R == 5)
        dw_launch_conv<5>(x, w16, y, d.N, d.H, d.W, d.Ho, d.Wo, d.C, d.stride, 0, stream);
    else
        dw_launch_conv<7>(x, w16, y, d.N, d.H, d.W, d.Ho, d.Wo, d.C, d.stride, 0, stream);
    return 1;
}

extern "C" int launch_dwconv_dgrad(const void* dy, const void* w16, void* dx,
                                   ConvDims d, hipStream_t stream) {
    if (!dw_ok(d)) return 0;
    if (d.stride == 1) {    // Ho == H, Wo == W: forward on dy, taps flipped
        if (d.R == 3)
            dw_launch_conv<3>(dy, w16, dx, d.N, d.Ho, d.Wo, d.H, d.W, d.C, 1, 1, stream);
        else if (d.R == 5)
            dw_launch_conv<5>(dy, w16, dx, d.N, d.Ho, d.Wo, d.H, d.W, d.C, 1, 1, stream);
        else
            dw_launch_conv<7>(dy, w16, dx, d.N, d.Ho, d.Wo, d.H, d.W, d.C, 1, 1, stream);
    } else if (d.R == 3) {
        dw_launch_dgrad_s2<3>(dy, w16, dx, d, stream);
    } else if (d.R == 5) {
        dw_launch_dgrad_s2<5>(dy, w16, dx, d, stream);
    } else {
        dw_launch_dgrad_s2<7>(dy, w16, dx, d, stream);
    }
    return 1;
}

// ws: fp32 [splits][C][k*k] with splits from dwconv_plan; dw += their sum
extern "C" int launch_dwconv_wgrad(const void* x, const void* dy, void* ws,
                                   void* dw, ConvDims d, hipStream_t stream) {
    if (!dw_ok(d)) return 0;
    if (d.R == 3) dw_launch_wgrad<3>(x, dy, ws, dw, d, stream);
    else if (d.R == 5) dw_launch_wgrad<5>(x, dy, ws, dw, d, stream);
    else dw_launch_wgrad<7>(x, dy, ws, dw, d, stream);
    return 1;
}

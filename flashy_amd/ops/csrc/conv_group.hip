// Copyright (c) Flashy-AMD authors.
// NHWC bf16 GROUPED 3x3 convolution (pad 1, stride 1 or 2) for gfx950:
// forward, backward-data and backward-weights for C == K, C % 64 == 0 and
// Cg = C / groups in {4, 8, 16, 32} (the ResNeXt 32x4d / 64x4d / 32x8d
// family).  gconv_plan() below is the only place that decides.
//
// Unit of work: a CHUNK of 16 consecutive output channels = one MFMA tile.
//   Cg <= 16: a chunk holds 16/Cg whole groups and reads exactly its own 16
//             input channels (Ci = 16); per tap its weights are a 16x16
//             block-diagonal matrix whose zeros are multiplied on purpose.
//   Cg == 32: a chunk reads its group's 32 input channels (Ci = 32); per tap
//             its weights are a full 16x32 matrix.
// The problem is memory-bound (72..144 flop/B against ~300 flop/B of the
// part, derived not measured), so the kernels are built around traffic: the
// activation slab of a tile, with its halo, is staged ONCE into LDS and all
// taps are served from there; the output is written once.
//
// k_gconv_expand builds the chunk-major operand [K/16][9][16 out][Ci in]
// (bf16, explicit zeros) from the grouped weights [K][3][3][Cg]; with
// `dgrad` it builds the backward-data operand instead (in/out transposed
// within the group, taps flipped).
//
// MFMA K = 32.  At Ci = 32 one tap fills it.  At Ci = 16 the kernels PAIR
// taps (k = tapsel*16 + ci: lanes 0..31 carry tap 2p, lanes 32..63 tap 2p+1)
// instead of using the 16x16x16 instruction: 5 instead of 9 MFMA issues per
// 16 pixels and every LDS fragment read stays a 16-byte ds_read_b128.  The
// pairing happens when a lane picks its fragment, so the operand in memory
// needs no padding; the odd ninth tap's partner half is fed zeros on both
// sides (a zero weight alone would turn an Inf activation into NaN).
//
// Operands are swapped (A = weights, B = pixels) so an accumulator lane
// holds 4 consecutive channels of one pixel: the epilogue stores 8 packed
// bytes per lane, guarded by the tile extent.
//
// Tiles are rectangles of TR output rows x TW output columns of one image
// (whole rows where the width allows, see gconv_tile).  LDS slab: one row of
// 64 channels (128 B) per input pixel at a pitch of 144 B.
//   * 16-byte alignment holds for every b128 access.
//   * A 16-lane group of a fragment read takes 16 consecutive pixels of one
//     tap at one channel octet: 36 dwords apart, i.e. banks
//     {0,36,8,44,16,52,24,60,32,4,40,12,48,20,56,28} + 0..3, all distinct.
//   * At stride 2 consecutive output pixels sit two input columns apart
//     (72 dwords = 8 banks mod 64, a 2-way conflict), so the slab keeps even
//     and odd input columns in two halves of each row: a tap then reads
//     consecutive entries again.
//   * A pixel group that wraps to the next tile row breaks the sequence once;
//     its cost is not measured.  That b128 reads are resolved per 16 lanes
//     is the family's working assumption (conv_common.h), not measured here.
//
// Backward-data at stride 1 is the forward kernel on dy with the dgrad
// operand.  At stride 2 it is split by the parity of (h, w) as conv_dgrad8
// documents: dx[2i+ph][2j+pw] only sees taps with r = 1 (ph = 0) or r in
// {0, 2} (ph = 1), likewise s, so the four classes have 1, 2, 2 and 4 taps
// and no multiply meets a structural zero.  grid.z is the class, the class
// grid is tiled like an image, odd H / W shorten the odd classes (guarded by
// the class extent) and the epilogue writes rows 2i+ph, columns 2j+pw.
//
// Backward-weights: per chunk and tap D[16 out][Ci in] = sum_m dy[m][k] *
// x[m @ tap][c].  Both operands sit [pixel][channel] in LDS as loaded and are
// read transposed with ds_read_b64_tr_b16 exactly as conv_wgrad.hip does
// (a 16-lane group gathers [4 pixels][16 channels]; rows 144 B apart land on
// banks {0,36,8,44} + 0..7).  A pixel that carries no dy (tile padding, tile
// rows or columns past the image) reads zeros on BOTH sides, as in forward.
// A block owns a 64-channel slab and a range of
// tiles, keeps the 9 tap accumulators of its chunk in registers, and writes
// the diagonal Cg x Cg blocks as its own fp32 slice [K][9][Cg] of a
// workspace.  k_gconv_wgrad_combine sums the slices in split order and adds
// into dw: no atomics, no spin-waits, bitwise repeatable.

#include "conv_common.h"

#define GC_P 72            // LDS pixel pitch in bf16 elements (144 B)
#define GC_THREADS 256     // 4 waves, one chunk each
#define GC_MAXPIX 128      // output pixels per tile
#define GC_SLAB_BYTES (44 * 1024)

struct GTile {
    int TR, TW;     // output rows / columns per tile
    int rt, ct;     // tiles per image along rows / columns
    int SR, SWc;    // staged input rows / columns (with halo)
    int SW, HALF;   // LDS row pitch in pixels; offset of the odd-column half
};

// mode 0: conv stride 1, 1: conv stride 2, 2: one stride-2 dgrad class
static GTile gconv_tile(int mode, int Hc, int Wc) {
    GTile g;
    const int parts = (Wc + 31) / 32;
    g.TW = (Wc + parts - 1) / parts;
    g.TR = GC_MAXPIX / g.TW;
    if (g.TR > Hc) g.TR = Hc;
    if (g.TR < 1) g.TR = 1;
    for (;;) {
        if (mode == 0) {
            g.SR = g.TR + 2; g.SWc = g.TW + 2; g.SW = g.SWc; g.HALF = 0;
        } else if (mode == 1) {
            g.SR = 2 * g.TR + 1; g.SWc = 2 * g.TW + 1;
            g.HALF = g.TW + 1; g.SW = 2 * g.HALF;
        } else {
            g.SR = g.TR + 1; g.SWc = g.TW + 1; g.SW = g.SWc; g.HALF = 0;
        }
        if (g.SR * g.SW * GC_P * 2 <= GC_SLAB_BYTES || g.TR == 1) break;
        --g.TR;
    }
    g.rt = (Hc + g.TR - 1) / g.TR;
    g.ct = (Wc + g.TW - 1) / g.TW;
    return g;
}

static int gconv_ci(const ConvDims& d, int groups) {
    if (groups <= 1 || d.C != d.K || d.C % 64 != 0 || d.C % groups != 0)
        return 0;
    const int cg = d.C / groups;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return 0;
    if (d.R != 3 || d.S != 3 || d.pad != 1) return 0;
    if (d.stride != 1 && d.stride != 2) return 0;
    if (d.N < 1 || d.H < 1 || d.W < 1) return 0;
    if (d.Ho != (d.H - 1) / d.stride + 1 || d.Wo != (d.W - 1) / d.stride + 1)
        return 0;
    return cg == 32 ? 32 : 16;
}

static void gconv_wgrad_split(const ConvDims& d, GTile* g, int* ntiles,
                              int* tps, int* nsplit) {
    *g = gconv_tile(d.stride == 2 ? 1 : 0, d.Ho, d.Wo);
    *ntiles = d.N * g->rt * g->ct;
    const int slabs = d.C / 64;
    int want = (512 + slabs - 1) / slabs;    // two blocks per CU of 256
    if (want > *ntiles) want = *ntiles;
    *tps = (*ntiles + want - 1) / want;
    *nsplit = (*ntiles + *tps - 1) / *tps;
}

// Dims-only plan: the MFMA reduction width per tap (16 or 32) the grouped
// path runs `d` with, or 0 where it does not serve the shape; *wgrad_splits
// is the number of fp32 slices gconv_wgrad writes.
extern "C" int gconv_plan(ConvDims d, int groups, int* wgrad_splits) {
    const int ci = gconv_ci(d, groups);
    *wgrad_splits = 0;
    if (ci) {
        GTile g; int ntiles, tps;
        gconv_wgrad_split(d, &g, &ntiles, &tps, wgrad_splits);
    }
    return ci;
}

// ---------------------------------------------------------------------------
__global__ void k_gconv_expand(const uint16_t* __restrict__ w,
                               uint16_t* __restrict__ wexp, int K, int Cg,
                               int Ci, int dgrad) {
    const int total = (K / 16) * 9 * 16 * Ci;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += gridDim.x * blockDim.x) {
        const int i = idx % Ci;
        const int o = (idx / Ci) & 15;
        const int t = (idx / (Ci * 16)) % 9;
        const int j = idx / (Ci * 144);
        const int oc = j * 16 + o;
        const int g = oc / Cg;
        const int ic = (Ci == 16 ? j * 16 : g * 32) + i;
        uint16_t v = 0;
        if (ic / Cg == g)
            v = dgrad ? w[((int64_t)ic * 9 + (8 - t)) * Cg + (oc - g * Cg)]
                      : w[((int64_t)oc * 9 + t) * Cg + (ic - g * Cg)];
        wexp[idx] = v;
    }
}

// ---------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ int gc_pos(int sr, int sc, const GTile& g) {
    if (MODE == 1) return sr * g.SW + (sc & 1) * g.HALF + (sc >> 1);
    return sr * g.SW + sc;
}

template <int MODE>
__device__ __forceinline__ int gc_base(int pr, int pc, const GTile& g) {
    return (MODE == 1 ? 2 * pr : pr) * g.SW + pc;
}

// LDS pixel offset (relative to gc_base) and operand tap index of tap t
template <int MODE>
__device__ __forceinline__ void gc_tap(int t, int ph, int pw, const GTile& g,
                                       int& off, int& widx) {
    if (MODE == 2) {
        const int ns = pw ? 2 : 1;
        const int a = t / ns, b = t - a * ns;
        const int r = ph ? 2 * a : 1, dr = ph ? 1 - a : 0;
        const int s = pw ? 2 * b : 1, dc = pw ? 1 - b : 0;
        off = dr * g.SW + dc;
        widx = 8 - (r * 3 + s);      // the dgrad operand is tap-flipped
    } else {
        const int r = t / 3, s = t - r * 3;
        off = r * g.SW + (MODE == 1 ? (s & 1) * g.HALF + (s >> 1) : s);
        widx = t;
    }
}

// Stage the 64-channel slab rows [oh, oh+SR) x columns [ow, ow+SWc) of image
// n into LDS, zeros outside the image; one 16-byte lane per channel octet.
template <int MODE>
__device__ __forceinline__ void gc_stage(const uint16_t* __restrict__ in,
                                         uint16_t* lds, int n, int Hin,
                                         int Win, int C, int ch0, int oh,
                                         int ow, const GTile& g) {
    const int oct = (threadIdx.x & 7) * 8;
    const int count = g.SR * g.SWc;
    for (int pix = threadIdx.x >> 3; pix < count; pix += GC_THREADS / 8) {
        const int sr = pix / g.SWc, sc = pix - sr * g.SWc;
        const int ih = oh + sr, iw = ow + sc;
        short8 v = {};
        if (ih >= 0 && ih < Hin && iw >= 0 && iw < Win)
            v = *reinterpret_cast<const short8*>(
                in + (((int64_t)n * Hin + ih) * Win + iw) * C + ch0 + oct);
        *reinterpret_cast<short8*>(&lds[gc_pos<MODE>(sr, sc, g) * GC_P + oct]) = v;
    }
}

template <int Ci, int MODE, int NT>
__device__ __forceinline__ void gc_body(
    const uint16_t* lds, const uint16_t* __restrict__ wexp,
    uint16_t* __restrict__ out, int n, int Hout, int Wout, int C, int Hc,
    int Wc, int r0, int c0, int ph, int pw, const GTile& g) {
    constexpr int NA = Ci == 16 ? (NT + 1) / 2 : NT;
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int chunk = blockIdx.y * 4 + wid;
    const int koff = Ci == 16 ? ((lane >> 4) & 1) * 8 : (lane >> 4) * 8;
    const int chin = (Ci == 16 ? wid * 16 : (wid >> 1) * 32) + koff;
    short8 a[NA];
    int toff[NA];
    bool tval[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int t = Ci == 16 ? 2 * i + (lane >> 5) : i;
        tval[i] = t < NT;
        int off, widx;
        gc_tap<MODE>(tval[i] ? t : 0, ph, pw, g, off, widx);
        a[i] = short8{};
        if (tval[i])
            a[i] = *reinterpret_cast<const short8*>(
                wexp + (((int64_t)chunk * 9 + widx) * 16 + (lane & 15)) * Ci + koff);
        toff[i] = off * GC_P + chin;
    }
    const int npix = g.TR * g.TW;
    for (int pg = 0; pg * 16 < npix; ++pg) {
        const int p = pg * 16 + (lane & 15);
        const int pcl = min(p, npix - 1);
        const int pr = pcl / g.TW, pc = pcl - pr * g.TW;
        const int base = gc_base<MODE>(pr, pc, g) * GC_P;
        short8 b[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            b[i] = *reinterpret_cast<const short8*>(&lds[base + toff[i]]);
            if (!tval[i]) b[i] = short8{};
        }
        floatx4 acc = {};
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < NA; ++i) acc = MFMA_BF16(a[i], b[i], acc);
        __builtin_amdgcn_s_setprio(0);
        const int orow = r0 + pr, ocol = c0 + pc;
        if (p < npix && orow < Hc && ocol < Wc) {
            const int h = MODE == 2 ? 2 * orow + ph : orow;
            const int w = MODE == 2 ? 2 * ocol + pw : ocol;
            uint2 v;
            v.x = (uint32_t)f32_to_bf16(acc[0]) | ((uint32_t)f32_to_bf16(acc[1]) << 16);
            v.y = (uint32_t)f32_to_bf16(acc[2]) | ((uint32_t)f32_to_bf16(acc[3]) << 16);
            *reinterpret_cast<uint2*>(
                out + (((int64_t)n * Hout + h) * Wout + w) * C +
                chunk * 16 + (lane >> 4) * 4) = v;
        }
    }
}

// in: [N][Hin][Win][C], out: [N][Hout][Wout][C].  MODE 0 / 1: conv at stride
// 1 / 2 (also stride-1 dgrad with the dgrad operand); MODE 2: stride-2 dgrad,
// in = dy, out = dx, blockIdx.z = parity class.
template <int Ci, int MODE>
__global__ void __launch_bounds__(GC_THREADS)
k_gconv_fwd(const uint16_t* __restrict__ in, const uint16_t* __restrict__ wexp,
            uint16_t* __restrict__ out, int Hin, int Win, int Hout, int Wout,
            int C, GTile g) {
    extern __shared__ __attribute__((aligned(16))) uint16_t gc_lds[];
    const int ph = MODE == 2 ? (int)(blockIdx.z >> 1) : 0;
    const int pw = MODE == 2 ? (int)(blockIdx.z & 1) : 0;
    const int Hc = MODE == 2 ? (Hout - ph + 1) >> 1 : Hout;
    const int Wc = MODE == 2 ? (Wout - pw + 1) >> 1 : Wout;
    int tile = blockIdx.x;
    const int c0 = (tile % g.ct) * g.TW; tile /= g.ct;
    const int r0 = (tile % g.rt) * g.TR;
    const int n = tile / g.rt;
    if (r0 >= Hc || c0 >= Wc) return;   // block-uniform: a shorter odd class
    const int oh = MODE == 0 ? r0 - 1 : MODE == 1 ? 2 * r0 - 1 : r0;
    const int ow = MODE == 0 ? c0 - 1 : MODE == 1 ? 2 * c0 - 1 : c0;
    gc_stage<MODE>(in, gc_lds, n, Hin, Win, C, blockIdx.y * 64, oh, ow, g);
    __syncthreads();
    if (MODE != 2)
        gc_body<Ci, MODE, 9>(gc_lds, wexp, out, n, Hout, Wout, C, Hc, Wc, r0,
                             c0, 0, 0, g);
    else if (ph && pw)
        gc_body<Ci, MODE, 4>(gc_lds, wexp, out, n, Hout, Wout, C, Hc, Wc, r0,
                             c0, ph, pw, g);
    else if (ph || pw)
        gc_body<Ci, MODE, 2>(gc_lds, wexp, out, n, Hout, Wout, C, Hc, Wc, r0,
                             c0, ph, pw, g);
    else
        gc_body<Ci, MODE, 1>(gc_lds, wexp, out, n, Hout, Wout, C, Hc, Wc, r0,
                             c0, ph, pw, g);
}

// ---------------------------------------------------------------------------
// two transpose reads (+4 pixel rows) build one 8-deep MFMA operand
__device__ __forceinline__ short8 gc_tr2(const uint16_t* p0, const uint16_t* p1) {
    union { struct { unsigned long long lo, hi; } q; short8 v; } u;
    const unsigned a0 = (unsigned)(unsigned long long)(const void*)p0;
    const unsigned a1 = (unsigned)(unsigned long long)(const void*)p1;
    asm volatile(
        "ds_read_b64_tr_b16 %0, %2\n\t"
        "ds_read_b64_tr_b16 %1, %3\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(u.q.lo), "=&v"(u.q.hi) : "v"(a0), "v"(a1) : "memory");
    return u.v;
}

template <int Ci>
__global__ void __launch_bounds__(GC_THREADS)
k_gconv_wgrad(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy,
              float* __restrict__ ws, int H, int W, int Ho, int Wo, int C,
              int Cg, int stride, GTile g, int ntiles, int tps) {
    constexpr int NB = Ci / 16;
    extern __shared__ __attribute__((aligned(16))) uint16_t gc_lds[];
    uint16_t* const xs = gc_lds;
    uint16_t* const dys = gc_lds + g.SR * g.SW * GC_P;
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int chunk = blockIdx.y * 4 + wid;
    const int sub = 4 * (lane & 3);                 // channels of this tr lane
    const int chin = (Ci == 16 ? wid * 16 : (wid >> 1) * 32) + sub;
    const int npix = g.TR * g.TW;
    const int npad = (npix + 31) & ~31;
    // one zero pixel row: the x operand of a pixel that carries no dy (tile
    // padding, tile rows / columns past the image), so that such a pixel
    // contributes 0 * 0 and never 0 * Inf
    uint16_t* const zrow = dys + npad * GC_P;
    if (threadIdx.x < GC_P / 8)
        *reinterpret_cast<short8*>(&zrow[threadIdx.x * 8]) = short8{};
    floatx4 acc[9][NB] = {};

    const int t_end = min(ntiles, ((int)blockIdx.x + 1) * tps);
    for (int tile = blockIdx.x * tps; tile < t_end; ++tile) {
        int tt = tile;
        const int c0 = (tt % g.ct) * g.TW; tt /= g.ct;
        const int r0 = (tt % g.rt) * g.TR;
        const int n = tt / g.rt;
        __syncthreads();    // the previous tile's reads are done
        if (stride == 2)
            gc_stage<1>(x, xs, n, H, W, C, blockIdx.y * 64, 2 * r0 - 1,
                        2 * c0 - 1, g);
        else
            gc_stage<0>(x, xs, n, H, W, C, blockIdx.y * 64, r0 - 1, c0 - 1, g);
        // dy rows of the tile's pixels, zeros for pixels outside the image
        // and for the padding up to a multiple of 32
        for (int p = threadIdx.x >> 3; p < npad; p += GC_THREADS / 8) {
            const int pr = p / g.TW, pc = p - pr * g.TW;
            const int oct = (threadIdx.x & 7) * 8;
            short8 v = {};
            if (p < npix && r0 + pr < Ho && c0 + pc < Wo)
                v = *reinterpret_cast<const short8*>(
                    dy + (((int64_t)n * Ho + r0 + pr) * Wo + c0 + pc) * C +
                    blockIdx.y * 64 + oct);
            *reinterpret_cast<short8*>(&dys[p * GC_P + oct]) = v;
        }
        __syncthreads();
        for (int m0 = 0; m0 < npad; m0 += 32) {
            const uint16_t* xb[2];
            const uint16_t* db[2];
            bool live[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int m = m0 + (lane >> 4) * 8 + h * 4 + ((lane & 15) >> 2);
                const int mcl = min(m, npix - 1);
                const int pr = mcl / g.TW, pc = mcl - pr * g.TW;
                live[h] = m < npix && r0 + pr < Ho && c0 + pc < Wo;
                const int base = (stride == 2 ? 2 * pr : pr) * g.SW + pc;
                xb[h] = xs + base * GC_P + chin;
                db[h] = dys + m * GC_P + wid * 16 + sub;
            }
            const short8 a = gc_tr2(db[0], db[1]);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int r = t / 3, s = t % 3;
                const int off = (r * g.SW + (stride == 2
                    ? (s & 1) * g.HALF + (s >> 1) : s)) * GC_P;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const short8 b = gc_tr2(
                        live[0] ? xb[0] + off + nb * 16 : zrow + sub + nb * 16,
                        live[1] ? xb[1] + off + nb * 16 : zrow + sub + nb * 16);
                    acc[t][nb] = MFMA_BF16(a, b, acc[t][nb]);
                }
            }
        }
    }
    // this split's slice [K][9][Cg]: only the diagonal blocks are kept
    float* const slice = ws + (int64_t)blockIdx.x * C * 9 * Cg;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int o = (lane >> 4) * 4 + rr;
                const int i = nb * 16 + (lane & 15);
                if (Ci == 32 || o / Cg == i / Cg)
                    slice[((int64_t)(chunk * 16 + o) * 9 + t) * Cg +
                          (Ci == 32 ? i : i % Cg)] = acc[t][nb][rr];
            }
}

// One gradient element per thread (a wave reads 256 contiguous bytes of each
// slice): dw[i] += ws[0][i] + ws[1][i] + ..., summed in split order.
__global__ void k_gconv_wgrad_combine(const float* __restrict__ ws,
                                      float* __restrict__ dw, int n,
                                      int splits) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * blockDim.x) {
        float s = ws[i];
        for (int z = 1; z < splits; ++z) s += ws[(int64_t)z * n + i];
        dw[i] += s;
    }
}

// ---------------------------------------------------------------------------
extern "C" void launch_gconv_expand(const void* w16, void* wexp, int K, int Cg,
                                    int dgrad, hipStream_t stream) {
    const int ci = Cg == 32 ? 32 : 16;
    const int total = (K / 16) * 9 * 16 * ci;
    k_gconv_expand<<<ew_grid(total, 256, 1), 256, 0, stream>>>(
        (const uint16_t*)w16, (uint16_t*)wexp, K, Cg, ci, dgrad);
}

template <int MODE>
static void gconv_launch(int ci, const void* in, const void* wexp, void* out,
                         int N, int Hin, int Win, int Hout, int Wout, int C,
                         hipStream_t stream) {
    // MODE 2 tiles the largest class (even rows, even columns)
    const GTile g = MODE == 2
        ? gconv_tile(2, (Hout + 1) / 2, (Wout + 1) / 2)
        : gconv_tile(MODE, Hout, Wout);
    const dim3 grid(N * g.rt * g.ct, C / 64, MODE == 2 ? 4 : 1);
    const size_t lds = (size_t)g.SR * g.SW * GC_P * 2;
    if (ci == 16)
        k_gconv_fwd<16, MODE><<<grid, GC_THREADS, lds, stream>>>(
            (const uint16_t*)in, (const uint16_t*)wexp, (uint16_t*)out, Hin,
            Win, Hout, Wout, C, g);
    else
        k_gconv_fwd<32, MODE><<<grid, GC_THREADS, lds, stream>>>(
            (const uint16_t*)in, (const uint16_t*)wexp, (uint16_t*)out, Hin,
            Win, Hout, Wout, C, g);
}

// wexp: the forward operand of k_gconv_expand.  Returns 0 (nothing launched)
// where gconv_plan declines the shape.
extern "C" int launch_gconv_fwd(const void* x, const void* wexp, void* y,
                                ConvDims d, int groups, hipStream_t stream) {
    const int ci = gconv_ci(d, groups);
    if (!ci) return 0;
    if (d.stride == 1)
        gconv_launch<0>(ci, x, wexp, y, d.N, d.H, d.W, d.Ho, d.Wo, d.C, stream);
    else
        gconv_launch<1>(ci, x, wexp, y, d.N, d.H, d.W, d.Ho, d.Wo, d.C, stream);
    return 1;
}

// wexp: the dgrad operand of k_gconv_expand
extern "C" int launch_gconv_dgrad(const void* dy, const void* wexp, void* dx,
                                  ConvDims d, int groups, hipStream_t stream) {
    const int ci = gconv_ci(d, groups);
    if (!ci) return 0;
    if (d.stride == 1)
        gconv_launch<0>(ci, dy, wexp, dx, d.N, d.Ho, d.Wo, d.H, d.W, d.C, stream);
    else
        gconv_launch<2>(ci, dy, wexp, dx, d.N, d.Ho, d.Wo, d.H, d.W, d.C, stream);
    return 1;
}

// ws: fp32 [splits][K][9][Cg] with splits from gconv_plan; dw += their sum
extern "C" int launch_gconv_wgrad(const void* x, const void* dy, void* ws,
                                  void* dw, ConvDims d, int groups,
                                  hipStream_t stream) {
    const int ci = gconv_ci(d, groups);
    if (!ci) return 0;
    GTile g; int ntiles, tps, nsplit;
    gconv_wgrad_split(d, &g, &ntiles, &tps, &nsplit);
    const int cg = d.C / groups;
    const dim3 grid(nsplit, d.C / 64);
    const int npad = (g.TR * g.TW + 31) & ~31;
    const size_t lds = ((size_t)g.SR * g.SW + npad + 1) * GC_P * 2;
    if (ci == 16)
        k_gconv_wgrad<16><<<grid, GC_THREADS, lds, stream>>>(
            (const uint16_t*)x, (const uint16_t*)dy, (float*)ws, d.H, d.W,
            d.Ho, d.Wo, d.C, cg, d.stride, g, ntiles, tps);
    else
        k_gconv_wgrad<32><<<grid, GC_THREADS, lds, stream>>>(
            (const uint16_t*)x, (const uint16_t*)dy, (float*)ws, d.H, d.W,
            d.Ho, d.Wo, d.C, cg, d.stride, g, ntiles, tps);
    const int n = d.K * 9 * cg;
    k_gconv_wgrad_combine<<<ew_grid(n, 256, 1), 256, 0, stream>>>(
        (const float*)ws, (float*)dw, n, nsplit);
    return 1;
}

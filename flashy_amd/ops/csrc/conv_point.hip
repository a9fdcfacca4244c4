// Copyright (c) Flashy-AMD authors.
// NHWC bf16 POINTWISE (non-overlapping dense) convolution for gfx950:
// groups == 1, square kernel == stride == p in {1, 2}, pad 0, C % 8 == 0,
// K % 8 == 0, 8 <= K <= 4096, 8 <= p*p*C <= 4096, weights [K][p][p][C].
// Forward, backward-data and backward-weights.  pwconv_plan() below is the
// only place that decides support, column panels, reduction chunks and
// weight-gradient splits.
//
// GEMM view.  y[M][K] = A[M][KD] * W[K][KD]^T with M = N*Ho*Wo, KD = p*p*C.
// Row m of A is p runs of p*C contiguous, 16-byte aligned elements, one per
// tap row r, starting at x[n][ho*p + r][wo*p][0] (pw_row_off).  At p = 1, A
// is the activation tensor itself.  Backward-data is the same product with
// A = dy (a plain [M][K] matrix), the weight transposed and the row map on
// the store side: dx runs = dy[M][K] * W[K][KD].
//
// One core, k_pwconv_gemm<DGRAD, NTW>: out[M][NC] = A[M][RD] * B[NC][RD]^T,
// WEIGHT-STATIONARY over persistent blocks.  (RD, NC) = (KD, K) forward and
// (K, KD) backward-data.
//   * Panel.  Block (x, y) keeps B rows [y*NCP, (y+1)*NCP) for ALL RDp
//     reduction elements (RD padded to 32 with zeros written in LDS) in
//     Wp[NCP][RDp + 8] for its whole life.  Forward copies W rows in 16-byte
//     lanes.  Backward-data transposes while it fills the panel: consecutive
//     lanes take consecutive filters k, load the 16 bytes W[k][c .. c+8] and
//     write eight 2-byte elements Wp[c + j][k], consecutive lanes to
//     consecutive LDS addresses.  It costs each block one strided pass over
//     the weight (out of L2) and needs no extra launch, no workspace and no
//     second copy of the MFMA loop's fragment reads.
//   * Tiles.  The block walks row tiles x, x + gridDim.x, ... of 64 rows.
//     The reduction runs in chunks of CH elements (<= 256); a step is one
//     (tile, chunk).  A step's A tile is staged once, in 16-byte lanes, into
//     At[64][CH + 8]; lanes past RD and rows past M are explicit zeros.  The
//     next step's global loads are issued into registers as soon as the
//     current step's lanes sit in LDS, ahead of the MFMAs and the stores.
//   * MFMA.  v_mfma_f32_16x16x32_bf16.  Wave w owns the 16-column tiles w,
//     w + 4, ... (at most NTW) for all four 16-row sub-tiles; accumulators
//     (4 x NTW x 4 VGPRs) stay in registers across the chunks of a tile.
//   * Output.  The accumulators are rounded once into an LDS image
//     Ot[64][NCP + 8] and leave in full 16-byte lanes: forward to
//     y[m][col ..], backward-data to the run the row map names.  Columns are
//     guarded at 8-channel granularity (NC % 8 == 0).
//   * Backward-data writes every element of dx once: the GEMM writes what
//     the patches cover, and where H % 2 or W % 2 leaves a rim that no patch
//     covers, k_pwconv_dgrad_rim writes it as zeros (one small launch, only
//     at such sizes; the two kernels' elements are disjoint).
//
// LDS banks.  Every pitch is (32 j + 8) elements = 4 (4 j + 1) dwords.  A
// ds_read_b128 fragment read has 16 lanes on rows i = 0..15 at one column:
// lane i starts at dword 4 (4 j + 1) i, bank 4 ((4 j + 1) i mod 16); 4 j + 1
// is odd, so i -> (4 j + 1) i mod 16 is a bijection and the 16 lanes cover
// all 64 banks once, 4 dwords each.
//
// Backward-weights: dw[K][KD] += dy^T[K][M] * A[M][KD].  Block (s, t) owns
// the 64-filter x 128-column tile t of dw in fp32 accumulators (wave w: the
// filter tile w x 8 column tiles) and the contiguous range of 64-row steps
// [s * sps, (s + 1) * sps).  dy and A tiles are staged as loaded ([m][k],
// [m][kd]; ragged K / KD edges and the tail of M zero-filled) and both read
// transposed with ds_read_b64_tr_b16 as conv_wgrad.hip does.  Each split
// writes one fp32 slice of the workspace; k_pwconv_wgrad_combine sums the
// slices in split order and adds into dw.  No atomics: bitwise repeatable.

#include "conv_common.h"

#define PW_THREADS 256
#define PW_TM 64             // rows of a tile
#define PW_NV 8              // 16-byte lanes of A a thread prefetches
#define PW_CH 256            // reduction chunk, at most
#define PW_MAXNCP 384        // columns of a panel, at most (NTW = 6)
#define PW_LDS (160 * 1024)  // one block per CU at worst
#define PW_MAXGRID 512
#define PW_WK 64             // weight gradient: filters of a tile
#define PW_WC 128            //                  columns of a tile
#define PW_WBLOCKS 512       //                  blocks aimed at
#define PW_MAXSPLIT 512

struct PwGeom {
    int H, W, Ho, Wo, C, p;
    int M;        // N * Ho * Wo
    int RD, RDp;  // reduction length, padded to 32
    int CH;       // reduction chunk (a multiple of 32)
    int nch;      // chunks
    int NC;       // output columns
    int NCP;      // columns of a panel (a multiple of 16)
    int npanels;
    int ntiles;
};

static bool pw_ok(const ConvDims& d) {
    if (d.R != d.S || d.R != d.stride || (d.R != 1 && d.R != 2)) return false;
    if (d.pad != 0 || d.C < 8 || d.C % 8 != 0) return false;
    if (d.K < 8 || d.K > 4096 || d.K % 8 != 0) return false;
    if (d.R * d.R * d.C > 4096) return false;
    if (d.N < 1 || d.H < d.R || d.W < d.R) return false;
    if (d.Ho != d.H / d.R || d.Wo != d.W / d.R) return false;
    return (int64_t)d.N * d.H * d.W * d.C < (1ll << 40) &&
           (int64_t)d.N * d.Ho * d.Wo < (1ll << 30);
}

static PwGeom pw_geom(const ConvDims& d, bool dgrad) {
    PwGeom g;
    g.H = d.H; g.W = d.W; g.Ho = d.Ho; g.Wo = d.Wo; g.C = d.C; g.p = d.R;
    g.M = d.N * d.Ho * d.Wo;
    const int KD = d.R * d.R * d.C;
    g.RD = dgrad ? d.K : KD;
    g.NC = dgrad ? KD : d.K;
    g.RDp = (g.RD + 31) / 32 * 32;
    // a long reduction leaves the A tile less room beside a 16-column panel
    g.CH = g.RDp <= PW_CH ? g.RDp : g.RDp <= 2048 ? PW_CH : PW_CH / 2;
    g.nch = (g.RDp + g.CH - 1) / g.CH;
    // panel + output image per column, A tile and its pad per block
    const int per_col = (g.RDp + 8) * 2 + PW_TM * 2;
    const int fixed = PW_TM * (g.CH + 8) * 2 + PW_TM * 8 * 2;
    int fit = (PW_LDS - fixed) / per_col / 16 * 16;
    if (fit > PW_MAXNCP) fit = PW_MAXNCP;
    const int nc16 = (g.NC + 15) / 16;
    g.npanels = fit < 16 ? 0 : (nc16 * 16 + fit - 1) / fit;
    g.NCP = g.npanels ? (nc16 + g.npanels - 1) / g.npanels * 16 : 0;
    g.ntiles = (g.M + PW_TM - 1) / PW_TM;
    return g;
}

static size_t pw_gemm_lds(const PwGeom& g) {
    return ((size_t)g.NCP * (g.RDp + 8) + (size_t)PW_TM * (g.CH + 8) +
            (size_t)PW_TM * (g.NCP + 8)) * 2;
}

// steps of 64 rows per split, splits
static void pw_wgrad_split(const ConvDims& d, int* sps, int* nsplit) {
    const int KD = d.R * d.R * d.C;
    const int tiles = ((d.K + PW_WK - 1) / PW_WK) * ((KD + PW_WC - 1) / PW_WC);
    const int nsteps = (d.N * d.Ho * d.Wo + PW_TM - 1) / PW_TM;
    int want = (PW_WBLOCKS + tiles - 1) / tiles;
    if (want > PW_MAXSPLIT) want = PW_MAXSPLIT;
    if (want > nsteps) want = nsteps;
    *sps = (nsteps + want - 1) / want;
    *nsplit = (nsteps + *sps - 1) / *sps;
}

// Dims-only plan: 1 where the pointwise path serves `d`, else 0.  Outputs:
// column panels and reduction chunks of the forward and the backward-data
// GEMM, and the number of fp32 slices pwconv_wgrad writes.
extern "C" int pwconv_plan(ConvDims d, int* fwd_panels, int* fwd_chunks,
                           int* dgrad_panels, int* dgrad_chunks,
                           int* wgrad_splits) {
    *fwd_panels = *fwd_chunks = *dgrad_panels = *dgrad_chunks = 0;
    *wgrad_splits = 0;
    if (!pw_ok(d)) return 0;
    const PwGeom f = pw_geom(d, false), b = pw_geom(d, true);
    if (!f.npanels || !b.npanels) return 0;
    if (pw_gemm_lds(f) > PW_LDS || pw_gemm_lds(b) > PW_LDS) return 0;
    *fwd_panels = f.npanels; *fwd_chunks = f.nch;
    *dgrad_panels = b.npanels; *dgrad_chunks = b.nch;
    int sps;
    pw_wgrad_split(d, &sps, wgrad_splits);
    return 1;
}

// Everything up to the matching pop is compiled without packed fp32 math (see
// fused_optim.hip for why); a function under this attribute can only inline
// always_inline callees.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// what __syncthreads expands to
__device__ __forceinline__ void pw_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The row map: element offset in x / dx of column e (a multiple of 8, below
// p*p*C) of GEMM row m.  A 16-byte lane never straddles two runs: p*C % 8 == 0.
__device__ __forceinline__ int64_t pw_row_off(const PwGeom& g, int m, int e) {
    if (g.p == 1) return (int64_t)m * g.C + e;
    const int gr = m / g.Wo, wo = m - gr * g.Wo;
    const int n = gr / g.Ho, ho = gr - n * g.Ho;
    const int pc = g.p * g.C;
    const int r = e / pc, t = e - r * pc;
    return (((int64_t)n * g.H + ho * g.p + r) * g.W + wo * g.p) * g.C + t;
}

// Issue the loads of rows [m0, m0 + 64) x columns [e0, e0 + CH) of A; zeros
// past M and past RD.  MAPPED: A is x behind the row map, else a plain
// [M][RD] matrix.
template <bool MAPPED>
__device__ __forceinline__ void pw_load_a(const uint16_t* __restrict__ a,
                                          const PwGeom& g, int m0, int e0,
                                          short8* pre) {
    const int cpr = g.CH >> 3, nvec = PW_TM * cpr;
#pragma unroll
    for (int v = 0; v < PW_NV; ++v) {
        const int idx = threadIdx.x + v * PW_THREADS;
        short8 val = {};
        if (idx < nvec) {
            const int i = idx / cpr, e = e0 + 8 * (idx - i * cpr);
            const int m = m0 + i;
            if (m < g.M && e < g.RD) {
                const int64_t at = MAPPED ? pw_row_off(g, m, e)
                                          : (int64_t)m * g.RD + e;
                val = *reinterpret_cast<const short8*>(a + at);
            }
        }
        pre[v] = val;
    }
}

// into At[64][pitch]
__device__ __forceinline__ void pw_store_a(uint16_t* At, int cpr, int pitch,
                                           const short8* pre) {
    const int nvec = PW_TM * cpr;
#pragma unroll
    for (int v = 0; v < PW_NV; ++v) {
        const int idx = threadIdx.x + v * PW_THREADS;
        if (idx < nvec) {
            const int i = idx / cpr, c = idx - i * cpr;
            *reinterpret_cast<short8*>(&At[i * pitch + c * 8]) = pre[v];
        }
    }
}

// out[M][NC] = A[M][RD] * B[NC][RD]^T.  !DGRAD: A = x behind the row map,
// B = W [K][KD], out = y.  DGRAD: A = dy, B = W^T, out = dx behind the map.
template <bool DGRAD, int NTW>
__global__ void __launch_bounds__(PW_THREADS)
k_pwconv_gemm(const uint16_t* __restrict__ a, const uint16_t* __restrict__ w,
              uint16_t* __restrict__ out, PwGeom g) {
    extern __shared__ __attribute__((aligned(16))) uint16_t pw_lds[];
    const int PWP = g.RDp + 8, AP = g.CH + 8, OP = g.NCP + 8;
    uint16_t* const Wp = pw_lds;                 // [NCP][PWP]
    uint16_t* const At = Wp + g.NCP * PWP;       // [64][AP]
    uint16_t* const Ot = At + PW_TM * AP;        // [64][OP]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int col0 = blockIdx.y * g.NCP;
    const int ncols = min(g.NCP, g.NC - col0);          // a multiple of 8
    const int my_nt = (((ncols + 15) >> 4) - wid + 3) >> 2;

    // the panel, zeros past RD and past NC
    if (!DGRAD) {
        const int rv = g.RDp >> 3;
        for (int idx = tid; idx < g.NCP * rv; idx += PW_THREADS) {
            const int c = idx / rv, e = 8 * (idx - c * rv);
            short8 v = {};
            if (c < ncols && e < g.RD)
                v = *reinterpret_cast<const short8*>(
                    w + (int64_t)(col0 + c) * g.RD + e);
            *reinterpret_cast<short8*>(&Wp[c * PWP + e]) = v;
        }
    } else {
        // Wp[c][k] = W[k][col0 + c]: lanes along k, eight columns each
        for (int idx = tid; idx < (g.NCP >> 3) * g.RDp; idx += PW_THREADS) {
            const int cv = idx / g.RDp, k = idx - cv * g.RDp;
            short8 v = {};
            if (k < g.RD && 8 * cv < ncols)
                v = *reinterpret_cast<const short8*>(
                    w + (int64_t)k * g.NC + col0 + 8 * cv);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                Wp[(8 * cv + j) * PWP + k] = (uint16_t)v[j];
        }
    }

    floatx4 acc[4][NTW];
#pragma unroll
    for (int ms = 0; ms < 4; ++ms)
#pragma unroll
        for (int n = 0; n < NTW; ++n) acc[ms][n] = floatx4{};

    const int cpr = g.CH >> 3;
    short8 pre[PW_NV];
    int tile = blockIdx.x, ch = 0;
    if (tile < g.ntiles) pw_load_a<!DGRAD>(a, g, tile * PW_TM, 0, pre);
    while (tile < g.ntiles) {
        pw_store_a(At, cpr, AP, pre);
        pw_barrier();       // also: the panel is in place
        int tile_n = tile, ch_n = ch + 1;
        if (ch_n == g.nch) { ch_n = 0; tile_n = tile + gridDim.x; }
        if (tile_n < g.ntiles)      // in flight under the work below
            pw_load_a<!DGRAD>(a, g, tile_n * PW_TM, ch_n * g.CH, pre);
        const int kend = min(g.CH, g.RDp - ch * g.CH);
        for (int kk = 0; kk < kend; kk += 32) {
            short8 af[4];
#pragma unroll
            for (int ms = 0; ms < 4; ++ms)
                af[ms] = *reinterpret_cast<const short8*>(
                    &At[(ms * 16 + l15) * AP + kk + lq * 8]);
#pragma unroll
            for (int n = 0; n < NTW; ++n) {
                if (n < my_nt) {
                    const short8 bf = *reinterpret_cast<const short8*>(
                        &Wp[((wid + 4 * n) * 16 + l15) * PWP + ch * g.CH + kk +
                            lq * 8]);
#pragma unroll
                    for (int ms = 0; ms < 4; ++ms)
                        acc[ms][n] = MFMA_BF16(af[ms], bf, acc[ms][n]);
                }
            }
        }
        if (ch + 1 < g.nch) {
            pw_barrier();   // At is free again
        } else {
            const int m0 = tile * PW_TM, rows = min(PW_TM, g.M - m0);
#pragma unroll
            for (int n = 0; n < NTW; ++n) {
                if (n < my_nt) {
                    const int col = (wid + 4 * n) * 16 + l15;
#pragma unroll
                    for (int ms = 0; ms < 4; ++ms) {
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr)
                            Ot[(ms * 16 + lq * 4 + rr) * OP + col] =
                                f32_to_bf16(acc[ms][n][rr]);
                        acc[ms][n] = floatx4{};
                    }
                }
            }
            pw_barrier();   // the image is whole; At is free again
            const int ncv = ncols >> 3;
            for (int idx = tid; idx < rows * ncv; idx += PW_THREADS) {
                const int i = idx / ncv, c = 8 * (idx - i * ncv);
                const int64_t at = DGRAD ? pw_row_off(g, m0 + i, col0 + c)
                                         : (int64_t)(m0 + i) * g.NC + col0 + c;
                *reinterpret_cast<short8*>(out + at) =
                    *reinterpret_cast<const short8*>(&Ot[i * OP + c]);
            }
        }
        tile = tile_n; ch = ch_n;
    }
}

// dx's rim as zeros, in 16-byte lanes: per image the columns past the last
// patch of the rows [0, Ho * p), then the whole rows past them
__global__ void k_pwconv_dgrad_rim(uint16_t* __restrict__ dx, PwGeom g,
                                   int64_t total) {
    const int cv = g.C >> 3, hp = g.Ho * g.p;
    const int remw = (g.W - g.Wo * g.p) * cv, side = hp * remw;
    const int per = side + (g.H - hp) * g.W * cv;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = idx / per;
        const int q = (int)(idx - n * per);
        int64_t lane;       // 16-byte lane within the image
        if (q < side) {
            const int h = q / remw;
            lane = ((int64_t)h * g.W + g.Wo * g.p) * cv + (q - h * remw);
        } else {
            lane = (int64_t)hp * g.W * cv + (q - side);
        }
        *reinterpret_cast<short8*>(
            dx + (n * g.H * g.W * cv + lane) * 8) = short8{};
    }
}

// 16 rows (filters or columns at `p`, 4 contiguous per lane) x 32 pixels of a
// pixel-major LDS tile, transposed by the read: the lane ends with its row's
// 8 consecutive pixels (conv_wgrad.hip)
__device__ __forceinline__ short8 pw_tr_frag(const uint16_t* p, int pitch) {
    union { struct { unsigned long long lo, hi; } q; short8 v; } f;
    const unsigned a0 = (unsigned)(unsigned long long)(const void*)p;
    const unsigned a1 = a0 + (unsigned)pitch * 8;      // + 4 pixel rows
    asm volatile(
        "ds_read_b64_tr_b16 %0, %2\n\t"
        "ds_read_b64_tr_b16 %1, %3\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(f.q.lo), "=&v"(f.q.hi)
        : "v"(a0), "v"(a1)
        : "memory");
    return f.v;
}

#define PW_WDP (PW_WK + 8)   // pitch of the dy tile
#define PW_WAP (PW_WC + 8)   // pitch of the A tile

// Issue the loads of one 64-row step of the weight gradient: dy columns
// [k0, k0 + 64) (2 lanes a thread) and A columns [c0, c0 + 128) (4 lanes)
__device__ __forceinline__ void pw_wgrad_load(const uint16_t* __restrict__ x,
                                              const uint16_t* __restrict__ dy,
                                              const PwGeom& g, int K, int m0,
                                              int mend, int k0, int c0,
                                              short8* dpre, short8* apre) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int idx = threadIdx.x + v * PW_THREADS;
        const int i = idx >> 3, k = k0 + 8 * (idx & 7);
        short8 val = {};
        if (m0 + i < mend && k < K)
            val = *reinterpret_cast<const short8*>(
                dy + (int64_t)(m0 + i) * K + k);
        dpre[v] = val;
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int idx = threadIdx.x + v * PW_THREADS;
        const int i = idx >> 4, e = c0 + 8 * (idx & 15);
        short8 val = {};
        if (m0 + i < mend && e < g.RD)
            val = *reinterpret_cast<const short8*>(
                x + pw_row_off(g, m0 + i, e));
        apre[v] = val;
    }
}

// ws: fp32 [nsplit][K][KD]; block (s, t) reduces steps [s * sps, (s + 1) * sps)
// of 64 rows into the tile t = (filter tile, column tile) of slice s
__global__ void __launch_bounds__(PW_THREADS)
k_pwconv_wgrad(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy,
               float* __restrict__ ws, PwGeom g, int K, int sps) {
    __shared__ __attribute__((aligned(16))) uint16_t dyT[PW_TM * PW_WDP];
    __shared__ __attribute__((aligned(16))) uint16_t At[PW_TM * PW_WAP];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int KD = g.RD;
    const int kts = (K + PW_WK - 1) / PW_WK;
    const int k0 = ((int)blockIdx.y % kts) * PW_WK;
    const int c0 = ((int)blockIdx.y / kts) * PW_WC;
    // this lane's read of a transposed fragment: pixel row, 4-element column
    const int tr_row = lq * 8 + (l15 >> 2), tr_col = 4 * (lane & 3);

    floatx4 acc[PW_WC / 16];
#pragma unroll
    for (int n = 0; n < PW_WC / 16; ++n) acc[n] = floatx4{};

    const int m_lo = min(g.M, (int)blockIdx.x * sps * PW_TM);
    const int m_hi = min(g.M, m_lo + sps * PW_TM);
    short8 dpre[2], apre[4];
    pw_wgrad_load(x, dy, g, K, m_lo, m_hi, k0, c0, dpre, apre);
    for (int m0 = m_lo; m0 < m_hi; m0 += PW_TM) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int idx = tid + v * PW_THREADS;
            *reinterpret_cast<short8*>(
                &dyT[(idx >> 3) * PW_WDP + 8 * (idx & 7)]) = dpre[v];
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int idx = tid + v * PW_THREADS;
            *reinterpret_cast<short8*>(
                &At[(idx >> 4) * PW_WAP + 8 * (idx & 15)]) = apre[v];
        }
        pw_barrier();
        // past m_hi every lane loads zeros: nothing is read
        pw_wgrad_load(x, dy, g, K, m0 + PW_TM, m_hi, k0, c0, dpre, apre);
#pragma unroll
        for (int sc = 0; sc < PW_TM / 32; ++sc) {
            const short8 af = pw_tr_frag(
                &dyT[(sc * 32 + tr_row) * PW_WDP + wid * 16 + tr_col], PW_WDP);
#pragma unroll
            for (int n = 0; n < PW_WC / 16; ++n) {
                const short8 bf = pw_tr_frag(
                    &At[(sc * 32 + tr_row) * PW_WAP + n * 16 + tr_col], PW_WAP);
                acc[n] = MFMA_BF16(af, bf, acc[n]);
            }
        }
        pw_barrier();       // the tiles are free again
    }
    float* const slice = ws + (int64_t)blockIdx.x * K * KD;
#pragma unroll
    for (int n = 0; n < PW_WC / 16; ++n) {
        const int kk = c0 + n * 16 + l15;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int k = k0 + wid * 16 + lq * 4 + rr;
            if (k < K && kk < KD) slice[(int64_t)k * KD + kk] = acc[n][rr];
        }
    }
}

// dw[i] += ws[0][i] + ws[1][i] + ..., summed in split order
__global__ void k_pwconv_wgrad_combine(const float* __restrict__ ws,
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
template <bool DGRAD, int NTW>
static void pw_launch_gemm(const void* a, const void* w, void* out,
                           const PwGeom& g, hipStream_t stream) {
    static const bool attr_set = [] {
        (void)hipFuncSetAttribute((const void*)&k_pwconv_gemm<DGRAD, NTW>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  PW_LDS);
        return true;
    }();
    (void)attr_set;
    const int gx = g.ntiles < PW_MAXGRID ? g.ntiles : PW_MAXGRID;
    dim3 grid((unsigned)gx, (unsigned)g.npanels);
    k_pwconv_gemm<DGRAD, NTW><<<grid, PW_THREADS, pw_gemm_lds(g), stream>>>(
        (const uint16_t*)a, (const uint16_t*)w, (uint16_t*)out, g);
}

static int pw_planned(const ConvDims& d, int* splits) {
    int fp, fc, bp, bc;
    return pwconv_plan(d, &fp, &fc, &bp, &bc, splits);
}

// w16: bf16 [K][p][p][C].  Each launcher returns 0 (nothing launched) where
// pwconv_plan declines the shape.
extern "C" int launch_pwconv_fwd(const void* x, const void* w16, void* y,
                                 ConvDims d, hipStream_t stream) {
    int splits;
    if (!pw_planned(d, &splits)) return 0;
    const PwGeom g = pw_geom(d, false);
    if (g.NCP <= 128) pw_launch_gemm<false, 2>(x, w16, y, g, stream);
    else pw_launch_gemm<false, 6>(x, w16, y, g, stream);
    return 1;
}

extern "C" int launch_pwconv_dgrad(const void* dy, const void* w16, void* dx,
                                   ConvDims d, hipStream_t stream) {
    int splits;
    if (!pw_planned(d, &splits)) return 0;
    const PwGeom g = pw_geom(d, true);
    if (g.NCP <= 128) pw_launch_gemm<true, 2>(dy, w16, dx, g, stream);
    else pw_launch_gemm<true, 6>(dy, w16, dx, g, stream);
    const int64_t rim = (int64_t)d.N * (d.C / 8) *
        ((int64_t)d.Ho * d.R * (d.W - d.Wo * d.R) +
         (int64_t)(d.H - d.Ho * d.R) * d.W);
    if (rim > 0)
        k_pwconv_dgrad_rim<<<ew_grid(rim, 256, 1), 256, 0, stream>>>(
            (uint16_t*)dx, g, rim);
    return 1;
}

// ws: fp32 [splits][K][p*p*C] with splits from pwconv_plan; dw += their sum
extern "C" int launch_pwconv_wgrad(const void* x, const void* dy, void* ws,
                                   void* dw, ConvDims d, hipStream_t stream) {
    int nsplit, sps;
    if (!pw_planned(d, &nsplit)) return 0;
    const PwGeom g = pw_geom(d, false);
    pw_wgrad_split(d, &sps, &nsplit);
    const int KD = g.RD;
    dim3 grid((unsigned)nsplit, (unsigned)(((d.K + PW_WK - 1) / PW_WK) *
                                           ((KD + PW_WC - 1) / PW_WC)));
    k_pwconv_wgrad<<<grid, PW_THREADS, 0, stream>>>(
        (const uint16_t*)x, (const uint16_t*)dy, (float*)ws, g, d.K, sps);
    const int n = d.K * KD;
    k_pwconv_wgrad_combine<<<ew_grid(n, 256, 1), 256, 0, stream>>>(
        (const float*)ws, (float*)dw, n, nsplit);
    return 1;
}

// Copyright (c) Flashy-AMD authors.
// NHWC bf16 PATCH convolution for gfx950: kernel == stride == p in {2, 4},
// pad 0, C in {3, 4} input channels, K % 16 == 0 filters (16..512), weights
// [K][p][p][C]: the ConvNeXt patchify stem.  Forward, backward-data and
// backward-weights.  patchconv_plan() below is the only place that decides.
//
// A patch conv has no halo and no overlap: y[M][K] = X'[M][KD] * W[K][KD]^T
// with KD = p*p*C (12, 16, 48, 64) and X'[m][r*p*C + t] = the t-th element of
// the contiguous run x[n][ho*p + r][wo*p*C ...].  Nothing is padded or
// reshuffled in global memory; each direction reads every input byte once.
//
// Tiles and runs.  A tile is TM consecutive output pixels of the flattened
// (n, ho, wo) order (64 / 32 / 16 by K, so that TM * K <= 8192), whatever
// rows and images it crosses.  The tile's input is one RUN per (output row it
// touches, tap row r): (pixels of that row in the tile) * p * C contiguous
// elements.  A run's start is only 2- or 4-byte aligned (p = 2, C = 3: W * 6
// bytes per row), so the run is fetched from its start ALIGNED DOWN to 16
// bytes, in 16-byte lanes, into a slot of SL elements of the raw LDS buffer;
// the slot keeps the misalignment (`head`, 0..7 elements, parked in a small
// LDS table).  A lane whose 16 bytes would pass the end of the tensor loads
// the valid elements one by one instead: no wide load leaves the allocation.
// The (wo, r, s, c) re-indexing happens on the LDS side: pc_repack gathers
// bf16 pairs out of the runs into a clean operand tile At[TM][KP + 8], KP =
// KD padded with zeros to the next multiple of 32 (the k of
// v_mfma_f32_16x16x32_bf16), never to an 8x8 tap grid.
//
// Pipeline (forward, backward-data): a block walks tiles blockIdx.x,
// + gridDim.x, ...; the next tile's global loads are issued into registers
// before the current tile's LDS work and MFMAs, and land in LDS after them.
//
// Forward: the weights stay in REGISTERS for the whole block.  Wave w owns
// the 16-filter column tiles w, w + 4, ... (at most 8), as B fragments read
// once from the KRSC tensor; every wave reads all A fragments of the tile
// (ds_read_b128 from At, pitch 80 / 144 bytes).  The fp32 accumulators are
// rounded once into an LDS image [TM][K] of the output, which is one
// contiguous run of y: lanes store 16 bytes, a wave whole 128-byte lines.
//
// Backward-data: dx'[M][KD] = dy[M][K] * W[K][KD].  The dy tile is a
// contiguous run of global memory and is staged as it is ([TM][K32 + 8], K
// padded with zeros to 32).  Wave (nt, mg) owns the 16-column tile nt of KD
// (1, 1, 3, 4 of them) for the pixel sub-tiles mg, mg + G, ... and keeps its
// B fragments W[k][nt*16 ..] for all K in registers (at most 16 x 4 VGPRs).
// The accumulators are rounded into the SAME run layout the forward reads
// (slot, head, pixel * p * C + t), so the tile leaves as runs: 16-byte lanes
// where a lane lies inside the run, single elements at its two ragged ends
// (the neighbours there belong to other blocks).  The columns that no patch
// covers (W % p) ride at the end of the run that reaches the row's last
// patch, as zeros; the rows that no patch covers (H % p) are zeroed by the
// block whose tile holds the image's last pixel.  dx may arrive
// uninitialised.
//
// Backward-weights: dw[K][KD] += dy^T[K][M] * X'[M][KD], the reduction over
// M.  Block b owns the contiguous tile range [b * tps, (b + 1) * tps) and
// keeps the whole K x KD fp32 result in accumulators (wave w: filter tiles w,
// w + 4, ... x all column tiles, at most 8 x 4 x 4 VGPRs).  Both operands sit
// in LDS pixel-major ([m][k] as loaded, At as repacked) and are read with
// ds_read_b64_tr_b16 as conv_wgrad.hip does: two reads give a lane the 8
// consecutive pixels of one filter / one column.  The block writes one fp32
// slice [K][KD] of the workspace; k_patchconv_wgrad_combine sums the slices
// in block order and adds into dw.  No atomics: bitwise repeatable.
//
// Unmeasured: everything.  In particular the pair gather of pc_repack (two
// ds_read_u16 per 4 bytes), the duplicated A reads of the forward waves and
// the idle waves where KD has fewer than 4 column tiles.

#include "conv_common.h"

#define PC_THREADS 256
#define PC_NV 6          // 16-byte lanes of raw input a thread prefetches
#define PC_DV 8          // 16-byte lanes of dy a thread prefetches
#define PC_MAXGRID 512   // two blocks per CU of 256
#define PC_MAXSPLIT 256  // weight-gradient slices

struct PGeom {
    int H, W, Ho, Wo, K;
    int M;          // N * Ho * Wo
    int TM;         // pixels per tile
    int NR;         // output rows a tile touches, at most
    int SL;         // elements of a run's slot (a multiple of 8)
    int ntiles;
    int64_t xelems; // N * H * W * C
};

static bool pc_ok(const ConvDims& d) {
    if (d.R != d.S || d.R != d.stride || (d.R != 2 && d.R != 4)) return false;
    if (d.pad != 0 || (d.C != 3 && d.C != 4)) return false;
    if (d.K < 16 || d.K > 512 || d.K % 16 != 0) return false;
    if (d.N < 1 || d.H < d.R || d.W < d.R) return false;
    if (d.Ho != d.H / d.R || d.Wo != d.W / d.R) return false;
    return (int64_t)d.N * d.Ho * d.Wo < (1ll << 30);
}

// wgrad: tiles hold whole 32-pixel reduction chunks
static PGeom pc_geom(const ConvDims& d, bool wgrad) {
    PGeom g;
    g.H = d.H; g.W = d.W; g.Ho = d.Ho; g.Wo = d.Wo; g.K = d.K;
    g.M = d.N * d.Ho * d.Wo;
    g.TM = d.K <= 128 ? 64 : d.K <= 256 ? 32 : 16;
    if (wgrad && g.TM < 32) g.TM = 32;
    const int rw = d.Wo < g.TM ? d.Wo : g.TM;     // pixels of a run
    g.NR = (g.TM + d.Wo - 2) / d.Wo + 1;
    if (g.NR > g.TM) g.NR = g.TM;
    // a head of up to 7 elements, the run, the columns no patch covers
    g.SL = (7 + rw * d.R * d.C + (d.W - d.Wo * d.R) * d.C + 7) / 8 * 8;
    g.ntiles = (g.M + g.TM - 1) / g.TM;
    g.xelems = (int64_t)d.N * d.H * d.W * d.C;
    return g;
}

static int pc_kp(const ConvDims& d) { return (d.R * d.R * d.C + 31) / 32 * 32; }

static void pc_wgrad_split(const PGeom& g, int* tps, int* nsplit) {
    const int want = g.ntiles < PC_MAXSPLIT ? g.ntiles : PC_MAXSPLIT;
    *tps = (g.ntiles + want - 1) / want;
    *nsplit = (g.ntiles + *tps - 1) / *tps;
}

// Dims-only plan: 1 where the patch path serves `d`, else 0; *wgrad_splits is
// the number of fp32 slices patchconv_wgrad writes.
extern "C" int patchconv_plan(ConvDims d, int* wgrad_splits) {
    *wgrad_splits = 0;
    if (!pc_ok(d)) return 0;
    const PGeom g = pc_geom(d, true);
    if (g.NR * d.R * (g.SL / 8) > PC_NV * PC_THREADS) return 0;
    int tps;
    pc_wgrad_split(g, &tps, wgrad_splits);
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
__device__ __forceinline__ void pc_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int pc_min(int a, int b) { return a < b ? a : b; }

// The tile [m0, mend): its first output row and the column it starts at.
struct PTile { int m0, mend, grow0, wof; };

__device__ __forceinline__ PTile pc_tile(const PGeom& g, int tile) {
    PTile t;
    t.m0 = tile < g.ntiles ? tile * g.TM : g.M;
    t.mend = pc_min(t.m0 + g.TM, g.M);
    t.grow0 = t.m0 / g.Wo;
    t.wof = t.m0 - t.grow0 * g.Wo;
    return t;
}

// Run `run` = (row of the tile, tap row) in the x / dx tensor: it starts at
// element a0 + head, a0 a multiple of 8, and is len elements long (0: no
// such run).  With `rem` the columns no patch covers join the run that
// reaches the row's last patch.
struct PRun { int64_t a0; int head, len; };

template <int P, int C>
__device__ __forceinline__ PRun pc_run(const PGeom& g, const PTile& t, int run,
                                       bool rem) {
    const int row = run / P, r = run - row * P;
    const int gr = t.grow0 + row;
    const int wo_s = row == 0 ? t.wof : 0;
    const int wo_e = pc_min(g.Wo, t.mend - gr * g.Wo);
    PRun o;
    o.a0 = 0; o.head = 0; o.len = 0;
    if (wo_e <= wo_s) return o;
    const int n = gr / g.Ho, ho = gr - n * g.Ho;
    const int64_t e0 =
        (((int64_t)n * g.H + ho * P + r) * g.W + wo_s * P) * C;
    o.a0 = e0 & ~(int64_t)7;
    o.head = (int)(e0 - o.a0);
    o.len = (wo_e - wo_s) * P * C;
    if (rem && wo_e == g.Wo) o.len += (g.W - g.Wo * P) * C;
    return o;
}

// Issue the tile's raw input loads: lane idx of the slot image [NR * P][SL]
template <int P, int C>
__device__ __forceinline__ void pc_load_x(const uint16_t* __restrict__ x,
                                          const PGeom& g, const PTile& t,
                                          short8* pre) {
    const int vpr = g.SL >> 3, nvec = g.NR * P * vpr;
#pragma unroll
    for (int v = 0; v < PC_NV; ++v) {
        const int idx = threadIdx.x + v * PC_THREADS;
        short8 val = {};
        if (idx < nvec) {
            const int run = idx / vpr, j = idx - run * vpr;
            const PRun o = pc_run<P, C>(g, t, run, false);
            if (8 * j < o.head + o.len) {
                const int64_t at = o.a0 + 8 * j;
                if (at + 8 <= g.xelems) {
                    val = *reinterpret_cast<const short8*>(x + at);
                } else {    // the tensor ends inside this lane
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        if (at + c < g.xelems) val[c] = (short)x[at + c];
                }
            }
        }
        pre[v] = val;
    }
}

// Park the prefetched lanes in the raw buffer and the runs' heads beside it
template <int P, int C>
__device__ __forceinline__ void pc_store_x(uint16_t* raw, int* heads,
                                           const PGeom& g, const PTile& t,
                                           const short8* pre) {
    const int nvec = g.NR * P * (g.SL >> 3);
#pragma unroll
    for (int v = 0; v < PC_NV; ++v) {
        const int idx = threadIdx.x + v * PC_THREADS;
        if (idx < nvec) *reinterpret_cast<short8*>(&raw[idx * 8]) = pre[v];
    }
    if ((int)threadIdx.x < g.NR * P)
        heads[threadIdx.x] = pc_run<P, C>(g, t, threadIdx.x, false).head;
}

// Where pixel m of the tile sits in the slot image: base[r] is the element
// of its tap row r
template <int P, int C>
__device__ __forceinline__ void pc_pixel(const PGeom& g, const PTile& t,
                                         const int* heads, int m, int base[P]) {
    const int gr = m / g.Wo, wo = m - gr * g.Wo;
    const int row = gr - t.grow0;
    const int wo_s = row == 0 ? t.wof : 0;
#pragma unroll
    for (int r = 0; r < P; ++r)
        base[r] = (row * P + r) * g.SL + heads[row * P + r] +
                  (wo - wo_s) * P * C;
}

template <int P>
__device__ __forceinline__ int pc_pick(const int base[P], int r) {
    int b = base[0];
#pragma unroll
    for (int i = 1; i < P; ++i) b = r == i ? base[i] : b;
    return b;
}

// raw runs -> At[TM][KP + 8]: X' of the tile, zeros past KD and past mend
template <int P, int C>
__device__ __forceinline__ void pc_repack(const uint16_t* raw,
                                          const int* heads, uint16_t* At,
                                          const PGeom& g, const PTile& t) {
    constexpr int PCN = P * C, KD = P * PCN, KP = (KD + 31) / 32 * 32;
    constexpr int AP = KP + 8;
    const int tpp = PC_THREADS / g.TM;
    const int i = threadIdx.x / tpp, sub = threadIdx.x - i * tpp;
    const int m = t.m0 + i;
    int base[P];
#pragma unroll
    for (int r = 0; r < P; ++r) base[r] = 0;
    if (m < t.mend) pc_pixel<P, C>(g, t, heads, m, base);
    for (int pair = sub; pair < KP / 2; pair += tpp) {
        const int kk = 2 * pair;
        uint32_t v = 0;
        if (m < t.mend && kk < KD) {
            const int r = kk / PCN, tt = kk - r * PCN;
            const int b = pc_pick<P>(base, r) + tt;
            v = (uint32_t)raw[b] | ((uint32_t)raw[b + 1] << 16);
        }
        *reinterpret_cast<uint32_t*>(&At[i * AP + kk]) = v;
    }
}

// y[M][K] = X' * W^T
template <int P, int C>
__global__ void __launch_bounds__(PC_THREADS)
k_patchconv_fwd(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
                uint16_t* __restrict__ y, PGeom g) {
    constexpr int KD = P * P * C, KP = (KD + 31) / 32 * 32, KS = KP / 32;
    constexpr int AP = KP + 8;
    extern __shared__ __attribute__((aligned(16))) uint16_t pc_lds[];
    uint16_t* const raw = pc_lds;
    uint16_t* const At = raw + g.NR * P * g.SL;
    uint16_t* const ost = At + g.TM * AP;
    int* const heads = reinterpret_cast<int*>(ost + g.TM * g.K);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int ntl = g.K >> 4;
    const int my_nt = (ntl - wid + 3) >> 2;

    // this wave's filters as B fragments: B[kk][col] = W[col][kk]
    short8 wb[8][KS];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            short8 v = {};
            if (a < my_nt) {
                const int k = (wid + 4 * a) * 16 + l15;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int kk = ks * 32 + lq * 8 + j;
                    if (kk < KD) v[j] = (short)w[(int64_t)k * KD + kk];
                }
            }
            wb[a][ks] = v;
        }

    short8 pre[PC_NV];
    PTile t = pc_tile(g, blockIdx.x);
    pc_load_x<P, C>(x, g, t, pre);
    for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        pc_store_x<P, C>(raw, heads, g, t, pre);
        pc_barrier();
        const PTile tn = pc_tile(g, tile + gridDim.x);
        pc_load_x<P, C>(x, g, tn, pre);    // in flight under the work below
        pc_repack<P, C>(raw, heads, At, g, t);
        pc_barrier();
        for (int ms = 0; ms < g.TM / 16; ++ms) {
            short8 af[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                af[ks] = *reinterpret_cast<const short8*>(
                    &At[(ms * 16 + l15) * AP + ks * 32 + lq * 8]);
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                if (a < my_nt) {
                    floatx4 acc = {};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        acc = MFMA_BF16(af[ks], wb[a][ks], acc);
                    const int col = (wid + 4 * a) * 16 + l15;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr)
                        ost[(ms * 16 + lq * 4 + rr) * g.K + col] =
                            f32_to_bf16(acc[rr]);
                }
            }
        }
        pc_barrier();
        // the tile's [pixels][K] output is one contiguous run of y
        const int nv = (t.mend - t.m0) * (g.K >> 3);
        uint16_t* const dst = y + (int64_t)t.m0 * g.K;
        for (int idx = tid; idx < nv; idx += PC_THREADS)
            *reinterpret_cast<short8*>(dst + (int64_t)idx * 8) =
                *reinterpret_cast<const short8*>(&ost[idx * 8]);
        t = tn;
    }
}

// Issue the loads of the tile's dy rows, [TM][K] contiguous; zeros past mend
__device__ __forceinline__ void pc_load_dy(const uint16_t* __restrict__ dy,
                                           const PGeom& g, const PTile& t,
                                           short8* dpre) {
    const int kv = g.K >> 3, nv = (t.mend - t.m0) * kv;
    const uint16_t* const src = dy + (int64_t)t.m0 * g.K;
#pragma unroll
    for (int v = 0; v < PC_DV; ++v) {
        const int idx = threadIdx.x + v * PC_THREADS;
        short8 val = {};
        if (idx < nv) val = *reinterpret_cast<const short8*>(src + (int64_t)idx * 8);
        dpre[v] = val;
    }
}

// into dyT[TM][pitch]
__device__ __forceinline__ void pc_store_dy(uint16_t* dyT, int pitch,
                                            const PGeom& g,
                                            const short8* dpre) {
    const int kv = g.K >> 3, nv = g.TM * kv;
#pragma unroll
    for (int v = 0; v < PC_DV; ++v) {
        const int idx = threadIdx.x + v * PC_THREADS;
        if (idx < nv) {
            const int i = idx / kv, c = idx - i * kv;
            *reinterpret_cast<short8*>(&dyT[i * pitch + c * 8]) = dpre[v];
        }
    }
}

// dx: every element of [N][H][W][C] is written exactly once
template <int P, int C>
__global__ void __launch_bounds__(PC_THREADS)
k_patchconv_dgrad(const uint16_t* __restrict__ dy,
                  const uint16_t* __restrict__ w, uint16_t* __restrict__ dx,
                  PGeom g) {
    constexpr int PCN = P * C, KD = P * PCN, NT = (KD + 15) / 16;
    constexpr int G = 4 / NT;      // pixel sub-tile groups of waves
    extern __shared__ __attribute__((aligned(16))) uint16_t pc_lds[];
    const int K32 = (g.K + 31) / 32 * 32, KA = K32 + 8, KS = K32 / 32;
    uint16_t* const stg = pc_lds;                 // [NR * P][SL], as runs
    uint16_t* const dyT = stg + g.NR * P * g.SL;  // [TM][KA]
    int* const heads = reinterpret_cast<int*>(dyT + g.TM * KA);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int nt = wid % NT, mg = wid / NT;
    const int vpr = g.SL >> 3, nvec = g.NR * P * vpr;

    // B[k][col] = W[k][nt * 16 + col] for every k, zeros past K and KD
    short8 wb[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        short8 v = {};
        const int col = nt * 16 + l15;
        if (ks < KS && mg < G && col < KD) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = ks * 32 + lq * 8 + j;
                if (k < g.K) v[j] = (short)w[(int64_t)k * KD + col];
            }
        }
        wb[ks] = v;
    }
    // the zero columns K..K32 of dyT: nothing writes there again
    if (K32 != g.K)
        for (int idx = tid; idx < g.TM * 2; idx += PC_THREADS)
            *reinterpret_cast<short8*>(
                &dyT[(idx >> 1) * KA + g.K + (idx & 1) * 8]) = short8{};

    short8 dpre[PC_DV];
    PTile t = pc_tile(g, blockIdx.x);
    pc_load_dy(dy, g, t, dpre);
    for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        pc_store_dy(dyT, KA, g, dpre);
        for (int idx = tid; idx < nvec; idx += PC_THREADS)
            *reinterpret_cast<short8*>(&stg[idx * 8]) = short8{};
        if (tid < g.NR * P)
            heads[tid] = pc_run<P, C>(g, t, tid, true).head;
        pc_barrier();
        const PTile tn = pc_tile(g, tile + gridDim.x);
        pc_load_dy(dy, g, tn, dpre);       // in flight under the work below
        if (mg < G) {
            for (int ms = mg; ms < g.TM / 16; ms += G) {
                floatx4 acc = {};
#pragma unroll
                for (int ks = 0; ks < 16; ++ks)
                    if (ks < KS)
                        acc = MFMA_BF16(
                            *reinterpret_cast<const short8*>(
                                &dyT[(ms * 16 + l15) * KA + ks * 32 + lq * 8]),
                            wb[ks], acc);
                const int kk = nt * 16 + l15;
                const int r = kk / PCN, tt = kk - r * PCN;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int m = t.m0 + ms * 16 + lq * 4 + rr;
                    if (m < t.mend && kk < KD) {
                        int base[P];
                        pc_pixel<P, C>(g, t, heads, m, base);
                        stg[pc_pick<P>(base, r) + tt] = f32_to_bf16(acc[rr]);
                    }
                }
            }
        }
        pc_barrier();
        // the runs leave: whole 16-byte lanes inside, elements at the ends
        for (int idx = tid; idx < nvec; idx += PC_THREADS) {
            const int run = idx / vpr, j = idx - run * vpr;
            const PRun o = pc_run<P, C>(g, t, run, true);
            const int lo = 8 * j, end = o.head + o.len;
            if (o.len == 0 || lo >= end || lo + 8 <= o.head) continue;
            uint16_t* const dst = dx + o.a0 + lo;
            if (lo >= o.head && lo + 8 <= end) {
                *reinterpret_cast<short8*>(dst) =
                    *reinterpret_cast<const short8*>(&stg[idx * 8]);
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (lo + c >= o.head && lo + c < end)
                        dst[c] = stg[idx * 8 + c];
            }
        }
        // rows no patch covers, for every image whose last pixel is here
        if (g.H != g.Ho * P) {
            const int hw = g.Ho * g.Wo;
            const int span = (g.H - g.Ho * P) * g.W * C;
            for (int n = t.m0 / hw; n < (t.mend + hw - 1) / hw; ++n) {
                if ((n + 1) * hw > t.mend) break;
                uint16_t* const dst =
                    dx + ((int64_t)n * g.H + g.Ho * P) * g.W * C;
                for (int i = tid; i < span; i += PC_THREADS) dst[i] = 0;
            }
        }
        pc_barrier();       // stg and dyT are free again
        t = tn;
    }
}

// 16 rows (filters or columns at `p`, 4 contiguous per lane) x 32 pixels of a
// pixel-major LDS tile, transposed by the read: the lane ends with its row's
// 8 consecutive pixels (conv_wgrad.hip)
__device__ __forceinline__ short8 pc_tr_frag(const uint16_t* p, int pitch) {
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

// ws: fp32 [nsplit][K][KD]; block b reduces tiles [b * tps, (b + 1) * tps)
template <int P, int C>
__global__ void __launch_bounds__(PC_THREADS)
k_patchconv_wgrad(const uint16_t* __restrict__ x,
                  const uint16_t* __restrict__ dy, float* __restrict__ ws,
                  PGeom g, int tps) {
    constexpr int KD = P * P * C, KP = (KD + 31) / 32 * 32, AP = KP + 8;
    constexpr int NT = (KD + 15) / 16;
    extern __shared__ __attribute__((aligned(16))) uint16_t pc_lds[];
    const int DP = g.K + 8;
    uint16_t* const raw = pc_lds;
    uint16_t* const At = raw + g.NR * P * g.SL;
    uint16_t* const dyT = At + g.TM * AP;         // [TM][DP]
    int* const heads = reinterpret_cast<int*>(dyT + g.TM * DP);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int my_kt = ((g.K >> 4) - wid + 3) >> 2;
    // this lane's read of a transposed fragment: pixel row, 4-element column
    const int tr_row = lq * 8 + (l15 >> 2), tr_col = 4 * (lane & 3);

    floatx4 acc[8][NT];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[a][n] = floatx4{};

    const int t0 = blockIdx.x * tps, t1 = pc_min(t0 + tps, g.ntiles);
    short8 pre[PC_NV], dpre[PC_DV];
    PTile t = pc_tile(g, t0);
    pc_load_x<P, C>(x, g, t, pre);
    pc_load_dy(dy, g, t, dpre);
    for (int tile = t0; tile < t1; ++tile) {
        pc_store_x<P, C>(raw, heads, g, t, pre);
        pc_store_dy(dyT, DP, g, dpre);
        pc_barrier();
        const PTile tn = pc_tile(g, tile + 1 < t1 ? tile + 1 : g.ntiles);
        pc_load_x<P, C>(x, g, tn, pre);
        pc_load_dy(dy, g, tn, dpre);
        pc_repack<P, C>(raw, heads, At, g, t);
        pc_barrier();
        for (int sc = 0; sc < g.TM / 32; ++sc) {
            short8 bf[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n)
                bf[n] = pc_tr_frag(
                    &At[(sc * 32 + tr_row) * AP + n * 16 + tr_col], AP);
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                if (a < my_kt) {
                    const short8 af = pc_tr_frag(
                        &dyT[(sc * 32 + tr_row) * DP + (wid + 4 * a) * 16 +
                             tr_col], DP);
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        acc[a][n] = MFMA_BF16(af, bf[n], acc[a][n]);
                }
            }
        }
        pc_barrier();       // the tiles are free again
        t = tn;
    }
    float* const slice = ws + (int64_t)blockIdx.x * g.K * KD;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        if (a < my_kt) {
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int kk = n * 16 + l15;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int k = (wid + 4 * a) * 16 + lq * 4 + rr;
                    if (kk < KD) slice[(int64_t)k * KD + kk] = acc[a][n][rr];
                }
            }
        }
    }
}

// dw[i] += ws[0][i] + ws[1][i] + ..., summed in split order
__global__ void k_patchconv_wgrad_combine(const float* __restrict__ ws,
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
#define PC_DISPATCH(CALL)                                   \
    do {                                                    \
        if (d.R == 4 && d.C == 3) { CALL(4, 3); }           \
        else if (d.R == 4) { CALL(4, 4); }                  \
        else if (d.C == 3) { CALL(2, 3); }                  \
        else { CALL(2, 4); }                                \
    } while (0)

// w16: bf16 [K][p][p][C].  Each launcher returns 0 (nothing launched) where
// patchconv_plan declines the shape.
extern "C" int launch_patchconv_fwd(const void* x, const void* w16, void* y,
                                    ConvDims d, hipStream_t stream) {
    int splits;
    if (!patchconv_plan(d, &splits)) return 0;
    const PGeom g = pc_geom(d, false);
    const int grid = g.ntiles < PC_MAXGRID ? g.ntiles : PC_MAXGRID;
    const size_t lds = ((size_t)g.NR * d.R * g.SL + (size_t)g.TM * (pc_kp(d) + 8) +
                        (size_t)g.TM * d.K) * 2 + (size_t)g.NR * d.R * 4;
#define PC_CALL(P, C)                                                       \
    k_patchconv_fwd<P, C><<<grid, PC_THREADS, lds, stream>>>(               \
        (const uint16_t*)x, (const uint16_t*)w16, (uint16_t*)y, g)
    PC_DISPATCH(PC_CALL);
#undef PC_CALL
    return 1;
}

extern "C" int launch_patchconv_dgrad(const void* dy, const void* w16,
                                      void* dx, ConvDims d,
                                      hipStream_t stream) {
    int splits;
    if (!patchconv_plan(d, &splits)) return 0;
    const PGeom g = pc_geom(d, false);
    const int grid = g.ntiles < PC_MAXGRID ? g.ntiles : PC_MAXGRID;
    const int ka = (d.K + 31) / 32 * 32 + 8;
    const size_t lds = ((size_t)g.NR * d.R * g.SL + (size_t)g.TM * ka) * 2 +
                       (size_t)g.NR * d.R * 4;
#define PC_CALL(P, C)                                                       \
    k_patchconv_dgrad<P, C><<<grid, PC_THREADS, lds, stream>>>(             \
        (const uint16_t*)dy, (const uint16_t*)w16, (uint16_t*)dx, g)
    PC_DISPATCH(PC_CALL);
#undef PC_CALL
    return 1;
}

// ws: fp32 [splits][K][p*p*C] with splits from patchconv_plan; dw += their sum
extern "C" int launch_patchconv_wgrad(const void* x, const void* dy, void* ws,
                                      void* dw, ConvDims d,
                                      hipStream_t stream) {
    int nsplit;
    if (!patchconv_plan(d, &nsplit)) return 0;
    const PGeom g = pc_geom(d, true);
    int tps;
    pc_wgrad_split(g, &tps, &nsplit);
    const size_t lds = ((size_t)g.NR * d.R * g.SL + (size_t)g.TM * (pc_kp(d) + 8) +
                        (size_t)g.TM * (d.K + 8)) * 2 + (size_t)g.NR * d.R * 4;
#define PC_CALL(P, C)                                                       \
    k_patchconv_wgrad<P, C><<<nsplit, PC_THREADS, lds, stream>>>(           \
        (const uint16_t*)x, (const uint16_t*)dy, (float*)ws, g, tps)
    PC_DISPATCH(PC_CALL);
#undef PC_CALL
    const int n = d.K * d.R * d.R * d.C;
    k_patchconv_wgrad_combine<<<ew_grid(n, 256, 1), 256, 0, stream>>>(
        (const float*)ws, (float*)dw, n, nsplit);
    return 1;
}

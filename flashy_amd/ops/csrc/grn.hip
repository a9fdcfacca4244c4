// Copyright (c) Flashy-AMD authors.
// Global response normalization (ConvNeXt V2) over contiguous NHWC bf16
// [N][HW][C] activations for gfx950, forward and backward, and the bias+GELU
// forward that gathers GRN's sums of squares on its own walk.  gamma, beta and
// their gradients are fp32, all arithmetic is fp32, every stored activation is
// rounded to bf16 once.  grn_plan() below is the only place that decides.
//
//   S[n,c] = sum_hw x^2      Gx = sqrt(S)      mu[n] = mean_c Gx
//   Nx = Gx / (mu + eps)     a = 1 + gamma * Nx      out = a * x + beta
//
//   P[n,c] = sum_hw dout * x                   Q[n,c] = sum_hw dout
//   dbeta = sum_n Q    dgamma = sum_n Nx * P   dNx = gamma * P
//   b = (dNx - mean_c(dNx * Nx)) / ((mu + eps)^2 * Nx), 0 where Nx == 0
//   dx = a * dout + b * x
//
// b is dGx / Gx of the textbook form with Gx written as Nx * (mu + eps), so
// backward needs Nx, a and 1 / (mu + eps) besides x and never Gx itself.
//
// GRN is neither a row pass nor a batch column pass: it reduces over the
// pixels of ONE image per channel, then over the channels of that image.  So
// it runs as three launches each way, and the two that touch the activation
// are bound by traffic exactly as the elementwise families of layernorm.hip:
//
//   sums   grid (slices, N, chunks)   x [, dout] -> fp32 slices of S / (P, Q)
//   coef   grid (N)                   slices -> the per-(n, c) coefficients
//   apply  grid (slices, N, chunks)   out = a * x + beta / dx = a * dout + b * x
//
// Thread layout of sums and apply (256 threads): that of layernorm.hip's
// elementwise kernels.  A lane owns a channel octet (one 16-byte load or
// store), a row is served by a lane group of G = the smallest power of two
// >= min(C, 512) / 8, a block holds RB = 256 / G rows at once, and rows wider
// than 512 channels are cut into column chunks on grid.z.  What differs is the
// walk: a block walks the contiguous rows [s * rpb, (s + 1) * rpb) of image
// blockIdx.y only, so no block straddles an image, and the coefficients of its
// (n, octet) sit in registers for the whole walk.  Images beyond the 65535
// that grid.y can carry are reached by striding over n.
//
// Sums: a thread keeps fp32 accumulators for its octet over the rows it
// visits, the threads of equal octet fold through LDS in row-slot order, and
// the block writes one fp32 slice [k][C] of ws[n][slice] (k = 1 forward, 2
// backward).  No atomics, no last-block fan-in, no spin-wait; bitwise
// repeatable.  k_bias_gelu_sqsum is k_bias_gelu_fwd on this walk with the
// accumulators of k_grn_sqsum fed from the bf16-rounded g it stores: its g is
// bitwise that of k_bias_gelu_fwd, its slices bitwise those of k_grn_sqsum on
// that g, and the hidden tensor is read once less.
//
// coef: one block per image, a thread owns channels tid, tid + 256, ... (at
// most 16).  It adds the image's slices in slice order, and reduces over C in
// a fixed order: each thread its own channels in channel order, then a
// halving tree over the 256 partials in LDS.  The backward one also writes
// the image's (Nx * P, Q) as one [2][C] slice of a workspace [N][2][C], which
// k_colsum_combine of layernorm.hip adds into dgamma / dbeta with slices = N.
//
// Zeros: sqrt(0) = 0 and mu + eps > 0, so a channel that is zero over an
// image has Nx = 0 and b = 0 (torch.norm's subgradient), and an all-zero
// image has mu = 0, Nx = 0 / eps = 0; nothing divides by zero.
//
// Unmeasured: everything.  In particular the serial chain over up to 1024
// slices in coef when N is small and HW large (one block per image), whether
// saving a (N * C floats) beats recomputing it from Nx and gamma, and the
// slice traffic (1 or 2 / rpb of the activation bytes) against filling the
// chip when N * chunks is small.

#include "rowops.h"

#define GRN_BLOCKS 1024         // walk blocks aimed at: 4 per CU of 256
#define GRN_MINROWS 16          // floor on rows per block
#define GRN_MAXC 4096           // the pointwise kernels' widest output
#define GRN_PT (GRN_MAXC / LN_THREADS)  // channels of one coef thread
#define GRN_MAXY 65535          // grid.y

struct GrnGeom {
    int N, HW, C;
    int G;      // lanes per row
    int rpb;    // rows per block (a multiple of 256 / G)
};

// Dims-only plan.  Returns 1 where [N, HW, C] is served: C % 8 == 0,
// 8 <= C <= 4096, at least one image of at least one pixel.
// out = {lanes per row, rows per block, slices per image, column chunks}; the
// walk kernels run on grid (slices, min(N, 65535), chunks), coef on (N).
extern "C" int grn_plan(int N, int HW, int C, int* out) {
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (N < 1 || HW < 1 || C < 8 || C % 8 != 0 || C > GRN_MAXC) return 0;
    const int chunks = (C + LN_CHUNK - 1) / LN_CHUNK;
    const int nvec = (C < LN_CHUNK ? C : LN_CHUNK) / 8;
    int G = 1;
    while (G < nvec && G < LN_MAXG) G *= 2;
    const int RB = LN_THREADS / G;
    const int64_t per_slice = (int64_t)N * chunks;
    const int want = per_slice >= GRN_BLOCKS ? 1 : (int)(GRN_BLOCKS / per_slice);
    int64_t rpb = ((int64_t)HW + want - 1) / want;
    rpb = (rpb + RB - 1) / RB * RB;
    const int floor_rows = RB > GRN_MINROWS ? RB : GRN_MINROWS;
    if (rpb < floor_rows) rpb = floor_rows;
    out[0] = G;
    out[1] = (int)rpb;
    out[2] = (int)(((int64_t)HW + rpb - 1) / rpb);
    out[3] = chunks;
    return 1;
}

static bool grn_geom(int N, int HW, int C, GrnGeom* g, dim3* grid) {
    int p[4];
    if (!grn_plan(N, HW, C, p)) return false;
    g->N = N; g->HW = HW; g->C = C; g->G = p[0]; g->rpb = p[1];
    *grid = dim3(p[2], N < GRN_MAXY ? N : GRN_MAXY, p[3]);
    return true;
}

// Compiled without packed fp32 math, as layernorm.hip (see fused_optim.hip
// for why).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// The walk of one thread inside one image: its group lane, its row slot, its
// octet and its rows [row, rend) of the image, RB apart.
struct GrnWalk {
    int lig, rslot, RB, col0, ch;
    bool on;
    int64_t row, rend;      // 64-bit: row + RB may pass 2^31 at the last rows
    __device__ __forceinline__ GrnWalk(const GrnGeom& g) {
        const int tid = threadIdx.x;
        lig = tid & (g.G - 1);
        rslot = tid / g.G;
        RB = LN_THREADS / g.G;
        col0 = blockIdx.z * LN_CHUNK;
        ch = col0 + lig * 8;
        on = ch < g.C;
        const int64_t r0 = (int64_t)blockIdx.x * g.rpb;
        row = r0 + rslot;
        rend = r0 + g.rpb < g.HW ? r0 + g.rpb : g.HW;
    }
    // element offset of this thread's octet in row r of image n
    __device__ __forceinline__ int64_t at(const GrnGeom& g, int n,
                                           int64_t r) const {
        return ((int64_t)n * g.HW + r) * g.C + ch;
    }
};

// Fold one column sum of the block: acc[c] of every thread -> red [RB][G * 8]
// -> the sum over the row slots, in slot order, into dst[C].
__device__ __forceinline__ void grn_fold(float* red, const float acc[8],
                                         float* __restrict__ dst,
                                         const GrnWalk& w, const GrnGeom& g) {
    const int ncols = g.G * 8;
    ln_barrier();       // the previous fold's reads are done
#pragma unroll
    for (int c = 0; c < 8; ++c)
        red[w.rslot * ncols + w.lig * 8 + c] = acc[c];
    ln_barrier();
    for (int idx = threadIdx.x; idx < ncols; idx += LN_THREADS) {
        float s = red[idx];
        for (int r = 1; r < w.RB; ++r) s += red[r * ncols + idx];
        if (w.col0 + idx < g.C) dst[w.col0 + idx] = s;
    }
}

// the sum of v over the block in a fixed order: a halving tree over tid
__device__ __forceinline__ float grn_block_sum(float* red, float v) {
    const int tid = threadIdx.x;
    red[tid] = v;
    ln_barrier();
    for (int s = LN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        ln_barrier();
    }
    return red[0];
}

// ws[n][slice][C] = the column sums of x^2 over the slice's rows of image n
__global__ void __launch_bounds__(LN_THREADS)
k_grn_sqsum(const uint16_t* __restrict__ x, float* __restrict__ ws, GrnGeom g) {
    __shared__ float red[LN_THREADS * 8];
    const GrnWalk w(g);
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.f;
        if (w.on) {
            for (int64_t r = w.row; r < w.rend; r += w.RB) {
                float f[8];
                ln_load8(x, w.at(g, n, r), f);
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    acc[c] = __builtin_fmaf(f[c], f[c], acc[c]);
            }
        }
        grn_fold(red, acc,
                 ws + ((int64_t)n * gridDim.x + blockIdx.x) * g.C, w, g);
    }
}

// out = gelu(h + b) as k_bias_gelu_fwd gives it; ws as k_grn_sqsum on out
__global__ void __launch_bounds__(LN_THREADS)
k_bias_gelu_sqsum(const uint16_t* __restrict__ h, const float* __restrict__ b,
                  uint16_t* __restrict__ out, float* __restrict__ ws,
                  GrnGeom g) {
    __shared__ float red[LN_THREADS * 8];
    const GrnWalk w(g);
    float bi[8];
    ln_param8(b, w.ch, w.on, 0.f, bi);
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.f;
        if (w.on) {
            for (int64_t r = w.row; r < w.rend; r += w.RB) {
                const int64_t at = w.at(g, n, r);
                float f[8];
                ln_load8(h, at, f);
                short8 v;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float u = f[c] + bi[c];
                    float Phi, phi;
                    ln_gauss(u, &Phi, &phi);
                    const uint16_t q = f32_to_bf16(u * Phi);
                    v[c] = (short)q;
                    const float gq = bf16_to_f32(q);    // what is stored
                    acc[c] = __builtin_fmaf(gq, gq, acc[c]);
                }
                *reinterpret_cast<short8*>(out + at) = v;
            }
        }
        grn_fold(red, acc,
                 ws + ((int64_t)n * gridDim.x + blockIdx.x) * g.C, w, g);
    }
}

// One block per image: S = the slices of ws in slice order, Gx = sqrt(S),
// mu = mean_c Gx, rden[n] = 1 / (mu + eps), nx = Gx * rden, a = 1 + gamma * nx
__global__ void __launch_bounds__(LN_THREADS)
k_grn_coef(const float* __restrict__ ws, const float* __restrict__ gamma,
           float* __restrict__ nx, float* __restrict__ a,
           float* __restrict__ rden, int C, int slices, float eps) {
    __shared__ float red[LN_THREADS];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* const img = ws + (int64_t)n * slices * C;
    float gx[GRN_PT];
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < GRN_PT; ++j) {
        const int c = tid + j * LN_THREADS;
        float s = 0.f;
        if (c < C)
            for (int z = 0; z < slices; ++z) s += img[(int64_t)z * C + c];
        gx[j] = __builtin_sqrtf(s);
        part += gx[j];
    }
    const float mu = grn_block_sum(red, part) / (float)C;
    const float r = 1.f / (mu + eps);
    if (tid == 0) rden[n] = r;
#pragma unroll
    for (int j = 0; j < GRN_PT; ++j) {
        const int c = tid + j * LN_THREADS;
        if (c < C) {
            const float v = gx[j] * r;
            nx[(int64_t)n * C + c] = v;
            a[(int64_t)n * C + c] = __builtin_fmaf(gamma[c], v, 1.f);
        }
    }
}

// out = a[n] * x + beta
__global__ void __launch_bounds__(LN_THREADS)
k_grn_apply(const uint16_t* __restrict__ x, const float* __restrict__ a,
            const float* __restrict__ beta, uint16_t* __restrict__ out,
            GrnGeom g) {
    const GrnWalk w(g);
    if (!w.on) return;
    float be[8];
    ln_param8(beta, w.ch, true, 0.f, be);
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
        float an[8];
        ln_param8(a + (int64_t)n * g.C, w.ch, true, 0.f, an);
        for (int64_t r = w.row; r < w.rend; r += w.RB) {
            const int64_t at = w.at(g, n, r);
            float f[8];
            ln_load8(x, at, f);
#pragma unroll
            for (int c = 0; c < 8; ++c)
                f[c] = __builtin_fmaf(an[c], f[c], be[c]);
            ln_store8(out, at, f);
        }
    }
}

// ws[n][slice][2][C] = the column sums of dout * x and of dout
__global__ void __launch_bounds__(LN_THREADS)
k_grn_bwd_sums(const uint16_t* __restrict__ dout,
               const uint16_t* __restrict__ x, float* __restrict__ ws,
               GrnGeom g) {
    __shared__ float red[LN_THREADS * 8];
    const GrnWalk w(g);
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
        float a_p[8], a_q[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) a_p[c] = a_q[c] = 0.f;
        if (w.on) {
            for (int64_t r = w.row; r < w.rend; r += w.RB) {
                const int64_t at = w.at(g, n, r);
                float f[8], d[8];
                ln_load8(x, at, f);
                ln_load8(dout, at, d);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    a_p[c] = __builtin_fmaf(d[c], f[c], a_p[c]);
                    a_q[c] += d[c];
                }
            }
        }
        float* const slice =
            ws + ((int64_t)n * gridDim.x + blockIdx.x) * 2 * g.C;
        grn_fold(red, a_p, slice, w, g);
        grn_fold(red, a_q, slice + g.C, w, g);
    }
}

// One block per image: (P, Q) = the slices of ws in slice order,
// t = sum_c gamma * P * nx, b = rden^2 * (gamma * P - t / C) / nx (0 where
// nx == 0), pq[n] = (nx * P, Q): slice n of the parameter gradients' combine
__global__ void __launch_bounds__(LN_THREADS)
k_grn_bwd_coef(const float* __restrict__ ws, const float* __restrict__ gamma,
               const float* __restrict__ nx, const float* __restrict__ rden,
               float* __restrict__ b, float* __restrict__ pq, int C,
               int slices) {
    __shared__ float red[LN_THREADS];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* const img = ws + (int64_t)n * slices * 2 * C;
    float dnx[GRN_PT], nxr[GRN_PT];
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < GRN_PT; ++j) {
        const int c = tid + j * LN_THREADS;
        dnx[j] = nxr[j] = 0.f;
        if (c < C) {
            float p = 0.f, q = 0.f;
            for (int z = 0; z < slices; ++z) {
                p += img[(int64_t)z * 2 * C + c];
                q += img[(int64_t)z * 2 * C + C + c];
            }
            nxr[j] = nx[(int64_t)n * C + c];
            dnx[j] = gamma[c] * p;
            pq[(int64_t)n * 2 * C + c] = nxr[j] * p;
            pq[(int64_t)n * 2 * C + C + c] = q;
        }
        part = __builtin_fmaf(dnx[j], nxr[j], part);
    }
    const float m = grn_block_sum(red, part) / (float)C;
    const float r = rden[n];
    const float r2 = r * r;
#pragma unroll
    for (int j = 0; j < GRN_PT; ++j) {
        const int c = tid + j * LN_THREADS;
        if (c < C)
            b[(int64_t)n * C + c] =
                nxr[j] > 0.f ? r2 * (dnx[j] - m) / nxr[j] : 0.f;
    }
}

// dx = a[n] * dout + b[n] * x
__global__ void __launch_bounds__(LN_THREADS)
k_grn_bwd_apply(const uint16_t* __restrict__ dout,
                const uint16_t* __restrict__ x, const float* __restrict__ a,
                const float* __restrict__ b, uint16_t* __restrict__ dx,
                GrnGeom g) {
    const GrnWalk w(g);
    if (!w.on) return;
    for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
        float an[8], bn[8];
        ln_param8(a + (int64_t)n * g.C, w.ch, true, 0.f, an);
        ln_param8(b + (int64_t)n * g.C, w.ch, true, 0.f, bn);
        for (int64_t r = w.row; r < w.rend; r += w.RB) {
            const int64_t at = w.at(g, n, r);
            float f[8], d[8];
            ln_load8(x, at, f);
            ln_load8(dout, at, d);
#pragma unroll
            for (int c = 0; c < 8; ++c)
                d[c] = __builtin_fmaf(an[c], d[c], bn[c] * f[c]);
            ln_store8(dx, at, d);
        }
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// Activations: contiguous bf16 [N][HW][C], 16-byte aligned.  gamma, beta and
// the gradient targets: fp32 [C].  nx, a, b: fp32 [N][C]; rden: fp32 [N].
// Each launcher returns 0 (nothing launched) where grn_plan declines.

// ws: fp32 [N][slices][C]
extern "C" int launch_grn_sqsum(const void* x, void* ws, int N, int HW, int C,
                                hipStream_t stream) {
    GrnGeom g; dim3 grid;
    if (!grn_geom(N, HW, C, &g, &grid)) return 0;
    k_grn_sqsum<<<grid, LN_THREADS, 0, stream>>>((const uint16_t*)x,
                                                 (float*)ws, g);
    return 1;
}

// out = gelu(h + b); ws: fp32 [N][slices][C], the sums of squares of out
extern "C" int launch_bias_gelu_sqsum(const void* h, const void* b, void* out,
                                      void* ws, int N, int HW, int C,
                                      hipStream_t stream) {
    GrnGeom g; dim3 grid;
    if (!grn_geom(N, HW, C, &g, &grid)) return 0;
    k_bias_gelu_sqsum<<<grid, LN_THREADS, 0, stream>>>(
        (const uint16_t*)h, (const float*)b, (uint16_t*)out, (float*)ws, g);
    return 1;
}

// From the slices ws of x (either kernel above): the coefficients nx, a,
// rden, then out = a * x + beta.
extern "C" int launch_grn_fwd(const void* x, const void* ws, const void* gamma,
                              const void* beta, void* out, void* nx, void* a,
                              void* rden, int N, int HW, int C, float eps,
                              hipStream_t stream) {
    GrnGeom g; dim3 grid;
    if (!grn_geom(N, HW, C, &g, &grid)) return 0;
    k_grn_coef<<<N, LN_THREADS, 0, stream>>>(
        (const float*)ws, (const float*)gamma, (float*)nx, (float*)a,
        (float*)rden, C, (int)grid.x, eps);
    k_grn_apply<<<grid, LN_THREADS, 0, stream>>>(
        (const uint16_t*)x, (const float*)a, (const float*)beta,
        (uint16_t*)out, g);
    return 1;
}

// ws: fp32 [N][slices][2][C]; pq: fp32 [N][2][C]; b: fp32 [N][C].  dx and
// each of dgamma / dbeta may be null; the gradient targets are accumulated
// into.
extern "C" int launch_grn_bwd(const void* dout, const void* x, const void* nx,
                              const void* a, const void* rden,
                              const void* gamma, void* dx, void* ws, void* pq,
                              void* b, void* dgamma, void* dbeta, int N,
                              int HW, int C, hipStream_t stream) {
    GrnGeom g; dim3 grid;
    if (!grn_geom(N, HW, C, &g, &grid)) return 0;
    if (!dx && !dgamma && !dbeta) return 1;
    k_grn_bwd_sums<<<grid, LN_THREADS, 0, stream>>>(
        (const uint16_t*)dout, (const uint16_t*)x, (float*)ws, g);
    k_grn_bwd_coef<<<N, LN_THREADS, 0, stream>>>(
        (const float*)ws, (const float*)gamma, (const float*)nx,
        (const float*)rden, (float*)b, (float*)pq, C, (int)grid.x);
    if (dx)
        k_grn_bwd_apply<<<grid, LN_THREADS, 0, stream>>>(
            (const uint16_t*)dout, (const uint16_t*)x, (const float*)a,
            (const float*)b, (uint16_t*)dx, g);
    if (dgamma || dbeta) ln_combine(pq, dgamma, dbeta, nullptr, 2, C, N, stream);
    return 1;
}

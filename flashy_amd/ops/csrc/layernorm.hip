// Copyright (c) Flashy-AMD authors.
// Row and column passes over contiguous NHWC bf16 [M][C] activations for
// gfx950: LayerNorm over channels (with an optional folded input bias),
// bias + GELU (erf form) and layer scale + residual, each forward and
// backward, and the deterministic column sums their parameter gradients need.
// Parameters and their gradients are fp32, all arithmetic is fp32, every
// stored activation is rounded to bf16 once.  ln_plan() below is the only
// place that decides.
//
// Every kernel is bound by traffic: the design is about touching each byte
// once, in 16-byte lanes, and keeping a row's reduction out of LDS.
//
// Thread layout (256 threads): a lane owns a channel OCTET (8 bf16, one
// 16-byte load or store).  A row is served by a lane GROUP of G = the smallest
// power of two >= C / 8, at most 64, so a wave holds 64 / G rows at once and a
// block RB = 256 / G: C = 128 puts 4 rows in a wave, C = 96 uses 16-lane
// groups whose last 4 lanes load nothing and contribute zeros.  LayerNorm of
// 512 < C <= 1024 gives a lane two octets, l and l + 64 (the second one
// possibly absent): the template parameter NO.  The elementwise families have
// no row reduction, so wider rows are cut into 512-channel column chunks on
// grid.y instead and always run one octet per lane, whatever C is.
//
// Row reductions are xor butterflies over the G lanes of a group
// (ds_bpermute: the LDS crossbar, no LDS memory, no barrier).  Every lane of
// a group ends with the same bits, since each step adds the same two values
// in either order.  Groups never exchange data, so groups of one wave may run
// different trip counts (a ragged last block).
//
// A block walks the contiguous rows [b * rpb, (b + 1) * rpb), RB at a time;
// the per-channel parameters sit in registers for the whole walk.  LayerNorm
// forward keeps the row in registers and is TWO-PASS: the mean, then the sum
// of squared deviations from it, never E[x^2] - mean^2.
//
// LayerNorm backward does not take x + b - mean in one fp32 step.  Where the
// deviation is a hundredth of its operands, the roundings of x + b and of the
// saved fp32 mean (2^-25 of the operands each) are the whole error of the
// term dy * xhat of dgamma, and a column sum over a few rows shows it.  The
// kernel forms x + b - mean as an exact fp32 pair (two TwoSums), sums the
// pairs over the row with a compensated butterfly, which gives what the saved
// mean is off the row's own mean by, and takes that off: the deviation then
// carries one rounding of ITSELF.  Still fp32 arithmetic throughout; it costs
// about 25 adds per element and a third butterfly per row.
//
// Column sums (every backward): a thread keeps fp32 accumulators for its
// channels over all the rows it visits; at the end of the walk the threads of
// equal octet fold through LDS in row-slot order and the block writes one
// fp32 slice [k][C] of a workspace (k = 1..3 sums).  k_colsum_combine adds the
// slices and ACCUMULATES (+=) into the gradient buffers.  No atomics, no
// last-block fan-in, no spin-wait; bitwise repeatable.  One deviation from a
// plain walk in slice order: with up to 1024 slices a single serial chain per
// column would cost more than the pass it serves, so the combine sums 8
// contiguous RUNS of slices in slice order side by side and then adds the 8
// run totals in run order.  The shape of that tree depends on the slice
// count alone.
//
// erf has the shape of Abramowitz & Stegun 7.1.26, erfc(z) = exp(-z^2) *
// t * P(t) with t = 1 / (1 + 0.3275911 z), but P is a degree-9 least-squares
// fit of exp(z^2) erfc(z) for RELATIVE error on 0 <= z <= 10 (5e-9 in exact
// arithmetic, about 3e-7 as evaluated in fp32): the lower tail is formed as
// 0.5 * erfc(|z|) directly and stays accurate relative to itself, which the
// column sum of a strongly negative channel needs (the original A&S
// coefficients bound the absolute error only).  The library erff is not used
// because a function compiled without packed fp32 math (below) cannot inline
// it.
//
// Unmeasured: whether 4 blocks per CU with one row per group in flight keep
// enough loads outstanding (no row unrolling was tried), the cost of the
// butterfly against a DPP form, and the 16-row floor on rows per block, which
// trades slice traffic (2 / rpb of the activation bytes) against filling the
// chip at small M.

#include "rowops.h"

#define LN_BLOCKS 1024          // row blocks aimed at: 4 per CU of 256
#define LN_MINROWS 16           // floor on rows per block
#define LN_RUNS 8               // combine: runs of slices summed side by side
#define LN_RCOLS (LN_THREADS / LN_RUNS)

struct LnGeom {
    int M, C;
    int G;      // lanes per row
    int rpb;    // rows per block (a multiple of 256 / G)
};

// Dims-only plan.  Returns 0 where nothing serves [M, C], 1 where only the
// elementwise families do (C > 1024), 2 where LayerNorm does too.
// out = {lanes per row, rows per block, grid.x, column chunks (grid.y of the
// elementwise kernels), column-sum slices}.
extern "C" int ln_plan(int M, int C, int* out) {
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (M < 1 || C < 8 || C % 8 != 0) return 0;
    const int nvec = C / 8;
    int G = 1;
    while (G < nvec && G < LN_MAXG) G *= 2;
    const int RB = LN_THREADS / G;
    int rpb = (M + LN_BLOCKS - 1) / LN_BLOCKS;
    rpb = (rpb + RB - 1) / RB * RB;
    const int floor_rows = RB > LN_MINROWS ? RB : LN_MINROWS;
    if (rpb < floor_rows) rpb = floor_rows;
    const int grid = (int)(((int64_t)M + rpb - 1) / rpb);
    out[0] = G;
    out[1] = rpb;
    out[2] = grid;
    out[3] = (C + LN_CHUNK - 1) / LN_CHUNK;
    out[4] = grid;      // one slice per row block
    return C <= 2 * LN_CHUNK ? 2 : 1;
}

static bool ln_geom(int M, int C, bool layernorm, LnGeom* g, dim3* grid,
                    int* slices) {
    int p[5];
    const int served = ln_plan(M, C, p);
    if (served < (layernorm ? 2 : 1)) return false;
    g->M = M; g->C = C; g->G = p[0]; g->rpb = p[1];
    *grid = dim3(p[2], layernorm ? 1 : p[3]);
    *slices = p[4];
    return true;
}

// Everything up to the matching pop is compiled without packed fp32 math (see
// fused_optim.hip for why); a function under this attribute can only inline
// always_inline callees, hence ln_barrier and the builtins below.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// sum over the G lanes of this lane's group; every lane gets the same bits
__device__ __forceinline__ float ln_group_sum(float v, int lane, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) {
        const int o = __builtin_amdgcn_ds_bpermute((lane ^ off) << 2,
                                                   __builtin_bit_cast(int, v));
        v += __builtin_bit_cast(float, o);
    }
    return v;
}

// s + e == a + b exactly (Knuth's TwoSum; no multiply, so nothing contracts)
__device__ __forceinline__ void ln_two_sum(float a, float b, float* s,
                                           float* e) {
    const float t = a + b;
    const float bb = t - a;
    *e = (a - (t - bb)) + (b - bb);
    *s = t;
}

// ln_group_sum of the pairs hi + lo, the butterfly's own roundings kept in
// lo; TwoSum is symmetric, so every lane still ends with the same bits
__device__ __forceinline__ float ln_group_sum2(float hi, float lo, int lane,
                                               int G) {
    for (int off = G >> 1; off > 0; off >>= 1) {
        const int a = (lane ^ off) << 2;
        const float oh = __builtin_bit_cast(
            float, __builtin_amdgcn_ds_bpermute(a, __builtin_bit_cast(int, hi)));
        const float ol = __builtin_bit_cast(
            float, __builtin_amdgcn_ds_bpermute(a, __builtin_bit_cast(int, lo)));
        float r;
        ln_two_sum(hi, oh, &hi, &r);
        lo = (lo + ol) + r;
    }
    return hi + lo;
}

// The walk of one thread: its group lane, its row slot and its octets.
template <int NO>
struct LnWalk {
    int lane, lig, rslot, RB, col0;
    int ch[NO];
    bool on[NO];
    int row, rend;
    __device__ __forceinline__ LnWalk(const LnGeom& g) {
        const int tid = threadIdx.x;
        lane = tid & (WAVE_SIZE - 1);
        lig = tid & (g.G - 1);
        rslot = tid / g.G;
        RB = LN_THREADS / g.G;
        col0 = blockIdx.y * LN_CHUNK;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            ch[o] = col0 + (lig + o * LN_MAXG) * 8;
            on[o] = ch[o] < g.C;
        }
        row = blockIdx.x * g.rpb + rslot;
        const int64_t e = (int64_t)(blockIdx.x + 1) * g.rpb;
        rend = e < g.M ? (int)e : g.M;
    }
};

// Fold one column sum of the block: acc[o][c] of every thread -> red
// [RB][NO * G * 8] -> the sum over the row slots, in slot order, into
// dst[C] (one [C] row of the block's workspace slice).
template <int NO>
__device__ __forceinline__ void ln_fold(float* red, const float (*acc)[8],
                                        float* __restrict__ dst,
                                        const LnWalk<NO>& w, const LnGeom& g) {
    const int ncols = NO * g.G * 8;
    ln_barrier();       // the previous fold's reads are done
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int c = 0; c < 8; ++c)
            red[w.rslot * ncols + (o * g.G + w.lig) * 8 + c] = acc[o][c];
    ln_barrier();
    for (int idx = threadIdx.x; idx < ncols; idx += LN_THREADS) {
        float s = red[idx];
        for (int r = 1; r < w.RB; ++r) s += red[r * ncols + idx];
        if (w.col0 + idx < g.C) dst[w.col0 + idx] = s;
    }
}

// y = (x + b_in - mean) * rstd * gamma + beta; stats[row] = (mean, rstd)
template <int NO>
__global__ void __launch_bounds__(LN_THREADS)
k_ln_fwd(const uint16_t* __restrict__ x, const float* __restrict__ b_in,
         const float* __restrict__ gamma, const float* __restrict__ beta,
         uint16_t* __restrict__ y, float* __restrict__ stats, LnGeom g,
         float eps) {
    LnWalk<NO> w(g);
    float bi[NO][8], ga[NO][8], be[NO][8];
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        ln_param8(b_in, w.ch[o], w.on[o], 0.f, bi[o]);
        ln_param8(gamma, w.ch[o], w.on[o], 0.f, ga[o]);
        ln_param8(beta, w.ch[o], w.on[o], 0.f, be[o]);
    }
    const float inv_c = 1.f / (float)g.C;
    for (int row = w.row; row < w.rend; row += w.RB) {
        const int64_t base = (int64_t)row * g.C;
        float f[NO][8];
        float s = 0.f;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (w.on[o]) {
                ln_load8(x, base + w.ch[o], f[o]);
#pragma unroll
                for (int c = 0; c < 8; ++c) { f[o][c] += bi[o][c]; s += f[o][c]; }
            }
        }
        const float mean = ln_group_sum(s, w.lane, g.G) * inv_c;
        float ss = 0.f;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (w.on[o]) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    f[o][c] -= mean;
                    ss = __builtin_fmaf(f[o][c], f[o][c], ss);
                }
            }
        }
        const float var = ln_group_sum(ss, w.lane, g.G) * inv_c;
        const float rstd = 1.f / __builtin_sqrtf(var + eps);
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (w.on[o]) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    f[o][c] = __builtin_fmaf(f[o][c] * rstd, ga[o][c], be[o][c]);
                ln_store8(y, base + w.ch[o], f[o]);
            }
        }
        if (w.lig == 0) {
            stats[2 * (int64_t)row] = mean;
            stats[2 * (int64_t)row + 1] = rstd;
        }
    }
}

// dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)), g = dy * gamma (not
// stored where dx is null); slice sums: dy * xhat, dy and, with b_in, dx.
template <int NO>
__global__ void __launch_bounds__(LN_THREADS)
k_ln_bwd(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
         const float* __restrict__ b_in, const float* __restrict__ stats,
         const float* __restrict__ gamma, uint16_t* __restrict__ dx,
         float* __restrict__ ws, LnGeom g) {
    __shared__ float red[LN_THREADS * 8 * NO];
    LnWalk<NO> w(g);
    float bi[NO][8], ga[NO][8];
    float a_g[NO][8], a_b[NO][8], a_x[NO][8];
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        ln_param8(b_in, w.ch[o], w.on[o], 0.f, bi[o]);
        ln_param8(gamma, w.ch[o], w.on[o], 0.f, ga[o]);
#pragma unroll
        for (int c = 0; c < 8; ++c) a_g[o][c] = a_b[o][c] = a_x[o][c] = 0.f;
    }
    const float inv_c = 1.f / (float)g.C;
    for (int row = w.row; row < w.rend; row += w.RB) {
        const int64_t base = (int64_t)row * g.C;
        const float mean = stats[2 * (int64_t)row];
        const float rstd = stats[2 * (int64_t)row + 1];
        float xh[NO][8], lo[NO][8], gg[NO][8];
        // x + b - mean as an exact pair xh + lo, and the pair sum of the row:
        // what the saved fp32 mean is off the row's own mean by
        float sh = 0.f, sl = 0.f;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (w.on[o]) {
                ln_load8(x, base + w.ch[o], xh[o]);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    float e, r;
                    ln_two_sum(xh[o][c], bi[o][c], &xh[o][c], &e);
                    ln_two_sum(xh[o][c], -mean, &xh[o][c], &lo[o][c]);
                    lo[o][c] += e;
                    ln_two_sum(sh, xh[o][c], &sh, &r);
                    sl += r + lo[o][c];
                }
            }
        }
        const float off = ln_group_sum2(sh, sl, w.lane, g.G) * inv_c;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (w.on[o]) {
                float d[8];
                ln_load8(dy, base + w.ch[o], d);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    xh[o][c] = ((xh[o][c] - off) + lo[o][c]) * rstd;
                    gg[o][c] = d[c] * ga[o][c];
                    s1 += gg[o][c];
                    s2 = __builtin_fmaf(gg[o][c], xh[o][c], s2);
                    a_g[o][c] = __builtin_fmaf(d[c], xh[o][c], a_g[o][c]);
                    a_b[o][c] += d[c];
                }
            }
        }
        const float m1 = ln_group_sum(s1, w.lane, g.G) * inv_c;
        const float m2 = ln_group_sum(s2, w.lane, g.G) * inv_c;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            if (w.on[o]) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    gg[o][c] = rstd * (gg[o][c] - m1 - xh[o][c] * m2);
                    a_x[o][c] += gg[o][c];
                }
                if (dx) ln_store8(dx, base + w.ch[o], gg[o]);
            }
        }
    }
    const int k = b_in ? 3 : 2;
    float* const slice = ws + (int64_t)blockIdx.x * k * g.C;
    ln_fold<NO>(red, a_g, slice, w, g);
    ln_fold<NO>(red, a_b, slice + g.C, w, g);
    if (b_in) ln_fold<NO>(red, a_x, slice + 2 * g.C, w, g);
}

// g = gelu(h + b)
__global__ void __launch_bounds__(LN_THREADS)
k_bias_gelu_fwd(const uint16_t* __restrict__ h, const float* __restrict__ b,
                uint16_t* __restrict__ out, LnGeom g) {
    LnWalk<1> w(g);
    float bi[8];
    ln_param8(b, w.ch[0], w.on[0], 0.f, bi);
    if (!w.on[0]) return;
    for (int row = w.row; row < w.rend; row += w.RB) {
        const int64_t at = (int64_t)row * g.C + w.ch[0];
        float f[8];
        ln_load8(h, at, f);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float u = f[c] + bi[c];
            float Phi, phi;
            ln_gauss(u, &Phi, &phi);
            f[c] = u * Phi;
        }
        ln_store8(out, at, f);
    }
}

// dh = dg * (Phi(u) + u * phi(u)), u = h + b recomputed; slice sum: dh
__global__ void __launch_bounds__(LN_THREADS)
k_bias_gelu_bwd(const uint16_t* __restrict__ dg, const uint16_t* __restrict__ h,
                const float* __restrict__ b, uint16_t* __restrict__ dh,
                float* __restrict__ ws, LnGeom g) {
    __shared__ float red[LN_THREADS * 8];
    LnWalk<1> w(g);
    float bi[8], a_b[1][8];
    ln_param8(b, w.ch[0], w.on[0], 0.f, bi);
#pragma unroll
    for (int c = 0; c < 8; ++c) a_b[0][c] = 0.f;
    if (w.on[0]) {
        for (int row = w.row; row < w.rend; row += w.RB) {
            const int64_t at = (int64_t)row * g.C + w.ch[0];
            float f[8], d[8];
            ln_load8(h, at, f);
            ln_load8(dg, at, d);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float u = f[c] + bi[c];
                float Phi, phi;
                ln_gauss(u, &Phi, &phi);
                d[c] *= __builtin_fmaf(u, phi, Phi);
                a_b[0][c] += d[c];
            }
            ln_store8(dh, at, d);
        }
    }
    ln_fold<1>(red, a_b, ws + (int64_t)blockIdx.x * g.C, w, g);
}

// out = res + s * (z + b)
__global__ void __launch_bounds__(LN_THREADS)
k_scale_residual_fwd(const uint16_t* __restrict__ z,
                     const float* __restrict__ b, const float* __restrict__ s,
                     const uint16_t* __restrict__ res,
                     uint16_t* __restrict__ out, LnGeom g) {
    LnWalk<1> w(g);
    float bi[8], sc[8];
    ln_param8(b, w.ch[0], w.on[0], 0.f, bi);
    ln_param8(s, w.ch[0], w.on[0], 0.f, sc);
    if (!w.on[0]) return;
    for (int row = w.row; row < w.rend; row += w.RB) {
        const int64_t at = (int64_t)row * g.C + w.ch[0];
        float f[8], r[8];
        ln_load8(z, at, f);
        ln_load8(res, at, r);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            f[c] = __builtin_fmaf(sc[c], f[c] + bi[c], r[c]);
        ln_store8(out, at, f);
    }
}

// dz = s * dout; slice sums: dout * (z + b) and s * dout
__global__ void __launch_bounds__(LN_THREADS)
k_scale_residual_bwd(const uint16_t* __restrict__ dout,
                     const uint16_t* __restrict__ z,
                     const float* __restrict__ b, const float* __restrict__ s,
                     uint16_t* __restrict__ dz, float* __restrict__ ws,
                     LnGeom g) {
    __shared__ float red[LN_THREADS * 8];
    LnWalk<1> w(g);
    float bi[8], sc[8], a_s[1][8], a_b[1][8];
    ln_param8(b, w.ch[0], w.on[0], 0.f, bi);
    ln_param8(s, w.ch[0], w.on[0], 0.f, sc);
#pragma unroll
    for (int c = 0; c < 8; ++c) a_s[0][c] = a_b[0][c] = 0.f;
    if (w.on[0]) {
        for (int row = w.row; row < w.rend; row += w.RB) {
            const int64_t at = (int64_t)row * g.C + w.ch[0];
            float f[8], d[8];
            ln_load8(z, at, f);
            ln_load8(dout, at, d);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                a_s[0][c] = __builtin_fmaf(d[c], f[c] + bi[c], a_s[0][c]);
                d[c] *= sc[c];
                a_b[0][c] += d[c];
            }
            ln_store8(dz, at, d);
        }
    }
    float* const slice = ws + (int64_t)blockIdx.x * 2 * g.C;
    ln_fold<1>(red, a_s, slice, w, g);
    ln_fold<1>(red, a_b, slice + g.C, w, g);
}

// z = bf16(z + b), in place
__global__ void __launch_bounds__(LN_THREADS)
k_bias_add(uint16_t* z, const float* __restrict__ b, LnGeom g) {
    LnWalk<1> w(g);
    float bi[8];
    ln_param8(b, w.ch[0], w.on[0], 0.f, bi);
    if (!w.on[0]) return;
    for (int row = w.row; row < w.rend; row += w.RB) {
        const int64_t at = (int64_t)row * g.C + w.ch[0];
        float f[8];
        ln_load8(z, at, f);
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] += bi[c];
        ln_store8(z, at, f);
    }
}

// slice sum: dout (the gradient of a per-channel bias; dz is dout itself)
__global__ void __launch_bounds__(LN_THREADS)
k_bias_add_bwd(const uint16_t* __restrict__ dout, float* __restrict__ ws,
               LnGeom g) {
    __shared__ float red[LN_THREADS * 8];
    LnWalk<1> w(g);
    float a_b[1][8];
#pragma unroll
    for (int c = 0; c < 8; ++c) a_b[0][c] = 0.f;
    if (w.on[0]) {
        for (int row = w.row; row < w.rend; row += w.RB) {
            float d[8];
            ln_load8(dout, (int64_t)row * g.C + w.ch[0], d);
#pragma unroll
            for (int c = 0; c < 8; ++c) a_b[0][c] += d[c];
        }
    }
    ln_fold<1>(red, a_b, ws + (int64_t)blockIdx.x * g.C, w, g);
}

// ws: fp32 [slices][k][C].  d_j[c] += sum over the slices of ws[.][j][c] for
// every non-null d_j: 8 contiguous runs of slices, each in slice order, then
// the run totals in run order.  A block serves LN_RCOLS of the k * C columns.
__global__ void __launch_bounds__(LN_THREADS)
k_colsum_combine(const float* __restrict__ ws, float* __restrict__ d0,
                 float* __restrict__ d1, float* __restrict__ d2, int k, int C,
                 int slices) {
    __shared__ float red[LN_RUNS][LN_RCOLS];
    const int col = threadIdx.x % LN_RCOLS, run = threadIdx.x / LN_RCOLS;
    const int kc = k * C;
    const int i = blockIdx.x * LN_RCOLS + col;
    const int per = (slices + LN_RUNS - 1) / LN_RUNS;
    const int z0 = run * per;
    const int z1 = z0 + per < slices ? z0 + per : slices;
    float s = 0.f;
    if (i < kc)
        for (int z = z0; z < z1; ++z) s += ws[(int64_t)z * kc + i];
    red[run][col] = s;
    ln_barrier();
    if (run == 0 && i < kc) {
        float t = red[0][col];
#pragma unroll
        for (int r = 1; r < LN_RUNS; ++r) t += red[r][col];
        const int j = i / C;
        float* const d = j == 0 ? d0 : j == 1 ? d1 : d2;
        if (d) d[i - j * C] += t;
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
void ln_combine(const void* ws, void* d0, void* d1, void* d2, int k, int C,
                int slices, hipStream_t stream) {
    const int blocks = (k * C + LN_RCOLS - 1) / LN_RCOLS;
    k_colsum_combine<<<blocks, LN_THREADS, 0, stream>>>(
        (const float*)ws, (float*)d0, (float*)d1, (float*)d2, k, C, slices);
}

// Activations: contiguous bf16 [M][C], 16-byte aligned.  Parameters and
// gradient targets: fp32 [C].  Workspaces: fp32 [slices][k][C] with slices
// from ln_plan.  Each launcher returns 0 (nothing launched) where ln_plan
// declines the shape.

// b_in may be null; stats: fp32 [M][2]
extern "C" int launch_ln_fwd(const void* x, const void* b_in,
                             const void* gamma, const void* beta, void* y,
                             void* stats, int M, int C, float eps,
                             hipStream_t stream) {
    LnGeom g; dim3 grid; int slices;
    if (!ln_geom(M, C, true, &g, &grid, &slices)) return 0;
    if (C <= LN_CHUNK)
        k_ln_fwd<1><<<grid, LN_THREADS, 0, stream>>>(
            (const uint16_t*)x, (const float*)b_in, (const float*)gamma,
            (const float*)beta, (uint16_t*)y, (float*)stats, g, eps);
    else
        k_ln_fwd<2><<<grid, LN_THREADS, 0, stream>>>(
            (const uint16_t*)x, (const float*)b_in, (const float*)gamma,
            (const float*)beta, (uint16_t*)y, (float*)stats, g, eps);
    return 1;
}

// b_in, dx and each of dgamma / dbeta / db_in may be null; k = 3 with b_in,
// else 2.  The gradient targets are accumulated into.
extern "C" int launch_ln_bwd(const void* dy, const void* x, const void* b_in,
                             const void* stats, const void* gamma, void* dx,
                             void* ws, void* dgamma, void* dbeta, void* db_in,
                             int M, int C, hipStream_t stream) {
    LnGeom g; dim3 grid; int slices;
    if (!ln_geom(M, C, true, &g, &grid, &slices)) return 0;
    if (C <= LN_CHUNK)
        k_ln_bwd<1><<<grid, LN_THREADS, 0, stream>>>(
            (const uint16_t*)dy, (const uint16_t*)x, (const float*)b_in,
            (const float*)stats, (const float*)gamma, (uint16_t*)dx,
            (float*)ws, g);
    else
        k_ln_bwd<2><<<grid, LN_THREADS, 0, stream>>>(
            (const uint16_t*)dy, (const uint16_t*)x, (const float*)b_in,
            (const float*)stats, (const float*)gamma, (uint16_t*)dx,
            (float*)ws, g);
    ln_combine(ws, dgamma, dbeta, b_in ? db_in : nullptr, b_in ? 3 : 2, C,
               slices, stream);
    return 1;
}

extern "C" int launch_bias_gelu_fwd(const void* h, const void* b, void* out,
                                    int M, int C, hipStream_t stream) {
    LnGeom g; dim3 grid; int slices;
    if (!ln_geom(M, C, false, &g, &grid, &slices)) return 0;
    k_bias_gelu_fwd<<<grid, LN_THREADS, 0, stream>>>(
        (const uint16_t*)h, (const float*)b, (uint16_t*)out, g);
    return 1;
}

// k = 1; db may be null
extern "C" int launch_bias_gelu_bwd(const void* dg, const void* h,
                                    const void* b, void* dh, void* ws,
                                    void* db, int M, int C,
                                    hipStream_t stream) {
    LnGeom g; dim3 grid; int slices;
    if (!ln_geom(M, C, false, &g, &grid, &slices)) return 0;
    k_bias_gelu_bwd<<<grid, LN_THREADS, 0, stream>>>(
        (const uint16_t*)dg, (const uint16_t*)h, (const float*)b,
        (uint16_t*)dh, (float*)ws, g);
    ln_combine(ws, db, nullptr, nullptr, 1, C, slices, stream);
    return 1;
}

extern "C" int launch_scale_residual_fwd(const void* z, const void* b,
                                         const void* s, const void* res,
                                         void* out, int M, int C,
                                         hipStream_t stream) {
    LnGeom g; dim3 grid; int slices;
    if (!ln_geom(M, C, false, &g, &grid, &slices)) return 0;
    k_scale_residual_fwd<<<grid, LN_THREADS, 0, stream>>>(
        (const uint16_t*)z, (const float*)b, (const float*)s,
        (const uint16_t*)res, (uint16_t*)out, g);
    return 1;
}

extern "C" int launch_bias_add(void* z, const void* b, int M, int C,
                               hipStream_t stream) {
    LnGeom g; dim3 grid; int slices;
    if (!ln_geom(M, C, false, &g, &grid, &slices)) return 0;
    k_bias_add<<<grid, LN_THREADS, 0, stream>>>((uint16_t*)z, (const float*)b,
                                                g);
    return 1;
}

// k = 1; db += the column sums of dout
extern "C" int launch_bias_add_bwd(const void* dout, void* ws, void* db, int M,
                                   int C, hipStream_t stream) {
    LnGeom g; dim3 grid; int slices;
    if (!ln_geom(M, C, false, &g, &grid, &slices)) return 0;
    k_bias_add_bwd<<<grid, LN_THREADS, 0, stream>>>((const uint16_t*)dout,
                                                    (float*)ws, g);
    ln_combine(ws, db, nullptr, nullptr, 1, C, slices, stream);
    return 1;
}

// k = 2; ds and db may be null
extern "C" int launch_scale_residual_bwd(const void* dout, const void* z,
                                         const void* b, const void* s,
                                         void* dz, void* ws, void* ds,
                                         void* db, int M, int C,
                                         hipStream_t stream) {
    LnGeom g; dim3 grid; int slices;
    if (!ln_geom(M, C, false, &g, &grid, &slices)) return 0;
    k_scale_residual_bwd<<<grid, LN_THREADS, 0, stream>>>(
        (const uint16_t*)dout, (const uint16_t*)z, (const float*)b,
        (const float*)s, (uint16_t*)dz, (float*)ws, g);
    ln_combine(ws, ds, db, nullptr, 2, C, slices, stream);
    return 1;
}

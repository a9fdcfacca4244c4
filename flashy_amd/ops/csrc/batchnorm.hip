// Copyright (c) Flashy-AMD authors.
// NHWC BatchNorm (training) for gfx950, operating on [M, C] with
// M = N*H*W, bf16 activations, fp32 stats/params.
//
// forward:  stats (per-channel sum/sumsq partials; short8 loads, one
//                  partial slot per block — no atomics, no pre-zeroing)
//        -> finalize (combine partials, mean/invstd/scale/shift, running)
//        -> apply (y = relu(scale*x + shift [+ res]), float4 param loads)
// backward: reduce (dz = dy * relu-mask; partial sums; dz written out —
//                   it IS the residual gradient)
//        -> grads (combine -> bsums; dgamma/dbeta += into flat fp32 grads)
//        -> apply (dx = scale*(dz - (sum_dz + xhat*sum_dzxhat)/M))
//
// partials layout [2][C][msplit] so the combine kernels read each channel's
// msplit partials CONTIGUOUSLY.
//
// Replaces the BatchNorm + ReLU + residual-add chains of the reference's
// ResNet workload with NHWC-native fused kernels.

#include "common.h"

// ---------------------------------------------------------------------------
// fwd 1: stats.  Block = 256 threads = 8 channel-octets x 32 m-lanes over a
// 64-channel group; short8 loads (16 B/lane).  Grid (C/64, msplit).
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
k_bn_stats(const uint16_t* __restrict__ x, float* __restrict__ partials,
           int64_t M, int C, int msplit, int m_per_block) {
    const int c8 = (threadIdx.x & 7) * 8;           // channel octet in group
    const int mlane = threadIdx.x >> 3;             // 0..31
    const int cbase = blockIdx.x * 64;
    const int64_t m0 = (int64_t)blockIdx.y * m_per_block;
    const int64_t m1 = min(m0 + (int64_t)m_per_block, M);
    float s[8] = {}, s2[8] = {};
    for (int64_t m = m0 + mlane; m < m1; m += 32) {
        const short8 v8 = *reinterpret_cast<const short8*>(
            x + m * C + cbase + c8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = bf16_to_f32(((const uint16_t*)&v8)[j]);
            s[j] += v;
            s2[j] = fmaf(v, v, s2[j]);
        }
    }
    // fold 32 m-lanes: LDS [2][32][64]
    __shared__ float red[2][32][64];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[0][mlane][c8 + j] = s[j];
        red[1][mlane][c8 + j] = s2[j];
    }
    __syncthreads();
    // 256 threads: tid<64 handles sum, tid in [64,128) handles sumsq
    const int c = threadIdx.x & 63;
    const int which = threadIdx.x >> 6;
    if (which < 2) {
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < 32; ++i) acc += red[which][i][c];
        partials[((int64_t)which * C + cbase + c) * msplit + blockIdx.y] = acc;
    }
}

// ---------------------------------------------------------------------------
// combine helper: [2][C][msplit] -> (s, s2) per channel.  Block = 256
// threads = 64 channels x 4 split-lanes; contiguous per-channel reads.
// ---------------------------------------------------------------------------

// Block = 8 channels x 32 split-lanes (grid C/8): at C=64 that is 8 blocks
// instead of 1, and each thread issues only ~msplit/16 float4 loads, so the
// single-digit-block latency wall of a C/64 mapping disappears.  Threads
// tid<8 leave with the channel's (s, s2); they are also the writers.
__device__ __forceinline__ void combine_partials8(
        const float* __restrict__ partials, int msplit, int C,
        float* s_out, float* s2_out) {
    const int ch = threadIdx.x & 7;               // channel within block
    const int slane = threadIdx.x >> 3;           // 0..31
    const int c = blockIdx.x * 8 + ch;
    const float* row0 = partials + (int64_t)c * msplit;
    const float* row1 = partials + ((int64_t)C + c) * msplit;
    float s = 0.f, s2 = 0.f;
    if (msplit & 3) {
        // row base c*msplit is 16B-aligned only when msplit % 4 == 0 (the
        // fused conv-epilogue path passes msplit = conv grid.x, which is
        // not forced to a multiple of 4) -> scalar loads for odd msplit.
        for (int i = slane; i < msplit; i += 32) {
            s += row0[i];
            s2 += row1[i];
        }
    } else {
        for (int i = slane * 4; i + 4 <= msplit; i += 128) {
            const float4 a = *reinterpret_cast<const float4*>(row0 + i);
            const float4 b = *reinterpret_cast<const float4*>(row1 + i);
            s += a.x + a.y + a.z + a.w;
            s2 += b.x + b.y + b.z + b.w;
        }
    }
    __shared__ float red[2][32][8];
    red[0][slane][ch] = s;
    red[1][slane][ch] = s2;
    __syncthreads();
    if (threadIdx.x < 16) {
        const int w = threadIdx.x >> 3;
        const int cc = threadIdx.x & 7;
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < 32; ++i) acc += red[w][i][cc];
        red[w][0][cc] = acc;
    }
    __syncthreads();
    *s_out = red[0][0][ch];
    *s2_out = red[1][0][ch];
}

// work[0..C) = mean, [C..2C) = invstd, [2C..3C) = scale, [3C..4C) = shift
// One channel's finalize, run by the 8 writer threads of a combine block;
// shared by k_bn_finalize and k_bn_fwd_small, which must agree bit for bit.
__device__ __forceinline__ void bn_finalize_channel(
        float s, float s2, int c,
        const float* __restrict__ gamma, const float* __restrict__ beta,
        float* __restrict__ running_mean, float* __restrict__ running_var,
        float* __restrict__ work, int64_t M, int C,
        float eps, float momentum, int update_running,
        float* scale_out, float* shift_out) {
    const float mean = s / (float)M;
    float var = s2 / (float)M - mean * mean;
    var = fmaxf(var, 0.f);
    const float invstd = rsqrtf(var + eps);
    const float scale = gamma[c] * invstd;
    const float shift = beta[c] - mean * scale;
    work[c] = mean;
    work[C + c] = invstd;
    work[2 * C + c] = scale;
    work[3 * C + c] = shift;
    if (update_running) {
        running_mean[c] += momentum * (mean - running_mean[c]);
        const float unbiased = M > 1 ? var * (float)M / (float)(M - 1) : var;
        running_var[c] += momentum * (unbiased - running_var[c]);
    }
    *scale_out = scale;
    *shift_out = shift;
}

__global__ void __launch_bounds__(256)
k_bn_finalize(const float* __restrict__ partials, int msplit,
              const float* __restrict__ gamma,
              const float* __restrict__ beta,
              float* __restrict__ running_mean,
              float* __restrict__ running_var,
              float* __restrict__ work, int64_t M, int C,
              float eps, float momentum, int update_running) {
    float s, s2;
    combine_partials8(partials, msplit, C, &s, &s2);
    if (threadIdx.x >= 8) return;
    float scale, shift;
    bn_finalize_channel(s, s2, blockIdx.x * 8 + threadIdx.x, gamma, beta,
                        running_mean, running_var, work, M, C, eps, momentum,
                        update_running, &scale, &shift);
}

// ---------------------------------------------------------------------------
// fwd 3: y = [relu](scale*x + shift [+ res]).  short8 data, float4 params.
// ---------------------------------------------------------------------------

template <bool RELU, bool RES>
__global__ void __launch_bounds__(256)
k_bn_apply(const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
           uint16_t* __restrict__ y, const float* __restrict__ work,
           int64_t M, int C, float slope) {
    const int64_t total8 = M * C / 8;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float4* scale4 = reinterpret_cast<const float4*>(work + 2 * (int64_t)C);
    const float4* shift4 = reinterpret_cast<const float4*>(work + 3 * (int64_t)C);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total8;
         i += stride) {
        const int co = (int)((i * 8) % C) / 4;
        const float4 sc[2] = {scale4[co], scale4[co + 1]};
        const float4 sh[2] = {shift4[co], shift4[co + 1]};
        short8 xv = *reinterpret_cast<const short8*>(x + i * 8);
        short8 rv = {};
        if (RES) rv = *reinterpret_cast<const short8*>(res + i * 8);
        short8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = fmaf(bf16_to_f32(((const uint16_t*)&xv)[j]),
                           ((const float*)sc)[j], ((const float*)sh)[j]);
            if (RES) v += bf16_to_f32(((const uint16_t*)&rv)[j]);
            if (RELU) v = v > 0.f ? v : slope * v;  // slope 0 = plain ReLU
            ((uint16_t*)&out)[j] = f32_to_bf16(v);
        }
        *reinterpret_cast<short8*>(y + i * 8) = out;
    }
}

// One output element of the forward apply / of the backward dx; shared by the
// channel-resident kernels below and the single-kernel small-M forms.
template <bool RELU, bool RES>
__device__ __forceinline__ uint16_t bn_apply_elem(uint16_t x, uint16_t r,
                                                  float sc, float sh,
                                                  float slope) {
    float v = fmaf(bf16_to_f32(x), sc, sh);
    if (RES) v += bf16_to_f32(r);
    if (RELU) v = v > 0.f ? v : slope * v;
    return f32_to_bf16(v);
}

// b0 = sum(dz)/M, b1 = sum(dz*xhat)/M
__device__ __forceinline__ uint16_t bn_bwd_dx_elem(uint16_t dz, uint16_t x,
                                                   float mn, float is, float sc,
                                                   float b0, float b1) {
    const float xhat = (bf16_to_f32(x) - mn) * is;
    const float g = bf16_to_f32(dz);
    return f32_to_bf16(sc * (g - b0 - xhat * b1));
}

// Channel-resident variant for C % 64 == 0 (every trunk BN): thread owns a
// fixed 8-channel group, coefficients load ONCE into registers, the loop is
// pure 16B streaming over m — no per-iteration int64 div/mod (the generic
// kernel's `(i*8) % C` is an emulated 64-bit divide and caps it ~3 TB/s).
template <bool RELU, bool RES>
__global__ void __launch_bounds__(256)
k_bn_apply_c64(const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
               uint16_t* __restrict__ y, const float* __restrict__ work,
               int64_t M, int C, float slope, int m_per_block) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 7) * 8;
    const int mlane = threadIdx.x >> 3;
    const int64_t m0 = (int64_t)blockIdx.y * m_per_block;
    const int64_t m1 = min(m0 + (int64_t)m_per_block, M);
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = work[2 * (int64_t)C + c + j];
        sh[j] = work[3 * (int64_t)C + c + j];
    }
    for (int64_t m = m0 + mlane; m < m1; m += 32) {
        const int64_t off = m * C + c;
        short8 xv = *reinterpret_cast<const short8*>(x + off);
        short8 rv = {};
        if (RES) rv = *reinterpret_cast<const short8*>(res + off);
        short8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            ((uint16_t*)&out)[j] = bn_apply_elem<RELU, RES>(
                ((const uint16_t*)&xv)[j], ((const uint16_t*)&rv)[j],
                sc[j], sh[j], slope);
        *reinterpret_cast<short8*>(y + off) = out;
    }
}

__global__ void __launch_bounds__(256)
k_bn_bwd_apply_c64(const uint16_t* __restrict__ dz,
                   const uint16_t* __restrict__ x,
                   const float* __restrict__ work,
                   const float* __restrict__ bsums,
                   uint16_t* __restrict__ dx, int64_t M, int C,
                   int m_per_block) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 7) * 8;
    const int mlane = threadIdx.x >> 3;
    const int64_t m0 = (int64_t)blockIdx.y * m_per_block;
    const int64_t m1 = min(m0 + (int64_t)m_per_block, M);
    const float invM = 1.f / (float)M;
    float mn[8], is[8], sc[8], b0[8], b1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mn[j] = work[c + j];
        is[j] = work[C + c + j];
        sc[j] = work[2 * (int64_t)C + c + j];
        b0[j] = bsums[c + j] * invM;
        b1[j] = bsums[C + c + j] * invM;
    }
    for (int64_t m = m0 + mlane; m < m1; m += 32) {
        const int64_t off = m * C + c;
        short8 gz = *reinterpret_cast<const short8*>(dz + off);
        short8 xv = *reinterpret_cast<const short8*>(x + off);
        short8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            ((uint16_t*)&out)[j] = bn_bwd_dx_elem(
                ((const uint16_t*)&gz)[j], ((const uint16_t*)&xv)[j],
                mn[j], is[j], sc[j], b0[j], b1[j]);
        *reinterpret_cast<short8*>(dx + off) = out;
    }
}

// m-blocks for the c64 apply kernels: ~1024 blocks saturate the chip
static inline int apply_mpb(int64_t M, int C) {
    const int cblocks = C / 64;
    int target = 1024 / cblocks;
    if (target < 1) target = 1;
    int64_t mblocks = (M + 31) / 32;
    if (mblocks > target) mblocks = target;
    return (int)((M + mblocks - 1) / mblocks);
}

// ---------------------------------------------------------------------------
// bwd 1: dz = dy * (y > 0) [if relu]; per-channel partial sums of dz and
// dz*xhat.  Same geometry as stats.
// ---------------------------------------------------------------------------

template <bool RELU>
__global__ void __launch_bounds__(256)
k_bn_bwd_reduce(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                const uint16_t* __restrict__ x, const float* __restrict__ work,
                uint16_t* __restrict__ dz_out, float* __restrict__ partials,
                int64_t M, int C, int msplit, int m_per_block, float slope) {
    const int c8 = (threadIdx.x & 7) * 8;
    const int mlane = threadIdx.x >> 3;
    const int cbase = blockIdx.x * 64;
    const int64_t m0 = (int64_t)blockIdx.y * m_per_block;
    const int64_t m1 = min(m0 + (int64_t)m_per_block, M);
    float mean[8], invstd[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mean[j] = work[cbase + c8 + j];
        invstd[j] = work[C + cbase + c8 + j];
    }
    float s[8] = {}, sx[8] = {};
    for (int64_t m = m0 + mlane; m < m1; m += 32) {
        const int64_t off = m * C + cbase + c8;
        const short8 g8 = *reinterpret_cast<const short8*>(dy + off);
        const short8 x8 = *reinterpret_cast<const short8*>(x + off);
        short8 y8 = {};
        if (RELU) y8 = *reinterpret_cast<const short8*>(y + off);
        short8 dz8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float g = bf16_to_f32(((const uint16_t*)&g8)[j]);
            if (RELU && bf16_to_f32(((const uint16_t*)&y8)[j]) <= 0.f)
                g *= slope;
            ((uint16_t*)&dz8)[j] = f32_to_bf16(g);
            s[j] += g;
            const float xh = (bf16_to_f32(((const uint16_t*)&x8)[j]) - mean[j]) * invstd[j];
            sx[j] = fmaf(g, xh, sx[j]);
        }
        *reinterpret_cast<short8*>(dz_out + off) = dz8;
    }
    __shared__ float red[2][32][64];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[0][mlane][c8 + j] = s[j];
        red[1][mlane][c8 + j] = sx[j];
    }
    __syncthreads();
    const int c = threadIdx.x & 63;
    const int which = threadIdx.x >> 6;
    if (which < 2) {
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < 32; ++i) acc += red[which][i][c];
        partials[((int64_t)which * C + cbase + c) * msplit + blockIdx.y] = acc;
    }
}

// combine partials -> bsums[2C]; dgamma/dbeta += (flat fp32 grads)
__global__ void __launch_bounds__(256)
k_bn_bwd_grads(const float* __restrict__ partials, int msplit,
               float* __restrict__ bsums,
               float* __restrict__ dgamma,
               float* __restrict__ dbeta, int C) {
    float s, sx;
    combine_partials8(partials, msplit, C, &s, &sx);
    if (threadIdx.x >= 8) return;
    const int c = blockIdx.x * 8 + threadIdx.x;
    bsums[c] = s;
    bsums[C + c] = sx;
    dbeta[c] += s;
    dgamma[c] += sx;
}

// ---------------------------------------------------------------------------
// bwd 3: dx = scale * (dz - (sum_dz + xhat * sum_dz_xhat) / M)
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
k_bn_bwd_apply(const uint16_t* __restrict__ dz, const uint16_t* __restrict__ x,
               const float* __restrict__ work, const float* __restrict__ bsums,
               uint16_t* __restrict__ dx, int64_t M, int C) {
    const int64_t total8 = M * C / 8;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float invM = 1.f / (float)M;
    const float4* mean4 = reinterpret_cast<const float4*>(work);
    const float4* invstd4 = reinterpret_cast<const float4*>(work + C);
    const float4* scale4 = reinterpret_cast<const float4*>(work + 2 * (int64_t)C);
    const float4* b04 = reinterpret_cast<const float4*>(bsums);
    const float4* b14 = reinterpret_cast<const float4*>(bsums + C);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total8;
         i += stride) {
        const int co = (int)((i * 8) % C) / 4;
        const float4 mn[2] = {mean4[co], mean4[co + 1]};
        const float4 is[2] = {invstd4[co], invstd4[co + 1]};
        const float4 sc[2] = {scale4[co], scale4[co + 1]};
        const float4 b0[2] = {b04[co], b04[co + 1]};
        const float4 b1[2] = {b14[co], b14[co + 1]};
        short8 gz = *reinterpret_cast<const short8*>(dz + i * 8);
        short8 xv = *reinterpret_cast<const short8*>(x + i * 8);
        short8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xhat = (bf16_to_f32(((const uint16_t*)&xv)[j]) -
                                ((const float*)mn)[j]) * ((const float*)is)[j];
            const float g = bf16_to_f32(((const uint16_t*)&gz)[j]);
            const float v = ((const float*)sc)[j] *
                (g - (((const float*)b0)[j] + xhat * ((const float*)b1)[j]) * invM);
            ((uint16_t*)&out)[j] = f32_to_bf16(v);
        }
        *reinterpret_cast<short8*>(dx + i * 8) = out;
    }
}

// ---------------------------------------------------------------------------
// Small-M single-kernel forms.  BatchNorm is independent per channel, so a
// block that owns a few channels and walks ALL M rows holds the complete
// per-channel sums itself: no partials round trip, no second launch.  Grid
// C/8 (C/4 for the 4-channel backward), 256 threads, thread t takes rows
// t, t+256, ...  Pays only while M is small (bn_small_plan): the grid is a
// few dozen blocks, each streaming M rows of 16 B.
// ---------------------------------------------------------------------------

// fwd: finalize + apply.  The combine and the finalize arithmetic are the
// chain's own (combine_partials8, bn_finalize_channel), so y, work and the
// running statistics equal bn_finalize + bn_apply bit for bit.  The first
// four rows of x (and res) are fetched before the combine, whose latency
// they hide; M <= 1024 never loads after it.
template <bool RELU, bool RES>
__global__ void __launch_bounds__(256)
k_bn_fwd_small(const float* __restrict__ partials, int msplit,
               const float* __restrict__ gamma, const float* __restrict__ beta,
               float* __restrict__ running_mean,
               float* __restrict__ running_var, float* __restrict__ work,
               const uint16_t* __restrict__ x, const uint16_t* __restrict__ res,
               uint16_t* __restrict__ y, int64_t M, int C, float eps,
               float momentum, int update_running, float slope) {
    const int c0 = blockIdx.x * 8;
    short8 xv[4] = {}, rv[4] = {};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = threadIdx.x + 256 * r;
        if (m < M) {
            xv[r] = *reinterpret_cast<const short8*>(x + m * C + c0);
            if (RES) rv[r] = *reinterpret_cast<const short8*>(res + m * C + c0);
        }
    }
    float s, s2;
    combine_partials8(partials, msplit, C, &s, &s2);
    __shared__ float coef[2][8];
    if (threadIdx.x < 8) {
        float scale, shift;
        bn_finalize_channel(s, s2, c0 + threadIdx.x, gamma, beta, running_mean,
                            running_var, work, M, C, eps, momentum,
                            update_running, &scale, &shift);
        coef[0][threadIdx.x] = scale;
        coef[1][threadIdx.x] = shift;
    }
    __syncthreads();
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = coef[0][j];
        sh[j] = coef[1][j];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = threadIdx.x + 256 * r;
        if (m < M) {
            short8 out;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                ((uint16_t*)&out)[j] = bn_apply_elem<RELU, RES>(
                    ((const uint16_t*)&xv[r])[j], ((const uint16_t*)&rv[r])[j],
                    sc[j], sh[j], slope);
            *reinterpret_cast<short8*>(y + m * C + c0) = out;
        }
    }
    for (int64_t m = threadIdx.x + 1024; m < M; m += 256) {
        const int64_t off = m * C + c0;
        const short8 xr = *reinterpret_cast<const short8*>(x + off);
        short8 rr = {};
        if (RES) rr = *reinterpret_cast<const short8*>(res + off);
        short8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            ((uint16_t*)&out)[j] = bn_apply_elem<RELU, RES>(
                ((const uint16_t*)&xr)[j], ((const uint16_t*)&rr)[j],
                sc[j], sh[j], slope);
        *reinterpret_cast<short8*>(y + off) = out;
    }
}

template <int CW> struct bn_vec {
    using type = __attribute__((ext_vector_type(CW))) short;
};

// One row of backward pass 1: dz = bf16(dy * relu-mask), sums of the
// unrounded g and g*xhat — the expressions of k_bn_bwd_reduce.
template <bool RELU, int CW>
__device__ __forceinline__ void bn_bwd_row(
        const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
        const uint16_t* __restrict__ x, int64_t off, const float* mean,
        const float* invstd, float slope, float* s, float* sx,
        typename bn_vec<CW>::type* dz_out, typename bn_vec<CW>::type* x_out) {
    using vec = typename bn_vec<CW>::type;
    const vec gv = *reinterpret_cast<const vec*>(dy + off);
    const vec xv = *reinterpret_cast<const vec*>(x + off);
    vec yv = {};
    if (RELU) yv = *reinterpret_cast<const vec*>(y + off);
    vec dzv;
#pragma unroll
    for (int j = 0; j < CW; ++j) {
        float g = bf16_to_f32(((const uint16_t*)&gv)[j]);
        if (RELU && bf16_to_f32(((const uint16_t*)&yv)[j]) <= 0.f)
            g *= slope;
        ((uint16_t*)&dzv)[j] = f32_to_bf16(g);
        s[j] += g;
        const float xh = (bf16_to_f32(((const uint16_t*)&xv)[j]) - mean[j]) * invstd[j];
        sx[j] = fmaf(g, xh, sx[j]);
    }
    *dz_out = dzv;
    *x_out = xv;
}

// bwd: reduce + grads + apply.  Pass 1 sums g and g*xhat per thread (dz is
// stored only when WRITE_DZ: it is the residual branch's gradient and has no
// other reader); the 256 threads' sums fold through LDS in a fixed order (no
// atomics: bitwise repeatable); dbeta/dgamma += the sums; pass 2 writes dx
// from the bf16-rounded dz, as the chain's apply reads it.
// The R rows of a thread (M <= 256*R) stay in registers between the passes;
// re-reading them in pass 2 instead lost everywhere in the sweep and is gone,
// as is a 4-channel block (CW stays a parameter; only 8 is instantiated).
// Blocks are dispatched round-robin over the 8 XCDs, and 64/CW neighbouring
// channel groups share each 128-byte line of a row: block b takes group
// (b%8)*(grid/8) + b/8, so the blocks one XCD receives own adjacent groups
// and its L2 fetches a line once (placement only; any order is correct).
template <bool RELU, bool WRITE_DZ, int CW, int R>
__global__ void __launch_bounds__(256)
k_bn_bwd_small(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
               const uint16_t* __restrict__ x, const float* __restrict__ work,
               uint16_t* __restrict__ dz_out, float* __restrict__ dgamma,
               float* __restrict__ dbeta, uint16_t* __restrict__ dx,
               int64_t M, int C, float slope) {
    using vec = typename bn_vec<CW>::type;
    constexpr int NQ = 128 / CW;      // fold stage 1: row groups per sum kind
    int grp = blockIdx.x;
    if (gridDim.x % 8 == 0)
        grp = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int c0 = grp * CW;
    const int t = threadIdx.x;
    float mean[CW], invstd[CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) {
        mean[j] = work[c0 + j];
        invstd[j] = work[C + c0 + j];
    }
    float s[CW] = {}, sx[CW] = {};
    vec dzk[R], xk[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t m = t + 256 * r;
        if (m < M) {
            const int64_t off = m * C + c0;
            bn_bwd_row<RELU, CW>(dy, y, x, off, mean, invstd, slope, s, sx,
                                 &dzk[r], &xk[r]);
            if (WRITE_DZ) *reinterpret_cast<vec*>(dz_out + off) = dzk[r];
        }
    }
    // fold: red[kind][thread][ch] -> NQ row-group sums per (kind, ch) -> one
    __shared__ float red[2][256][CW];
    __shared__ float red2[2][NQ][CW];
    __shared__ float fin[2][CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) {
        red[0][t][j] = s[j];
        red[1][t][j] = sx[j];
    }
    __syncthreads();
    {
        const int kind = t >> 7, q = t & 127;
        const int k = q / CW, ch = q % CW;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 256 / NQ; ++i) acc += red[kind][k + NQ * i][ch];
        red2[kind][k][ch] = acc;
    }
    __syncthreads();
    if (t < 2 * CW) {
        const int kind = t / CW, ch = t % CW;
        float acc = 0.f;
#pragma unroll 8
        for (int k = 0; k < NQ; ++k) acc += red2[kind][k][ch];
        fin[kind][ch] = acc;
        if (kind == 0) dbeta[c0 + ch] += acc;
        else dgamma[c0 + ch] += acc;
    }
    __syncthreads();
    const float invM = 1.f / (float)M;
    float sc[CW], b0[CW], b1[CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) {
        sc[j] = work[2 * (int64_t)C + c0 + j];
        b0[j] = fin[0][j] * invM;
        b1[j] = fin[1][j] * invM;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t m = t + 256 * r;
        if (m < M) {
            vec out;
#pragma unroll
            for (int j = 0; j < CW; ++j)
                ((uint16_t*)&out)[j] = bn_bwd_dx_elem(
                    ((const uint16_t*)&dzk[r])[j], ((const uint16_t*)&xk[r])[j],
                    mean[j], invstd[j], sc[j], b0[j], b1[j]);
            *reinterpret_cast<vec*>(dx + m * C + c0) = out;
        }
    }
}

// ---------------------------------------------------------------------------
// launchers (msplit chosen by the Python wrapper, shared by both phases)
// ---------------------------------------------------------------------------

extern "C" void launch_bn_stats(const void* x, void* partials, int64_t M, int C,
                                int msplit, hipStream_t stream) {
    const int mpb = (int)((M + msplit - 1) / msplit);
    dim3 grid((unsigned)(C / 64), (unsigned)msplit);
    k_bn_stats<<<grid, 256, 0, stream>>>((const uint16_t*)x, (float*)partials,
                                         M, C, msplit, mpb);
}

extern "C" void launch_bn_finalize(const void* partials, int msplit,
                                   const void* gamma, const void* beta,
                                   void* running_mean, void* running_var,
                                   void* work, int64_t M, int C, float eps,
                                   float momentum, int update_running,
                                   hipStream_t stream) {
    k_bn_finalize<<<C / 8, 256, 0, stream>>>(
        (const float*)partials, msplit, (const float*)gamma,
        (const float*)beta, (float*)running_mean, (float*)running_var,
        (float*)work, M, C, eps, momentum, update_running);
}

extern "C" void launch_bn_apply(const void* x, const void* res, void* y,
                                const void* work, int64_t M, int C, int relu,
                                float slope, hipStream_t stream) {
    if (C % 64 == 0) {
        const int mpb = apply_mpb(M, C);
        dim3 g((unsigned)(C / 64), (unsigned)((M + mpb - 1) / mpb));
        if (relu && res)
            k_bn_apply_c64<true, true><<<g, 256, 0, stream>>>(
                (const uint16_t*)x, (const uint16_t*)res, (uint16_t*)y,
                (const float*)work, M, C, slope, mpb);
        else if (relu)
            k_bn_apply_c64<true, false><<<g, 256, 0, stream>>>(
                (const uint16_t*)x, nullptr, (uint16_t*)y,
                (const float*)work, M, C, slope, mpb);
        else if (res)
            k_bn_apply_c64<false, true><<<g, 256, 0, stream>>>(
                (const uint16_t*)x, (const uint16_t*)res, (uint16_t*)y,
                (const float*)work, M, C, slope, mpb);
        else
            k_bn_apply_c64<false, false><<<g, 256, 0, stream>>>(
                (const uint16_t*)x, nullptr, (uint16_t*)y,
                (const float*)work, M, C, slope, mpb);
        return;
    }
    const int grid = ew_grid(M * C / 8, 256, 4);
    if (relu && res)
        k_bn_apply<true, true><<<grid, 256, 0, stream>>>(
            (const uint16_t*)x, (const uint16_t*)res, (uint16_t*)y,
            (const float*)work, M, C, slope);
    else if (relu)
        k_bn_apply<true, false><<<grid, 256, 0, stream>>>(
            (const uint16_t*)x, nullptr, (uint16_t*)y, (const float*)work, M, C, slope);
    else if (res)
        k_bn_apply<false, true><<<grid, 256, 0, stream>>>(
            (const uint16_t*)x, (const uint16_t*)res, (uint16_t*)y,
            (const float*)work, M, C, slope);
    else
        k_bn_apply<false, false><<<grid, 256, 0, stream>>>(
            (const uint16_t*)x, nullptr, (uint16_t*)y, (const float*)work, M, C, slope);
}

extern "C" void launch_bn_bwd_reduce(const void* dy, const void* y,
                                     const void* x, const void* work,
                                     void* dz_out, void* partials, int64_t M,
                                     int C, int msplit, int relu, float slope,
                                     hipStream_t stream) {
    const int mpb = (int)((M + msplit - 1) / msplit);
    dim3 grid((unsigned)(C / 64), (unsigned)msplit);
    if (relu)
        k_bn_bwd_reduce<true><<<grid, 256, 0, stream>>>(
            (const uint16_t*)dy, (const uint16_t*)y, (const uint16_t*)x,
            (const float*)work, (uint16_t*)dz_out, (float*)partials, M, C,
            msplit, mpb, slope);
    else
        k_bn_bwd_reduce<false><<<grid, 256, 0, stream>>>(
            (const uint16_t*)dy, (const uint16_t*)y, (const uint16_t*)x,
            (const float*)work, (uint16_t*)dz_out, (float*)partials, M, C,
            msplit, mpb, slope);
}

extern "C" void launch_bn_bwd_grads(const void* partials, int msplit,
                                    void* bsums, void* dgamma, void* dbeta,
                                    int C, hipStream_t stream) {
    k_bn_bwd_grads<<<C / 8, 256, 0, stream>>>(
        (const float*)partials, msplit, (float*)bsums, (float*)dgamma,
        (float*)dbeta, C);
}

extern "C" void launch_bn_bwd_apply(const void* dz, const void* x,
                                    const void* work, const void* bsums,
                                    void* dx, int64_t M, int C,
                                    hipStream_t stream) {
    if (C % 64 == 0) {
        const int mpb = apply_mpb(M, C);
        dim3 g((unsigned)(C / 64), (unsigned)((M + mpb - 1) / mpb));
        k_bn_bwd_apply_c64<<<g, 256, 0, stream>>>(
            (const uint16_t*)dz, (const uint16_t*)x, (const float*)work,
            (const float*)bsums, (uint16_t*)dx, M, C, mpb);
        return;
    }
    const int grid = ew_grid(M * C / 8, 256, 4);
    k_bn_bwd_apply<<<grid, 256, 0, stream>>>(
        (const uint16_t*)dz, (const uint16_t*)x, (const float*)work,
        (const float*)bsums, (uint16_t*)dx, M, C);
}

// ---------------------------------------------------------------------------
// small-M single-kernel forms: plan + launchers
// ---------------------------------------------------------------------------

// Forward and backward have one form each (1); 0 = the existing chain.
static inline int bn_bwd_small_rows(int64_t M) {
    return M <= 1024 ? 4 : M <= 4096 ? 16 : 0;   // rows/thread kept, 0 = none
}

// The one place that decides which BatchNorms take the single-kernel forms.
// Thresholds from scripts/bn_small_sweep.py (profiles/README.md, r06a): a
// block's time grows with M whatever C is.  Backward beats the chain up to
// M = 1024 (with and without the dz write) and loses at 3136 and 4096;
// forward, whose block order is tied to combine_partials8, wins at 512 and
// already loses at 1024.
// C % 64 != 0 is declined although the forms could run C % 8 == 0: the
// partials they read come from k_bn_stats or a conv epilogue, both 64-channel
// groups, so such a BatchNorm has no forward statistics to begin with and
// the wrappers of the chain refuse it.
extern "C" void bn_small_plan(int64_t M, int C, int* fwd_form, int* bwd_form) {
    *fwd_form = 0;
    *bwd_form = 0;
    if (M < 1 || C < 64 || C % 64) return;
    if (M <= 512) *fwd_form = 1;
    if (M <= 1024) *bwd_form = 1;
}

extern "C" int launch_bn_fwd_small(const void* partials, int msplit,
                                   const void* gamma, const void* beta,
                                   void* running_mean, void* running_var,
                                   void* work, const void* x, const void* res,
                                   void* y, int64_t M, int C, float eps,
                                   float momentum, int update_running,
                                   int relu, float slope, int form,
                                   hipStream_t stream) {
    if (form != 1 || M < 1 || C < 8 || C % 8) return 0;
#define BN_FWD_SMALL(RELU, RES)                                               \
    k_bn_fwd_small<RELU, RES><<<C / 8, 256, 0, stream>>>(                     \
        (const float*)partials, msplit, (const float*)gamma,                  \
        (const float*)beta, (float*)running_mean, (float*)running_var,        \
        (float*)work, (const uint16_t*)x, (const uint16_t*)res, (uint16_t*)y, \
        M, C, eps, momentum, update_running, slope)
    if (relu && res) BN_FWD_SMALL(true, true);
    else if (relu) BN_FWD_SMALL(true, false);
    else if (res) BN_FWD_SMALL(false, true);
    else BN_FWD_SMALL(false, false);
#undef BN_FWD_SMALL
    return 1;
}

template <int CW, int R>
static void bn_bwd_small_launch(const void* dy, const void* y, const void* x,
                                const void* work, void* dz, void* dgamma,
                                void* dbeta, void* dx, int64_t M, int C,
                                int relu, float slope, int write_dz,
                                hipStream_t stream) {
#define BN_BWD_SMALL(RELU, WDZ)                                               \
    k_bn_bwd_small<RELU, WDZ, CW, R><<<C / CW, 256, 0, stream>>>(             \
        (const uint16_t*)dy, (const uint16_t*)y, (const uint16_t*)x,          \
        (const float*)work, (uint16_t*)dz, (float*)dgamma, (float*)dbeta,     \
        (uint16_t*)dx, M, C, slope)
    if (relu && write_dz) BN_BWD_SMALL(true, true);
    else if (relu) BN_BWD_SMALL(true, false);
    else if (write_dz) BN_BWD_SMALL(false, true);
    else BN_BWD_SMALL(false, false);
#undef BN_BWD_SMALL
}

extern "C" int launch_bn_bwd_small(const void* dy, const void* y,
                                   const void* x, const void* work, void* dz,
                                   void* dgamma, void* dbeta, void* dx,
                                   int64_t M, int C, int relu, float slope,
                                   int write_dz, int form,
                                   hipStream_t stream) {
    if (form != 1 || M < 1 || C < 8 || C % 8) return 0;
    const int rows = bn_bwd_small_rows(M);
    if (!rows) return 0;
#define BN_BWD_GO(CW, R)                                                      \
    bn_bwd_small_launch<CW, R>(dy, y, x, work, dz, dgamma, dbeta, dx, M, C,   \
                               relu, slope, write_dz, stream)
    if (rows == 4) BN_BWD_GO(8, 4);
    else BN_BWD_GO(8, 16);
#undef BN_BWD_GO
    return 1;
}

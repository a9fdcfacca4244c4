// Copyright (c) Flashy-AMD authors.
// Device helpers shared by the row kernels of layernorm.hip and grn.hip: the
// 16-byte octet loads and stores, the per-block parameter loads, the barrier
// and the erf code of bias+GELU.  layernorm.hip's header comment describes the
// thread layout they serve and where the erf fit comes from.
#pragma once

#include "common.h"

#define LN_THREADS 256
#define LN_MAXG 64              // lanes of a group, at most one wave
#define LN_CHUNK 512            // channels of one elementwise column chunk

// k_colsum_combine of layernorm.hip: d_j[c] += sum over the slices of
// ws[slice][j][c] (fp32 [slices][k][C]) for every non-null d_j
void ln_combine(const void* ws, void* d0, void* d1, void* d2, int k, int C,
                int slices, hipStream_t stream);

// Compiled without packed fp32 math, as the kernels that inline these are
// (see fused_optim.hip for why).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// what __syncthreads expands to
__device__ __forceinline__ void ln_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void ln_load8(const uint16_t* __restrict__ p,
                                         int64_t at, float f[8]) {
    const short8 v = *reinterpret_cast<const short8*>(p + at);
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = bf16_to_f32((uint16_t)v[c]);
}

__device__ __forceinline__ void ln_store8(uint16_t* __restrict__ p, int64_t at,
                                          const float f[8]) {
    short8 v;
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = (short)f32_to_bf16(f[c]);
    *reinterpret_cast<short8*>(p + at) = v;
}

// 8 fp32 parameters at channel ch; `fill` where the lane is idle or the
// parameter is absent.  Scalar loads: a parameter may be a 4-byte aligned
// view into a flat arena, and this runs once per block.
__device__ __forceinline__ void ln_param8(const float* __restrict__ p, int ch,
                                          bool on, float fill, float f[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = (on && p) ? p[ch + c] : fill;
}

// Phi(u) (normal CDF) and phi(u) (density); gelu(u) = u * Phi(u)
__device__ __forceinline__ void ln_gauss(float u, float* Phi, float* phi) {
    const float z = __builtin_fabsf(u) * 0.70710678f;
    const float t = 1.f / __builtin_fmaf(0.3275911f, z, 1.f);
    // exp(-u^2 / 2) with the rounding of the square put back
    const float sq = u * u;
    const float e = __builtin_expf(-0.5f * sq) *
                    __builtin_fmaf(-0.5f, __builtin_fmaf(u, u, -sq), 1.f);
    float poly = 5.750628480e-02f;
    poly = __builtin_fmaf(poly, t, -3.215564865e-01f);
    poly = __builtin_fmaf(poly, t, 6.375867681e-01f);
    poly = __builtin_fmaf(poly, t, -5.734744838e-01f);
    poly = __builtin_fmaf(poly, t, 5.123662973e-01f);
    poly = __builtin_fmaf(poly, t, -5.620583739e-02f);
    poly = __builtin_fmaf(poly, t, 2.079440067e-01f);
    poly = __builtin_fmaf(poly, t, 1.652116966e-01f);
    poly = __builtin_fmaf(poly, t, 1.858453488e-01f);
    poly = __builtin_fmaf(poly, t, 1.847764033e-01f);
    const float tail = 0.5f * poly * t * e;        // 0.5 * erfc(|z|)
    *Phi = u < 0.f ? tail : 1.f - tail;
    *phi = 0.39894228f * e;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

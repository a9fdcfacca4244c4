// Copyright (c) Flashy-AMD authors.
// Classifier head for gfx950: global average pool over an NHWC bf16 trunk
// output fused with the small fp32 fc layer.
//
//   fwd:  pooled[n][c] = (1/HW) * sum_hw x[n][hw][c]        (fp32, saved)
//         y[n][o]      = b[o] + sum_c pooled[n][c] * w[o][c]
//   bwd:  dw[o][c] += sum_n dy[n][o] * pooled[n][c];  db[o] += sum_n dy[n][o]
//         dx[n][hw][c] = bf16((1/HW) * sum_o dy[n][o] * w[o][c])  for every hw
//
// Replaces the bf16->f32 cast + mean reduce + k_linear_fwd forward chain and
// the k_linear_dw/k_linear_dx + mean/cast autograd backward chain (nine
// launches for a 64x512->10 problem) with three.  All three kernels are
// deterministic: fixed in-thread / shuffle reduction orders, no atomics.
//
// Both ends also run WITHOUT the fc half (w == nullptr): that is the plain
// pool forward / backward pair used in front of a large rocBLAS head.
//
// Thread mapping shared by fwd and dx: a block's 256 threads are `cols`
// channel-octets x `rl` row lanes (cols = min(C/8, 256), rl = 256/cols);
// every global access is one 16 B piece.  Requires C % 8 == 0.

#include "common.h"

__global__ void __launch_bounds__(256)
k_pool_fc_fwd(const uint16_t* __restrict__ x, const float* __restrict__ w,
              const float* __restrict__ bias, float* __restrict__ pooled,
              float* __restrict__ y, int HW, int C, int O, int cols, int rl) {
    extern __shared__ float part[];               // [rl][C]
    const int n = blockIdx.x;
    const int col = threadIdx.x % cols;
    const int row = threadIdx.x / cols;
    const uint16_t* xn = x + (int64_t)n * HW * C;
    if (row < rl) {
        for (int c8 = col * 8; c8 < C; c8 += cols * 8) {
            float s[8] = {};
#pragma unroll 4
            for (int hw = row; hw < HW; hw += rl) {
                const short8 v8 = *reinterpret_cast<const short8*>(
                    xn + (int64_t)hw * C + c8);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    s[j] += bf16_to_f32(((const uint16_t*)&v8)[j]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) part[row * C + c8 + j] = s[j];
        }
    }
    __syncthreads();
    // fold the row lanes; column c is read and rewritten by one thread only
    const float inv = 1.f / (float)HW;
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = part[c];
        for (int r = 1; r < rl; ++r) acc += part[r * C + c];
        acc *= inv;
        part[c] = acc;
        pooled[(int64_t)n * C + c] = acc;
    }
    if (w == nullptr) return;
    __syncthreads();
    // one wave per output: float4 weight loads against the LDS-resident row
    const int lane = threadIdx.x & 63;
    for (int o = threadIdx.x >> 6; o < O; o += 4) {
        const float* wr = w + (int64_t)o * C;
        float acc = 0.f;
        for (int c = lane * 4; c < C; c += 256) {
            const float4 wv = *reinterpret_cast<const float4*>(wr + c);
            acc = fmaf(part[c], wv.x, acc);
            acc = fmaf(part[c + 1], wv.y, acc);
            acc = fmaf(part[c + 2], wv.z, acc);
            acc = fmaf(part[c + 3], wv.w, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0)
            y[(int64_t)n * O + o] = acc + (bias != nullptr ? bias[o] : 0.f);
    }
}

// dw[o][c] += sum_n dy[n][o] * pooled[n][c];  db[o] += sum_n dy[n][o].
// Thread per (o, c); the batch reduction runs in-thread in n order, so the
// result does not depend on the launch shape.  dw or db may be null (frozen).
__global__ void __launch_bounds__(256)
k_head_dw(const float* __restrict__ pooled, const float* __restrict__ dy,
          float* __restrict__ dw, float* __restrict__ db,
          int B, int C, int O) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= O * C) return;
    const int o = idx / C, c = idx - o * C;
    if (dw != nullptr) {
        float acc = 0.f;
#pragma unroll 8
        for (int n = 0; n < B; ++n)
            acc = fmaf(dy[(int64_t)n * O + o], pooled[(int64_t)n * C + c], acc);
        dw[idx] += acc;
    }
    if (db != nullptr && c == 0) {
        float bs = 0.f;
        for (int n = 0; n < B; ++n) bs += dy[(int64_t)n * O + o];
        db[o] += bs;
    }
}

// dx[n][hw][c] = bf16(inv_hw * g[n][c]) for every hw, with
//   g[n][c] = sum_o dy[n][o] * w[o][c]   (fused head), or
//   g[n][c] = dy[n][c]                   (w == nullptr: plain pool backward).
// grid (N, hw splits): each block recomputes its 8-channel g (O fmas per
// channel) and streams its share of the HW rows in 16 B stores.
__global__ void __launch_bounds__(256)
k_head_dx(const float* __restrict__ dy, const float* __restrict__ w,
          uint16_t* __restrict__ dx, int HW, int C, int O, int cols, int rl,
          int hw_per_block) {
    const int n = blockIdx.x;
    const int col = threadIdx.x % cols;
    const int row = threadIdx.x / cols;
    if (row >= rl) return;
    const int hw0 = blockIdx.y * hw_per_block;
    const int hw1 = min(hw0 + hw_per_block, HW);
    const float inv = 1.f / (float)HW;
    uint16_t* dxn = dx + (int64_t)n * HW * C;
    for (int c8 = col * 8; c8 < C; c8 += cols * 8) {
        float g[8];
        if (w != nullptr) {
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = 0.f;
            for (int o = 0; o < O; ++o) {
                const float d = dy[(int64_t)n * O + o];
                const float4 w0 = *reinterpret_cast<const float4*>(
                    w + (int64_t)o * C + c8);
                const float4 w1 = *reinterpret_cast<const float4*>(
                    w + (int64_t)o * C + c8 + 4);
                g[0] = fmaf(d, w0.x, g[0]); g[1] = fmaf(d, w0.y, g[1]);
                g[2] = fmaf(d, w0.z, g[2]); g[3] = fmaf(d, w0.w, g[3]);
                g[4] = fmaf(d, w1.x, g[4]); g[5] = fmaf(d, w1.y, g[5]);
                g[6] = fmaf(d, w1.z, g[6]); g[7] = fmaf(d, w1.w, g[7]);
            }
        } else {
            const float4 g0 = *reinterpret_cast<const float4*>(
                dy + (int64_t)n * C + c8);
            const float4 g1 = *reinterpret_cast<const float4*>(
                dy + (int64_t)n * C + c8 + 4);
            g[0] = g0.x; g[1] = g0.y; g[2] = g0.z; g[3] = g0.w;
            g[4] = g1.x; g[5] = g1.y; g[6] = g1.z; g[7] = g1.w;
        }
        short8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            ((uint16_t*)&out)[j] = f32_to_bf16(g[j] * inv);
        for (int hw = hw0 + row; hw < hw1; hw += rl)
            *reinterpret_cast<short8*>(dxn + (int64_t)hw * C + c8) = out;
    }
}

static inline void head_geometry(int C, int* cols, int* rl) {
    const int noct = C / 8;
    *cols = noct < 256 ? noct : 256;
    *rl = 256 / *cols;
}

// w == nullptr: pool forward only (y, bias unused)
extern "C" void launch_pool_fc_fwd(const void* x, const void* w, const void* b,
                                   void* pooled, void* y, int N, int HW, int C,
                                   int O, hipStream_t stream) {
    int cols, rl;
    head_geometry(C, &cols, &rl);
    const size_t lds = (size_t)rl * C * sizeof(float);
    k_pool_fc_fwd<<<(unsigned)N, 256, lds, stream>>>(
        (const uint16_t*)x, (const float*)w, (const float*)b, (float*)pooled,
        (float*)y, HW, C, O, cols, rl);
}

extern "C" void launch_head_dw(const void* pooled, const void* dy, void* dw,
                               void* db, int B, int C, int O,
                               hipStream_t stream) {
    k_head_dw<<<(unsigned)((O * C + 255) / 256), 256, 0, stream>>>(
        (const float*)pooled, (const float*)dy, (float*)dw, (float*)db, B, C,
        O);
}

// w == nullptr: pool backward only (dy is the fp32 [N][C] pooled gradient)
extern "C" void launch_head_dx(const void* dy, const void* w, void* dx, int N,
                               int HW, int C, int O, hipStream_t stream) {
    int cols, rl;
    head_geometry(C, &cols, &rl);
    // enough (n, hw-split) blocks to cover the chip's 256 CUs
    int split = (256 + N - 1) / N;
    const int max_split = (HW + rl - 1) / rl;
    if (split > max_split) split = max_split;
    if (split < 1) split = 1;
    const int hpb = (HW + split - 1) / split;
    dim3 grid((unsigned)N, (unsigned)((HW + hpb - 1) / hpb));
    k_head_dx<<<grid, 256, 0, stream>>>(
        (const float*)dy, (const float*)w, (uint16_t*)dx, HW, C, O, cols, rl,
        hpb);
}

// Copyright (c) Flashy-AMD authors.
// On-device image ingest for gfx950: random crop (with padding), horizontal
// flip and per-channel normalization, fused, from a uint8 NHWC batch to the
// bf16 NHWC tensor the native models consume.
//
// One launch per batch.  The per-sample draw (dy, dx, flip) is a pure
// function of (seed, *step_ptr, sample index), so a captured (HIP-graph)
// step crops differently on every replay with no host involvement — the
// same idea as Adam's on-device step counter, which the caller advances
// after this kernel with launch_adam_step_inc.  flashy_amd/data.py mirrors
// the hash bit for bit (DeviceAugment.params_at).
//
// Memory-bound: 3 B in, 6 B out per pixel.  A thread produces INGEST_PIX
// consecutive output pixels of one row (12 bf16 = three 8-byte stores when
// the address is 8-byte aligned, which holds for every item when OW % 4 ==
// 0); row tails and unaligned rows take scalar stores.  An item whose 4
// source pixels all lie inside the image reads its 12 contiguous bytes as
// three dwords (their address depends on the per-sample dx, so they are
// unaligned, which global loads allow); items touching the border read
// byte by byte.  Grid-stride over <= 2048 blocks.

#include "common.h"

#define INGEST_PIX 4

struct IngestArgs {
    const uint8_t* __restrict__ src;  // [N, H, W, 3]
    uint16_t* __restrict__ out;       // [N, OH, OW, 3] bf16 payload
    const long long* step_ptr;        // device step counter (train only)
    int N, H, W, OH, OW, pad;
    unsigned long long seed;
    unsigned int flip_thresh;         // round(p_flip * 2^24)
    float scale[3], bias[3];
    int fill, train;
};

__device__ __forceinline__ unsigned long long ingest_mix(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__global__ void __launch_bounds__(256)
k_image_ingest(IngestArgs a) {
    const unsigned long long G = 0x9E3779B97F4A7C15ull;
    const unsigned int ny = (unsigned int)(a.H + 2 * a.pad - a.OH + 1);
    const unsigned int nx = (unsigned int)(a.W + 2 * a.pad - a.OW + 1);
    unsigned long long step_key = 0;
    if (a.train) {
        const unsigned long long step = (unsigned long long)*a.step_ptr;
        step_key = ingest_mix(a.seed + G * (step + 1));
    }
    const float pad_v[3] = {fmaf((float)a.fill, a.scale[0], a.bias[0]),
                            fmaf((float)a.fill, a.scale[1], a.bias[1]),
                            fmaf((float)a.fill, a.scale[2], a.bias[2])};
    const uint16_t pad_b[3] = {f32_to_bf16(pad_v[0]), f32_to_bf16(pad_v[1]),
                               f32_to_bf16(pad_v[2])};

    const int groups = (a.OW + INGEST_PIX - 1) / INGEST_PIX;  // per row
    const int64_t items = (int64_t)a.N * a.OH * groups;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         it < items; it += stride) {
        const int64_t row = it / groups;          // n * OH + oy
        const int ox0 = (int)(it - row * groups) * INGEST_PIX;
        const int n = (int)(row / a.OH);
        const int oy = (int)(row - (int64_t)n * a.OH);

        int dy = (int)(ny - 1) / 2, dx = (int)(nx - 1) / 2;
        bool flip = false;
        if (a.train) {
            const unsigned long long h1 =
                ingest_mix(step_key + G * ((unsigned long long)n + 1));
            const unsigned long long h2 = ingest_mix(h1 + G);
            dy = (int)(((h1 & 0xffffffffull) * ny) >> 32);
            dx = (int)(((h1 >> 32) * nx) >> 32);
            flip = (unsigned int)(h2 >> 40) < a.flip_thresh;
        }

        const int sy = oy + dy - a.pad;
        const bool row_in = sy >= 0 && sy < a.H;
        const uint8_t* srow = a.src + ((int64_t)n * a.H + (row_in ? sy : 0)) *
                                          ((int64_t)a.W * 3);
        const int cnt = a.OW - ox0 < INGEST_PIX ? a.OW - ox0 : INGEST_PIX;

        uint16_t v[INGEST_PIX * 3];
        // source x of this item's leftmost source pixel (its last output
        // pixel when flipped)
        const int sx_lo = flip ? a.OW - ox0 - INGEST_PIX + dx - a.pad
                               : ox0 + dx - a.pad;
        if (row_in && cnt == INGEST_PIX && sx_lo >= 0 &&
            sx_lo + INGEST_PIX <= a.W) {
            // interior: the 12 source bytes are contiguous and all inside
            // the row -> three (unaligned) dword loads instead of 12 bytes
            uint32_t w[INGEST_PIX * 3 / 4];
            __builtin_memcpy(w, srow + sx_lo * 3, sizeof(w));
#pragma unroll
            for (int j = 0; j < INGEST_PIX; ++j) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int kf = (INGEST_PIX - 1 - j) * 3 + c;  // flipped
                    const int kn = j * 3 + c;
                    const uint32_t bf = (w[kf >> 2] >> (8 * (kf & 3))) & 0xffu;
                    const uint32_t bn = (w[kn >> 2] >> (8 * (kn & 3))) & 0xffu;
                    v[kn] = f32_to_bf16(fmaf((float)(flip ? bf : bn),
                                             a.scale[c], a.bias[c]));
                }
            }
        } else {
            // borders, tails: byte by byte, the fill value outside
#pragma unroll
            for (int j = 0; j < INGEST_PIX; ++j) {
                const int ox = ox0 + j;
                const int sx = (flip ? a.OW - 1 - ox : ox) + dx - a.pad;
                // ox < OW keeps the tail group's unused pixels from reading
                const bool in = row_in && ox < a.OW && sx >= 0 && sx < a.W;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    uint16_t b = pad_b[c];
                    if (in)
                        b = f32_to_bf16(fmaf((float)srow[sx * 3 + c],
                                             a.scale[c], a.bias[c]));
                    v[j * 3 + c] = b;
                }
            }
        }

        uint16_t* dst = a.out + (row * a.OW + ox0) * 3;
        if (cnt == INGEST_PIX && ((uintptr_t)dst & 7u) == 0) {
            ushort4* d4 = reinterpret_cast<ushort4*>(dst);
#pragma unroll
            for (int k = 0; k < INGEST_PIX * 3 / 4; ++k)
                d4[k] = ushort4{v[k * 4], v[k * 4 + 1], v[k * 4 + 2],
                                v[k * 4 + 3]};
        } else {
#pragma unroll
            for (int j = 0; j < INGEST_PIX; ++j) {
                if (j < cnt) {
                    dst[j * 3] = v[j * 3];
                    dst[j * 3 + 1] = v[j * 3 + 1];
                    dst[j * 3 + 2] = v[j * 3 + 2];
                }
            }
        }
    }
}

extern "C" void launch_image_ingest(const void* src, void* out,
                                    const void* step_dev, int N, int H, int W,
                                    int OH, int OW, int pad, uint64_t seed,
                                    uint32_t flip_thresh, const float* scale,
                                    const float* bias, int fill, int train,
                                    hipStream_t stream) {
    IngestArgs a{};
    a.src = (const uint8_t*)src;
    a.out = (uint16_t*)out;
    a.step_ptr = (const long long*)step_dev;
    a.N = N; a.H = H; a.W = W; a.OH = OH; a.OW = OW; a.pad = pad;
    a.seed = seed;
    a.flip_thresh = flip_thresh;
    for (int c = 0; c < 3; ++c) { a.scale[c] = scale[c]; a.bias[c] = bias[c]; }
    a.fill = fill;
    a.train = train;
    const int groups = (OW + INGEST_PIX - 1) / INGEST_PIX;
    const int grid = ew_grid((int64_t)N * OH * groups, 256, 1);
    k_image_ingest<<<grid, 256, 0, stream>>>(a);
}

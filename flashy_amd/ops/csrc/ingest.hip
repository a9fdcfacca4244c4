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

// ---------------------------------------------------------------------------
// Random resized crop (flashy_amd.data.DeviceResizedCrop): a draw kernel
// that writes one box per sample, then a bilinear resample of each box to
// the output size with flip and normalize fused.
//
// The draw is torchvision's RandomResizedCrop in integers: the host
// tabulates sqrt(area fraction), sqrt(ratio) and 1/sqrt(ratio) in Q16 at
// RC_TABLE levels and passes rootHW = isqrt((H*W) << 32), so no exp / log /
// sqrt runs here and DeviceResizedCrop.boxes_at reproduces every box bit
// for bit.  The 64-bit divisions (the resample steps, the fallback box)
// happen in the draw, once per sample, not per pixel.
// ---------------------------------------------------------------------------

#define RC_TABLE 1024
#define RC_TRIES 10

struct ResizedCropDrawArgs {
    int* __restrict__ boxes;          // [N, 8] (y0, x0, h, w, flip, step_y,
                                      //         step_x, fallback)
    const int* __restrict__ tables;   // [3, RC_TABLE] Q16: SA, SR, SRI
    const long long* step_ptr;        // device step counter (train only)
    int N, H, W, OH, OW;
    unsigned long long seed, root_hw;
    unsigned int flip_thresh;         // round(p_flip * 2^24)
    unsigned int r0, r1, eval_crop;   // Q16
    int train;
};

__global__ void __launch_bounds__(256)
k_resized_crop_draw(ResizedCropDrawArgs a) {
    typedef unsigned long long u64;
    const u64 G = 0x9E3779B97F4A7C15ull;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    const u64 H = (u64)a.H, W = (u64)a.W;
    u64 y0, x0, h, w;
    int flip = 0, fallback = 0;
    if (a.train) {
        const u64 step = (u64)*a.step_ptr;
        const u64 key = ingest_mix(a.seed + G * (step + 1));
        const u64 h0 = ingest_mix(key + G * ((u64)n + 1));
        bool found = false;
        for (int t = 0; t < RC_TRIES && !found; ++t) {
            const u64 ra = ingest_mix(h0 + G * (u64)(2 * t + 1));
            const int ja = (int)(((ra & 0xffffffffull) * RC_TABLE) >> 32);
            const int jr = (int)(((ra >> 32) * RC_TABLE) >> 32);
            const u64 side = (a.root_hw * (u64)a.tables[ja]) >> 16;
            w = (side * (u64)a.tables[RC_TABLE + jr] + (1ull << 31)) >> 32;
            h = (side * (u64)a.tables[2 * RC_TABLE + jr] + (1ull << 31)) >> 32;
            if (w >= 1 && w <= W && h >= 1 && h <= H) {
                const u64 rb = ingest_mix(h0 + G * (u64)(2 * t + 2));
                y0 = ((rb & 0xffffffffull) * (H - h + 1)) >> 32;
                x0 = ((rb >> 32) * (W - w + 1)) >> 32;
                found = true;
            }
        }
        if (!found) {
            // whole image when W/H lies within the ratio bounds, else the
            // largest centred box at the violated bound
            fallback = 1;
            h = H; w = W;
            if ((W << 16) < (u64)a.r0 * H)
                h = ((W << 17) + a.r0) / (2ull * a.r0);
            else if ((W << 16) > (u64)a.r1 * H)
                w = (H * a.r1 + (1ull << 15)) >> 16;
            h = h < 1 ? 1 : (h > H ? H : h);
            w = w < 1 ? 1 : (w > W ? W : w);
            y0 = (H - h) / 2;
            x0 = (W - w) / 2;
        }
        flip = (unsigned int)(ingest_mix(h0 + G * 21ull) >> 40) <
               a.flip_thresh;
    } else {
        // centred, aspect OW:OH, eval_crop of the largest such box
        u64 bh, bw;                                              // Q16
        if (W * (u64)a.OH >= H * (u64)a.OW) {
            bh = H << 16; bw = ((H * (u64)a.OW) << 16) / (u64)a.OH;
        } else {
            bh = ((W * (u64)a.OH) << 16) / (u64)a.OW; bw = W << 16;
        }
        h = (bh * a.eval_crop + (1ull << 31)) >> 32;
        w = (bw * a.eval_crop + (1ull << 31)) >> 32;
        h = h < 1 ? 1 : (h > H ? H : h);
        w = w < 1 ? 1 : (w > W ? W : w);
        y0 = (H - h) / 2;
        x0 = (W - w) / 2;
    }
    int* row = a.boxes + (int64_t)n * 8;
    row[0] = (int)y0; row[1] = (int)x0; row[2] = (int)h; row[3] = (int)w;
    row[4] = flip;
    row[5] = (int)((h << 16) / (u64)a.OH);
    row[6] = (int)((w << 16) / (u64)a.OW);
    row[7] = fallback;
}

// Bilinear resample with half-pixel centres in fixed point.  Per axis,
//   p  = clamp((lo << 16) + o*step + (step >> 1) - 32768,
//              lo << 16, (lo + size - 1) << 16)
//   i  = p >> 16,  f = (p >> 8) & 255,  i1 = min(i + 1, lo + size - 1)
// and per channel the exact integer
//   acc = (256-fy)*((256-fx)*p00 + fx*p01) + fy*((256-fx)*p10 + fx*p11)
// (<= 255 * 65536 < 2^24, exact in fp32) becomes
//   bf16(fmaf((float)acc, scale_c * 2^-16, bias_c)).
// The fma is explicit: a separate multiply and add rounds differently for
// about a thousand accumulator values per channel, and the host path is
// compared bitwise.  Coordinates are int32: the launcher requires
// H, W <= 32767.
//
// Same shape as k_image_ingest: a thread makes INGEST_PIX consecutive
// output pixels of a row, packed 8-byte stores when aligned, grid-stride
// over 64-bit items.  The taps are small unaligned gathers from two source
// rows (served by L2); every index is clamped into the box, the box into
// the image, and a tail group's unused pixels are not read.

struct ResizedCropArgs {
    const uint8_t* __restrict__ src;  // [N, H, W, 3]
    uint16_t* __restrict__ out;       // [N, OH, OW, 3] bf16 payload
    const int* __restrict__ boxes;    // [N, 8] from k_resized_crop_draw
    int N, H, W, OH, OW;
    float scale[3], bias[3];          // scale already times 2^-16
};

__global__ void __launch_bounds__(256)
k_resized_crop(ResizedCropArgs a) {
    const int groups = (a.OW + INGEST_PIX - 1) / INGEST_PIX;  // per row
    const int64_t items = (int64_t)a.N * a.OH * groups;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         it < items; it += stride) {
        const int64_t row = it / groups;          // n * OH + oy
        const int ox0 = (int)(it - row * groups) * INGEST_PIX;
        const int n = (int)(row / a.OH);
        const int oy = (int)(row - (int64_t)n * a.OH);

        const int4 b0 = reinterpret_cast<const int4*>(a.boxes)[n * 2];
        const int4 b1 = reinterpret_cast<const int4*>(a.boxes)[n * 2 + 1];
        // the draw keeps every box inside the image; clamp all the same,
        // so no content of `boxes` can send a load out of the source
        const int y0 = min(max(b0.x, 0), a.H - 1);
        const int x0 = min(max(b0.y, 0), a.W - 1);
        const int ylast = y0 + min(max(b0.z, 1), a.H - y0) - 1;
        const int xlast = x0 + min(max(b0.w, 1), a.W - x0) - 1;
        const bool flip = b1.x != 0;
        // steps are taken as they come: the coordinate sums below wrap in
        // unsigned arithmetic and are clamped into the box afterwards
        const unsigned int step_y = (unsigned int)b1.y;
        const unsigned int step_x = (unsigned int)b1.z;

        int py = (int)(((unsigned int)y0 << 16) + (unsigned int)oy * step_y +
                       (step_y >> 1) - 32768u);
        py = min(max(py, y0 << 16), ylast << 16);
        const int iy = py >> 16;
        const int iy1 = min(iy + 1, ylast);
        const unsigned int fy = (unsigned int)(py >> 8) & 255u;
        const int64_t img = (int64_t)n * a.H;
        const uint8_t* r0 = a.src + (img + iy) * ((int64_t)a.W * 3);
        const uint8_t* r1 = a.src + (img + iy1) * ((int64_t)a.W * 3);
        const int cnt = a.OW - ox0 < INGEST_PIX ? a.OW - ox0 : INGEST_PIX;

        uint16_t v[INGEST_PIX * 3];
#pragma unroll
        for (int j = 0; j < INGEST_PIX; ++j) {
            if (j < cnt) {  // a tail group's unused pixels are not read
                const int ox = ox0 + j;
                const int oxs = flip ? a.OW - 1 - ox : ox;
                int px = (int)(((unsigned int)x0 << 16) +
                               (unsigned int)oxs * step_x + (step_x >> 1) -
                               32768u);
                px = min(max(px, x0 << 16), xlast << 16);
                const int ix = (px >> 16) * 3;
                const int ix1 = min((px >> 16) + 1, xlast) * 3;
                const unsigned int fx = (unsigned int)(px >> 8) & 255u;
                // the right tap is the next pixel except at the box's last
                // column: then both taps of a row are 6 contiguous bytes,
                // read as (unaligned) dword + short instead of 6 byte loads
                uint8_t t[6], b[6];
                if (ix1 != ix) {
                    __builtin_memcpy(t, r0 + ix, 6);
                    __builtin_memcpy(b, r1 + ix, 6);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        t[c] = t[3 + c] = r0[ix + c];
                        b[c] = b[3 + c] = r1[ix + c];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned int top =
                        (256u - fx) * t[c] + fx * t[3 + c];
                    const unsigned int bot =
                        (256u - fx) * b[c] + fx * b[3 + c];
                    const unsigned int acc = (256u - fy) * top + fy * bot;
                    v[j * 3 + c] = f32_to_bf16(
                        fmaf((float)acc, a.scale[c], a.bias[c]));
                }
            } else {
                v[j * 3] = v[j * 3 + 1] = v[j * 3 + 2] = 0;
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

// boxes: int32 [N, 8], 16-byte aligned.  tables: int32 [3, RC_TABLE].
// step_dev may be null in eval mode (train = 0).
extern "C" void launch_resized_crop_draw(void* boxes, const void* tables,
                                         const void* step_dev, int N, int H,
                                         int W, int OH, int OW, uint64_t seed,
                                         uint64_t root_hw,
                                         uint32_t flip_thresh, uint32_t r0,
                                         uint32_t r1, uint32_t eval_crop,
                                         int train, hipStream_t stream) {
    ResizedCropDrawArgs a{};
    a.boxes = (int*)boxes;
    a.tables = (const int*)tables;
    a.step_ptr = (const long long*)step_dev;
    a.N = N; a.H = H; a.W = W; a.OH = OH; a.OW = OW;
    a.seed = seed;
    a.root_hw = root_hw;
    a.flip_thresh = flip_thresh;
    a.r0 = r0; a.r1 = r1; a.eval_crop = eval_crop;
    a.train = train;
    k_resized_crop_draw<<<(N + 255) / 256, 256, 0, stream>>>(a);
}

extern "C" void launch_resized_crop(const void* src, void* out,
                                    const void* boxes, int N, int H, int W,
                                    int OH, int OW, const float* scale,
                                    const float* bias, hipStream_t stream) {
    ResizedCropArgs a{};
    a.src = (const uint8_t*)src;
    a.out = (uint16_t*)out;
    a.boxes = (const int*)boxes;
    a.N = N; a.H = H; a.W = W; a.OH = OH; a.OW = OW;
    for (int c = 0; c < 3; ++c) {
        a.scale[c] = scale[c] * (1.0f / 65536.0f);  // exact: a power of two
        a.bias[c] = bias[c];
    }
    const int groups = (OW + INGEST_PIX - 1) / INGEST_PIX;
    const int grid = ew_grid((int64_t)N * OH * groups, 256, 1);
    k_resized_crop<<<grid, 256, 0, stream>>>(a);
}

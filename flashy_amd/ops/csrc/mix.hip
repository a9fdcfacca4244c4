// Copyright (c) Flashy-AMD authors.
// Batch mixing for gfx950 (flashy_amd.data.DeviceMix): Mixup and CutMix of a
// bf16 NHWC batch in place, sample i with sample N-1-i (timm's x.flip(0)).
//
// Two launches per batch.  k_batch_mix_draw, one thread, writes the batch's
// mix row (mode, y0, y1, x0, x1, lam as fp32 bits, j, 0) as a pure function
// of (seed, *step_ptr), so a captured (HIP-graph) step mixes differently on
// every replay; the caller advances the counter afterwards with
// launch_adam_step_inc, as for the ingest kernels.  k_batch_mix reads the
// row from device memory and blends (mode 1) or swaps a box (mode 2); the
// loss kernel reads lam from slot 5 of the same row.
//
// The draw is timm's Mixup (batch mode, rand_bbox with the area correction)
// in integers: Beta(alpha, alpha) is quantized to the midpoints of 1024
// equal-probability bins that the host tabulates (lam in fp32 for mixup,
// sqrt(1 - lam) in Q16 for cutmix), so no pow / log / sqrt runs here and
// DeviceMix.row_at reproduces every row bit for bit.  The one floating-point
// operation is a double division, correctly rounded on both sides.
//
// k_batch_mix is memory-bound: 2 B read + 2 B written per mixed element.  A
// work item owns the same 8 elements of both samples of a pair, so the
// in-place blend or swap needs no second buffer and reads each element
// once.  Items are cut at 16-byte boundaries of sample i's range; where the
// partner's range is misaligned by the same amount (always when the range
// length is a multiple of 8) a full item is one 16-byte load and store per
// sample, and heads, tails and incongruent ranges go element by element.
// Grid-stride over <= 2048 blocks.

#include "common.h"

#define MIX_TABLE 1024

struct MixDrawArgs {
    int* __restrict__ row;                // [8]
    const float* __restrict__ lam_table;  // [MIX_TABLE] mixup lam
    const int* __restrict__ sq_table;     // [MIX_TABLE] Q16 sqrt(1 - lam)
    const long long* step_ptr;            // device step counter
    int H, W;
    unsigned long long seed;
    unsigned int prob_thresh;             // round(prob * 2^24)
    unsigned int switch_thresh;           // round(switch_prob * 2^24)
    int mixup, cutmix;                    // which modes are enabled
};

__global__ void __launch_bounds__(64)
k_batch_mix_draw(MixDrawArgs a) {
    typedef unsigned long long u64;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const u64 G = 0x9E3779B97F4A7C15ull;
    const u64 step = (u64)*a.step_ptr;
    const u64 key = ingest_mix(a.seed + G * (step + 1));
    // the batch-level slot: the augments hash key + G*(i+1) for sample i
    const u64 hm = ingest_mix(key);
    const u64 ha = ingest_mix(hm + G);
    const u64 hb = ingest_mix(hm + 2ull * G);
    const u64 hc = ingest_mix(hm + 3ull * G);
    const bool apply = (unsigned int)(ha >> 40) < a.prob_thresh;
    const bool cut = a.cutmix &&
        (!a.mixup || (unsigned int)(ha & 0xffffffull) < a.switch_thresh);
    const int j = (int)(((hb & 0xffffffffull) * MIX_TABLE) >> 32);
    int mode = 0, y0 = 0, y1 = 0, x0 = 0, x1 = 0;
    float lam = 1.0f;
    if (apply && !cut && a.mixup) {
        mode = 1;
        lam = a.lam_table[j];
    } else if (apply && cut) {
        mode = 2;
        const long long H = a.H, W = a.W;
        const long long sq = a.sq_table[j];
        const int cut_h = (int)((H * sq) >> 16);
        const int cut_w = (int)((W * sq) >> 16);
        const int cy = (int)(((hc & 0xffffffffull) * (u64)H) >> 32);
        const int cx = (int)(((hc >> 32) * (u64)W) >> 32);
        y0 = max(cy - cut_h / 2, 0);
        y1 = min(cy + cut_h / 2, a.H);
        x0 = max(cx - cut_w / 2, 0);
        x1 = min(cx + cut_w / 2, a.W);
        const long long area = (long long)(y1 - y0) * (x1 - x0);
        lam = (float)(1.0 - (double)area / (double)(H * W));
    }
    a.row[0] = mode;
    a.row[1] = y0; a.row[2] = y1; a.row[3] = x0; a.row[4] = x1;
    a.row[5] = __float_as_int(lam);
    a.row[6] = j;
    a.row[7] = 0;
}

// lam*a + oml*b with every operation rounded on its own: the torch mirror
// x.float()*lam + x.flip(0).float()*oml is compared bitwise, so the compiler
// must not contract a multiply and the add into an fma.  The pragma does
// that; __fmul_rn / __fadd_rn would not, since the HIP headers define them as
// the plain operators, which are contracted like any other (the ISA showed
// v_pk_fma_f32 with them, v_pk_mul_f32 + v_pk_add_f32 with the pragma).
__device__ __forceinline__ uint16_t mix_blend(float lam, float oml,
                                              uint16_t a, uint16_t b) {
#pragma clang fp contract(off)
    const float ta = lam * bf16_to_f32(a);
    const float tb = oml * bf16_to_f32(b);
    return f32_to_bf16(ta + tb);
}

struct MixArgs {
    uint16_t* x;                      // [N, H, W, C] bf16 payload, in place
    const int* __restrict__ row;      // [8] from k_batch_mix_draw (or a caller)
    int N, H, W, C;
};

// One item of a pair: elements [lo, hi) of the ranges starting at pa / pb
// (the same elements of both samples), hi - lo <= 8.  `vec`: the item is a
// full 8 elements and both addresses are 16-byte aligned.  `same`: pa and pb
// are the same range (the middle sample of an odd batch).
__device__ __forceinline__ void mix_item(uint16_t* pa, uint16_t* pb,
                                         int64_t lo, int64_t hi, bool vec,
                                         bool same, bool blend, float lam,
                                         float oml) {
    if (vec) {
        const short8 va = *reinterpret_cast<const short8*>(pa + lo);
        const short8 vb = *reinterpret_cast<const short8*>(pb + lo);
        short8 oa, ob;
        if (blend) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                oa[k] = (short)mix_blend(lam, oml, (uint16_t)va[k],
                                         (uint16_t)vb[k]);
                ob[k] = (short)mix_blend(lam, oml, (uint16_t)vb[k],
                                         (uint16_t)va[k]);
            }
        } else {
            oa = vb; ob = va;
        }
        *reinterpret_cast<short8*>(pa + lo) = oa;
        if (!same) *reinterpret_cast<short8*>(pb + lo) = ob;
    } else {
        for (int64_t e = lo; e < hi; ++e) {
            const uint16_t a = pa[e], b = pb[e];
            pa[e] = blend ? mix_blend(lam, oml, a, b) : b;
            if (!same) pb[e] = blend ? mix_blend(lam, oml, b, a) : a;
        }
    }
}

__global__ void __launch_bounds__(256)
k_batch_mix(MixArgs a) {
    const int4 r0 = reinterpret_cast<const int4*>(a.row)[0];
    const int4 r1 = reinterpret_cast<const int4*>(a.row)[1];
    const int mode = r0.x;
    if (mode != 1 && mode != 2) return;
    const int64_t E = (int64_t)a.H * a.W * a.C;     // elements per sample
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;

    if (mode == 1) {
        const float lam = __int_as_float(r1.y);
        const float oml = 1.0f - lam;
        const int64_t pairs = (a.N + 1) / 2;        // the middle with itself
        // items are cut at multiples of 8 elements of the whole tensor, so a
        // range that starts `off` elements past one has a head of 8 - off
        const int64_t per = (E + 7) / 8 + 1;
        for (int64_t it = tid; it < pairs * per; it += stride) {
            const int64_t p = it / per;
            const int64_t k = it - p * per;
            const int64_t q = a.N - 1 - p;
            const int offa = (int)((p * E) & 7), offb = (int)((q * E) & 7);
            int64_t lo = k * 8 - offa, hi = lo + 8;
            const bool full = lo >= 0 && hi <= E;
            lo = lo < 0 ? 0 : lo;
            hi = hi > E ? E : hi;
            if (lo >= hi) continue;
            mix_item(a.x + p * E, a.x + q * E, lo, hi, full && offa == offb,
                     p == q, true, lam, oml);
        }
        return;
    }

    // mode 2: whatever the row holds, the box is clamped into the image
    // before any access
    const int y0 = min(max(r0.y, 0), a.H);
    const int y1 = min(max(r0.z, y0), a.H);
    const int x0 = min(max(r0.w, 0), a.W);
    const int x1 = min(max(r1.x, x0), a.W);
    const int64_t pairs = a.N / 2;                  // the middle stays
    const int64_t bh = y1 - y0;
    const int64_t L = (int64_t)(x1 - x0) * a.C;     // elements per box row
    if (bh == 0 || L == 0) return;
    const int64_t per = (L + 7) / 8 + 1;
    const int64_t rowlen = (int64_t)a.W * a.C;
    for (int64_t it = tid; it < pairs * bh * per; it += stride) {
        const int64_t pr = it / per;                // pair * bh + box row
        const int64_t k = it - pr * per;
        const int64_t p = pr / bh;
        const int64_t y = y0 + (pr - p * bh);
        const int64_t q = a.N - 1 - p;
        const int64_t in = y * rowlen + (int64_t)x0 * a.C;
        const int offa = (int)((p * E + in) & 7);
        const int offb = (int)((q * E + in) & 7);
        int64_t lo = k * 8 - offa, hi = lo + 8;
        const bool full = lo >= 0 && hi <= L;
        lo = lo < 0 ? 0 : lo;
        hi = hi > L ? L : hi;
        if (lo >= hi) continue;
        mix_item(a.x + p * E + in, a.x + q * E + in, lo, hi,
                 full && offa == offb, false, false, 1.0f, 0.0f);
    }
}

// row: int32 [8], 16-byte aligned.  lam_table: fp32 [MIX_TABLE]; sq_table:
// int32 [MIX_TABLE]; the table of a disabled mode is not read.
extern "C" void launch_batch_mix_draw(void* row, const void* lam_table,
                                      const void* sq_table,
                                      const void* step_dev, int H, int W,
                                      uint64_t seed, uint32_t prob_thresh,
                                      uint32_t switch_thresh, int mixup,
                                      int cutmix, hipStream_t stream) {
    MixDrawArgs a{};
    a.row = (int*)row;
    a.lam_table = (const float*)lam_table;
    a.sq_table = (const int*)sq_table;
    a.step_ptr = (const long long*)step_dev;
    a.H = H; a.W = W;
    a.seed = seed;
    a.prob_thresh = prob_thresh;
    a.switch_thresh = switch_thresh;
    a.mixup = mixup; a.cutmix = cutmix;
    k_batch_mix_draw<<<1, 64, 0, stream>>>(a);
}

// x: bf16 [N, H, W, C], 16-byte aligned.  The grid is sized for the full
// image: the box is not known at launch (nor at capture).
extern "C" void launch_batch_mix(void* x, const void* row, int N, int H,
                                 int W, int C, hipStream_t stream) {
    MixArgs a{};
    a.x = (uint16_t*)x;
    a.row = (const int*)row;
    a.N = N; a.H = H; a.W = W; a.C = C;
    const int64_t E = (int64_t)H * W * C;
    const int grid = ew_grid((int64_t)((N + 1) / 2) * ((E + 7) / 8 + 1), 256, 1);
    k_batch_mix<<<grid, 256, 0, stream>>>(a);
}

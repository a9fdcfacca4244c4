// Copyright (c) Flashy-AMD authors.
// 8-wave 256-row implicit-GEMM conv FORWARD for gfx950 — the deep-pipeline
// schedule (CDNA4 guide §5 "256² 8-phase template" adapted to conv):
//
//   * 512 threads (8 waves, 2M x 4N), tile BM=256 x BN in {64,128}, BK=64;
//   * BOTH operands staged to LDS by async global->LDS DMA
//     (`raw_ptr_buffer_load_lds` 16 B/lane): no staging registers, no
//     ds_write pass, and the A (im2col) padding is handled by the buffer
//     descriptor's bounds check — out-of-range taps load hardware zeros
//     (voffset sentinel far past num_bytes), so the inner loop has ZERO
//     branches;
//   * 4 (BN=64) or 3 (BN=128) LDS buffers, ONE raw `s_barrier` per 64-deep
//     stage, counted `s_waitcnt vmcnt` so the next one or two stages' DMA
//     stays in flight across the barrier (never vmcnt(0) in the main loop);
//   * swizzled LDS images, swapped-operand MFMA clusters under
//     `s_setprio`, packed 8 B stores.
//
// Plans, launch dispatch and the OOB sentinel are shared through conv8.h.
//
// Used for the large-M ResNet-50/224-class layers (C%64==0, K%64==0,
// tensor < 2 GB); small-M / long-K shapes stay on the 4-wave split-K
// kernel in conv_fwd.hip.  GEMM view and layouts as in conv_fwd.hip.

#include "conv8.h"

template <int BN, bool RELU, bool SPLITK = false>
__global__ void __launch_bounds__(512, 2)
k_conv_fwd8(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
            uint16_t* __restrict__ y, float* __restrict__ bn_ws,
            ConvDims d, unsigned x_nbytes, int spz = 0) {
    constexpr int BM = 256;
    constexpr int BK = 64;
    constexpr int NF = BN / 64;          // n fragments per wave (4 N-waves)
    constexpr int MF = 8;                // m fragments per wave (2 M-waves)
    constexpr int A_ELEMS = BM * BK;     // 16384 bf16 = 32 KiB
    constexpr int B_ELEMS = BN * BK;     // 4096/8192 bf16 = 8/16 KiB
    constexpr int BUF_ELEMS = A_ELEMS + B_ELEMS;
    constexpr int G = 4 + BN / 64;       // glds per wave per stage (A + B)
    // BN=64 buffers fit 4x in the 160 KiB LDS -> prefetch DEPTH 2 (two
    // stages' DMA in flight across barriers); BN=128 fits 3 -> depth 1
    constexpr int BUFS = BN == 64 ? 4 : 3;
    constexpr int DEPTH = BUFS - 2;

    const int rsc = d.R * d.S * d.C;
    const int64_t M = (int64_t)d.N * d.Ho * d.Wo;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wid_u >> 2;       // 0..1
    const int wave_n = wid_u & 3;        // 0..3

    unsigned bx = blockIdx.x;
    if ((gridDim.x & 7) == 0)            // XCD-aware m-tile order (T1)
        bx = (bx & 7) * (gridDim.x >> 3) + (bx >> 3);
    const int64_t m0 = (int64_t)bx * BM;
    const int col0 = blockIdx.y * BN;

    __shared__ uint16_t lds[BUFS * BUF_ELEMS];

    const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)x, 0 /*stride*/, x_nbytes, 0x00020000 /*flags*/);

    // --- A staging state: 4 dest chunks per thread, geometry fixed, tap
    // (r,s,c) walks +BK per stage with carries (no divides steady-state).
    int a_r[4], a_s[4], a_c[4], a_hi0[4], a_wi0[4];
    int64_t a_n[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int chunk = g * 512 + tid;          // dest chunk 0..2047
        const int row = chunk >> 3;
        const int kc_s = (chunk & 7) ^ (row & 7); // source k-chunk (swizzle)
        const int64_t m = m0 + row;
        if (m < M) {
            const int hw = d.Ho * d.Wo;
            a_n[g] = m / hw;
            const int rem = (int)(m % hw);
            a_hi0[g] = (rem / d.Wo) * d.stride - d.pad;
            a_wi0[g] = (rem % d.Wo) * d.stride - d.pad;
        } else {
            a_n[g] = -1;
        }
        const int kk = (SPLITK ? blockIdx.z * spz * 64 : 0) + kc_s * 8;
        a_r[g] = kk / (d.S * d.C);
        const int sc = kk - a_r[g] * d.S * d.C;
        a_s[g] = sc / d.C;
        a_c[g] = sc - a_s[g] * d.C;
    }
    // B staging: source byte offset advances by BK*2 per stage.
    unsigned b_src[2];
#pragma unroll
    for (int g = 0; g < NF; ++g) {
        const int chunk = g * 512 + tid;          // dest chunk 0..BN*8-1
        const int col = chunk >> 3;
        const int kc_s = (chunk & 7) ^ (col & 7);
        b_src[g] = (unsigned)(((int64_t)(col0 + col) * rsc +
                              (SPLITK ? blockIdx.z * spz * 64 : 0) +
                              kc_s * 8) * 2);
    }

    auto issue_stage = [&](int stage, int buf) {
        uint16_t* base = lds + buf * BUF_ELEMS;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned voff = kOobSentinel;
            if (a_n[g] >= 0 && a_r[g] < d.R) {
                const int hi = a_hi0[g] + a_r[g];
                const int wi = a_wi0[g] + a_s[g];
                if (hi >= 0 && hi < d.H && wi >= 0 && wi < d.W)
                    voff = (unsigned)((((a_n[g] * d.H + hi) * d.W + wi) *
                                       (int64_t)d.C + a_c[g]) * 2);
            }
            // advance tap by one stage (+BK) with carries
            int c = a_c[g] + BK;
            while (c >= d.C) {
                c -= d.C;
                if (++a_s[g] == d.S) { a_s[g] = 0; ++a_r[g]; }
            }
            a_c[g] = c;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                xrsrc,
                (__attribute__((address_space(3))) void*)
                    (base + (g * 512 + wid_u * 64) * 8),
                16, voff, 0, 0, 0);
        }
        uint16_t* bbase = base + A_ELEMS;
        const unsigned kb = (unsigned)(stage * BK * 2);
#pragma unroll
        for (int g = 0; g < NF; ++g) {
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned int*)
                    ((const char*)w + b_src[g] + kb),
                (__attribute__((address_space(3))) unsigned int*)
                    (bbase + (g * 512 + wid_u * 64) * 8),
                16, 0, 0);
        }
    };

    // fragment LDS byte offsets (swizzled), fixed per lane
    const int a_row_l = wave_m * 128 + (lane & 15);   // + mf*16
    const int frag_kb = (lane >> 4) * 16;             // byte within 64B half
    const int b_col_l = wave_n * (BN / 4) + (lane & 15);  // + nf*16

    floatx4 acc[MF][NF] = {};
    int n_stages = rsc / BK;
    if (SPLITK) {
        const int remain = n_stages - blockIdx.z * spz;
        n_stages = remain < spz ? remain : spz;
        if (n_stages <= 0) return;
    }

    auto compute_stage = [&](int buf) {
        const uint16_t* base = lds + buf * BUF_ELEMS;
        const uint16_t* bbase = base + A_ELEMS;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            short8 a[MF], b[NF];
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int row = a_row_l + mf * 16;
                const int byte = (row * 128 + sub * 64 + frag_kb) ^
                                 ((row & 7) << 4);
                a[mf] = *reinterpret_cast<const short8*>(
                    (const char*)base + byte);
            }
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const int col = b_col_l + nf * 16;
                const int byte = (col * 128 + sub * 64 + frag_kb) ^
                                 ((col & 7) << 4);
                b[nf] = *reinterpret_cast<const short8*>(
                    (const char*)bbase + byte);
            }
            __builtin_amdgcn_s_setprio(1);
            // operands SWAPPED (weights first): the D-fragment then holds
            // 4 CONSECUTIVE output channels per lane ((l>>4)*4+rr) at one
            // pixel (l&15) — the epilogue packs them into one 8 B store
            // instead of four scalar 2 B stores (the big-K 1x1 layers are
            // store-issue-bound).  A- and B-fragment lane maps are
            // transposes of each other, so the same LDS reads serve both.
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
#pragma unroll
                for (int nf = 0; nf < NF; ++nf)
                    acc[mf][nf] = MFMA_BF16(b[nf], a[mf], acc[mf][nf]);
            __builtin_amdgcn_s_setprio(0);
        }
        // no tail barrier: wave skew is bounded by the next iteration's
        // barrier, and the in-flight writes always target b[(i+2)%3] while
        // laggards read b[i%3] — never the same buffer.
    };

    for (int p = 0; p < DEPTH && p < n_stages; ++p)
        issue_stage(p, p % BUFS);
    for (int i = 0; i + DEPTH < n_stages; ++i) {
        issue_stage(i + DEPTH, (i + DEPTH) % BUFS);
        // stage i landed; own DEPTH*G loads stay in flight across the
        // barrier (counted wait — never vmcnt(0) in the hot loop)
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(DEPTH * G) : "memory");
        __builtin_amdgcn_s_barrier();
        compute_stage(i % BUFS);
    }
    if (DEPTH == 2 && n_stages >= 2) {   // tail with one stage in flight
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(G) : "memory");
        __builtin_amdgcn_s_barrier();
        compute_stage((n_stages - 2) % BUFS);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    compute_stage((n_stages - 1) % BUFS);

    // --- epilogue ---------------------------------------------------------
    // Swapped-operand D layout: lane l of acc[mf][nf] holds pixel row
    // (mf*16 + (l&15)) at output channels (nf*16 + (l>>4)*4 + rr) — four
    // CONSECUTIVE channels per lane, packed into one 8 B store.
    const int64_t out_row0 = m0 + wave_m * 128 + (lane & 15);
    const int out_col0 = col0 + wave_n * (BN / 4) + (lane >> 4) * 4;
    if (SPLITK) {   // fp32 partials slab [z][M][K], float4 per lane
        float* ws = reinterpret_cast<float*>(bn_ws);   // reused arg
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const int64_t row = out_row0 + mf * 16;
            if (row < M) {
#pragma unroll
                for (int nf = 0; nf < NF; ++nf)
                    *reinterpret_cast<float4*>(
                        ws + ((int64_t)blockIdx.z * M + row) * d.K +
                        out_col0 + nf * 16) =
                        make_float4(acc[mf][nf][0], acc[mf][nf][1],
                                    acc[mf][nf][2], acc[mf][nf][3]);
            }
        }
        return;
    }
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const int64_t row = out_row0 + mf * 16;
        if (row < M) {
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                ushort4 pk;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    float v = acc[mf][nf][rr];
                    if (RELU) v = fmaxf(v, 0.f);
                    ((uint16_t*)&pk)[rr] = f32_to_bf16(v);
                }
                *reinterpret_cast<ushort4*>(
                    y + row * d.K + out_col0 + nf * 16) = pk;
            }
        }
    }

    if (bn_ws != nullptr) {
        __syncthreads();                 // main loop fully done: reuse lds
        float* sred = reinterpret_cast<float*>(lds);   // [2*WM][BN]
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
            float s[4] = {}, s2[4] = {};
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int64_t row = out_row0 + mf * 16;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    float v = acc[mf][nf][rr];
                    if (RELU) v = fmaxf(v, 0.f);
                    if (row >= M) v = 0.f;
                    s[rr] += v;
                    s2[rr] = fmaf(v, v, s2[rr]);
                }
            }
            // reduce over the 16 pixel lanes (low 4 lane bits)
#pragma unroll
            for (int off = 1; off < 16; off <<= 1)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    s[rr] += __shfl_xor(s[rr], off, 64);
                    s2[rr] += __shfl_xor(s2[rr], off, 64);
                }
            if ((lane & 15) == 0) {
                const int colL = wave_n * (BN / 4) + nf * 16 + (lane >> 4) * 4;
                *reinterpret_cast<float4*>(&sred[wave_m * BN + colL]) =
                    make_float4(s[0], s[1], s[2], s[3]);
                *reinterpret_cast<float4*>(&sred[(2 + wave_m) * BN + colL]) =
                    make_float4(s2[0], s2[1], s2[2], s2[3]);
            }
        }
        __syncthreads();
        if (tid < BN) {
            const float s = sred[tid] + sred[BN + tid];
            const float s2 = sred[2 * BN + tid] + sred[3 * BN + tid];
            const int c = col0 + tid;
            bn_ws[(int64_t)c * gridDim.x + blockIdx.x] = s;
            bn_ws[((int64_t)d.K + c) * gridDim.x + blockIdx.x] = s2;
        }
    }
}

// --- persistent-B m-loop 1x1 kernel ----------------------------------------
// For single-stage 1x1 convs (C == 64, stride 1): the generic kernel's
// whole life is ONE stage, so every block pays a full un-pipelined
// HBM->LDS->MFMA round trip (r1_1x1b measured 116 TF).  Here each block
// keeps the weight tile resident in LDS and loops over MANY 256-row
// m-tiles, pipelining the A DMA two tiles ahead — the round-trip latency
// amortizes across the whole m walk.  BN-stats partials are written
// per-(tile, wave_m) slice (msplit = 2 * mtiles), so the epilogue needs no
// LDS and no barrier that would drain the in-flight DMA.

template <int BN, bool RELU>
__global__ void __launch_bounds__(512, 2)
k_conv1x1_mloop(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
                uint16_t* __restrict__ y, float* __restrict__ bn_ws,
                ConvDims d, unsigned x_nbytes, int mtiles) {
    constexpr int BK = 64;               // = C
    constexpr int NF = BN / 64;
    constexpr int MF = 8;
    constexpr int A_ELEMS = 256 * BK;
    constexpr int B_ELEMS = BN * BK;

    const int64_t M = (int64_t)d.N * d.Ho * d.Wo;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wid_u >> 2;
    const int wave_n = wid_u & 3;

    unsigned bx = blockIdx.x;
    if ((gridDim.x & 7) == 0)
        bx = (bx & 7) * (gridDim.x >> 3) + (bx >> 3);
    const int col0 = blockIdx.y * BN;
    const int gT = gridDim.x;

    __shared__ uint16_t lds[3 * A_ELEMS + B_ELEMS];
    uint16_t* const bbase = lds + 3 * A_ELEMS;

    const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)x, 0, x_nbytes, 0x00020000);

    // B once: dest chunk t -> source chunk (col, kc ^ (col&7))
#pragma unroll
    for (int g = 0; g < NF; ++g) {
        const int chunk = g * 512 + tid;
        const int col = chunk >> 3;
        const int kc_s = (chunk & 7) ^ (col & 7);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)
                (w + (int64_t)(col0 + col) * BK + kc_s * 8),
            (__attribute__((address_space(3))) unsigned int*)
                (bbase + (g * 512 + wid_u * 64) * 8),
            16, 0, 0);
    }

    // per-thread A chunk geometry (fixed): row + swizzled k-chunk
    int a_row[4], a_koff[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int chunk = g * 512 + tid;
        const int row = chunk >> 3;
        a_row[g] = row;
        a_koff[g] = ((chunk & 7) ^ (row & 7)) * 8;
    }
    auto issue_a = [&](int64_t tile, int slot) {
        uint16_t* base = lds + slot * A_ELEMS;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t m = tile * 256 + a_row[g];
            const unsigned voff = m < M
                ? (unsigned)((m * BK + a_koff[g]) * 2) : kOobSentinel;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                xrsrc,
                (__attribute__((address_space(3))) void*)
                    (base + (g * 512 + wid_u * 64) * 8),
                16, voff, 0, 0, 0);
        }
    };

    const int a_row_l = wave_m * 128 + (lane & 15);
    const int frag_kb = (lane >> 4) * 16;
    const int b_col_l = wave_n * (BN / 4) + (lane & 15);

    short8 bfrag[2][NF];
    const int64_t ntl = (mtiles - (int64_t)bx + gT - 1) / gT;  // my tiles
    if (ntl <= 0) return;
    issue_a(bx, 0);
    if (ntl > 1) issue_a(bx + gT, 1);

    for (int64_t k = 0; k < ntl; ++k) {
        const int64_t tile = bx + k * gT;
        if (k + 2 < ntl) {
            issue_a(tile + 2 * gT, (int)((k + 2) % 3));
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else if (k + 1 < ntl) {
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        if (k == 0) {   // weights landed (oldest DMA): load the B fragments
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    const int col = b_col_l + nf * 16;
                    const int byte = (col * 128 + sub * 64 + frag_kb) ^
                                     ((col & 7) << 4);
                    bfrag[sub][nf] = *reinterpret_cast<const short8*>(
                        (const char*)bbase + byte);
                }
        }
        const uint16_t* base = lds + (k % 3) * A_ELEMS;
        floatx4 acc[MF][NF] = {};
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            short8 a[MF];
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int row = a_row_l + mf * 16;
                const int byte = (row * 128 + sub * 64 + frag_kb) ^
                                 ((row & 7) << 4);
                a[mf] = *reinterpret_cast<const short8*>(
                    (const char*)base + byte);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
#pragma unroll
                for (int nf = 0; nf < NF; ++nf)
                    acc[mf][nf] =
                        MFMA_BF16(bfrag[sub][nf], a[mf], acc[mf][nf]);
            __builtin_amdgcn_s_setprio(0);
        }
        // epilogue for this tile (packed 8 B stores, swapped layout)
        const int64_t out_row0 = tile * 256 + wave_m * 128 + (lane & 15);
        const int out_col0 = col0 + wave_n * (BN / 4) + (lane >> 4) * 4;
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const int64_t row = out_row0 + mf * 16;
            if (row < M) {
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    ushort4 pk;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        float v = acc[mf][nf][rr];
                        if (RELU) v = fmaxf(v, 0.f);
                        ((uint16_t*)&pk)[rr] = f32_to_bf16(v);
                    }
                    *reinterpret_cast<ushort4*>(
                        y + row * d.K + out_col0 + nf * 16) = pk;
                }
            }
        }
        if (bn_ws != nullptr) {   // per-(tile, wave_m) slice: LDS-free
            const int64_t msplit = 2 * (int64_t)mtiles;
            const int64_t slice = tile * 2 + wave_m;
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                float s[4] = {}, s2[4] = {};
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) {
                    const int64_t row = out_row0 + mf * 16;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        float v = acc[mf][nf][rr];
                        if (RELU) v = fmaxf(v, 0.f);
                        if (row >= M) v = 0.f;
                        s[rr] += v;
                        s2[rr] = fmaf(v, v, s2[rr]);
                    }
                }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        s[rr] += __shfl_xor(s[rr], off, 64);
                        s2[rr] += __shfl_xor(s2[rr], off, 64);
                    }
                if ((lane & 15) == 0) {
                    const int c = col0 + wave_n * (BN / 4) + nf * 16 +
                                  (lane >> 4) * 4;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        bn_ws[(int64_t)(c + rr) * msplit + slice] = s[rr];
                        bn_ws[((int64_t)d.K + c + rr) * msplit + slice] =
                            s2[rr];
                    }
                }
            }
        }
    }
}

extern "C" int conv1x1_mloop_plan(ConvDims d, int* bn_out, int* gridx_out) {
    if (conv8_disabled()) return 0;
    if (d.R != 1 || d.S != 1 || d.stride != 1 || d.pad != 0) return 0;
    if (d.C != 64 || d.K % 64) return 0;
    const int64_t M = (int64_t)d.N * d.Ho * d.Wo;
    const int64_t x_elems = (int64_t)d.N * d.H * d.W * d.C;
    if (x_elems * 2 >= (int64_t)kOobSentinel) return 0;
    const int mtiles = (int)((M + 255) / 256);
    if (mtiles < 128) return 0;
    const int bn = d.K % 128 == 0 ? 128 : 64;
    *bn_out = bn;
    int gx = 256 / (d.K / bn);
    if (gx < 8) gx = 8;
    if (gx > mtiles) gx = mtiles;
    *gridx_out = gx;
    return mtiles;
}

extern "C" void launch_conv1x1_mloop(const void* x, const void* w, void* y,
                                     ConvDims d, int relu, void* bn_ws,
                                     int bn, int gridx, int mtiles,
                                     hipStream_t stream) {
    dim3 grid((unsigned)gridx, (unsigned)(d.K / bn));
    const unsigned xb = (unsigned)((int64_t)d.N * d.H * d.W * d.C * 2);
    dispatch8(bn, relu, [&](auto BN, auto RELU) {
        k_conv1x1_mloop<decltype(BN)::value, decltype(RELU)::value>
            <<<grid, 512, 0, stream>>>((const uint16_t*)x, (const uint16_t*)w,
                                       (uint16_t*)y, (float*)bn_ws, d, xb,
                                       mtiles);
    });
}

// --- stem padding helpers ---------------------------------------------------
// The C=3 7x7 stem is run through the 8-wave kernel by padding to C'=4,
// R'=S'=8 (taps beyond 7x7 carry zero weights; borders are zero pixels), so
// every 16 B glds chunk is two contiguous (w, w+1) pixels and rsc' = 256.
// Useful/total MFMA work = 147/256, vs the direct stem kernel's 47 TF/s.

__global__ void __launch_bounds__(256)
k_stem_pad_x(const uint16_t* __restrict__ x, uint16_t* __restrict__ xp,
             int64_t N, int H, int W, int Hp, int Wp, int pad) {
    const int64_t total = N * Hp * Wp;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += stride) {
        const int wp_ = (int)(i % Wp);
        const int hp_ = (int)((i / Wp) % Hp);
        const int64_t n = i / ((int64_t)Hp * Wp);
        const int h = hp_ - pad, w = wp_ - pad;
        ushort4 v = {};
        if (h >= 0 && h < H && w >= 0 && w < W) {
            const uint16_t* src = x + ((n * H + h) * (int64_t)W + w) * 3;
            v.x = src[0];
            v.y = src[1];
            v.z = src[2];
        }
        *reinterpret_cast<ushort4*>(xp + i * 4) = v;
    }
}

__global__ void __launch_bounds__(256)
k_stem_pad_w(const uint16_t* __restrict__ w, uint16_t* __restrict__ wp,
             int K, int R, int S) {
    // wp[k][8][8][4] from w[k][R][S][3]
    const int total = K * 64;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gridDim.x * blockDim.x) {
        const int s = i % 8, r = (i / 8) % 8, k = i / 64;
        ushort4 v = {};
        if (r < R && s < S) {
            const uint16_t* src = w + ((k * R + r) * S + s) * 3;
            v.x = src[0];
            v.y = src[1];
            v.z = src[2];
        }
        *reinterpret_cast<ushort4*>(wp + i * 4) = v;
    }
}

__global__ void __launch_bounds__(256)
k_stem_unpad_dw(const float* __restrict__ dwp, float* __restrict__ dw,
                int K, int R, int S) {
    // dw[k][R][S][3] += dwp[k][8][8][4]
    const int total = K * R * S * 3;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gridDim.x * blockDim.x) {
        const int c = i % 3, s = (i / 3) % S, r = (i / (3 * S)) % R,
                  k = i / (3 * S * R);
        dw[i] += dwp[((k * 8 + r) * 8 + s) * 4 + c];
    }
}

extern "C" void launch_stem_pad_x(const void* x, void* xp, int64_t N, int H,
                                  int W, int Hp, int Wp, int pad,
                                  hipStream_t stream) {
    k_stem_pad_x<<<ew_grid(N * Hp * Wp, 256, 2), 256, 0, stream>>>(
        (const uint16_t*)x, (uint16_t*)xp, N, H, W, Hp, Wp, pad);
}

extern "C" void launch_stem_pad_w(const void* w, void* wp, int K, int R,
                                  int S, hipStream_t stream) {
    k_stem_pad_w<<<(K * 64 + 255) / 256, 256, 0, stream>>>(
        (const uint16_t*)w, (uint16_t*)wp, K, R, S);
}

extern "C" void launch_stem_unpad_dw(const void* dwp, void* dw, int K, int R,
                                     int S, hipStream_t stream) {
    k_stem_unpad_dw<<<(K * R * S * 3 + 255) / 256, 256, 0, stream>>>(
        (const float*)dwp, (float*)dw, K, R, S);
}

// --- fwd8 plan + launchers ----------------------------------------------------
extern "C" int conv_fwd8_plan(ConvDims d, int* bn_out) {
    if (conv8_disabled()) return 0;
    const int64_t M = (int64_t)d.N * d.Ho * d.Wo;
    const int rsc = d.R * d.S * d.C;
    if (d.C % 64 || d.K % 64 || rsc % 64) return 0;
    const int64_t x_elems = (int64_t)d.N * d.H * d.W * d.C;
    if (x_elems * 2 >= (int64_t)kOobSentinel) return 0;   // 32-bit voffset
    const int mtiles = (int)((M + 255) / 256);
    return pick_bn8(mtiles, d.K, 160, bn_out) ? mtiles : 0;
}

extern "C" void launch_conv_fwd8(const void* x, const void* w, void* y,
                                 ConvDims d, int relu, void* bn_ws, int bn,
                                 int mtiles, hipStream_t stream) {
    dim3 grid((unsigned)mtiles, (unsigned)(d.K / bn));
    const unsigned xb = (unsigned)((int64_t)d.N * d.H * d.W * d.C * 2);
    dispatch8(bn, relu, [&](auto BN, auto RELU) {
        k_conv_fwd8<decltype(BN)::value, decltype(RELU)::value>
            <<<grid, 512, 0, stream>>>((const uint16_t*)x, (const uint16_t*)w,
                                       (uint16_t*)y, (float*)bn_ws, d, xb);
    });
}

extern "C" void launch_conv_fwd8_splitk(const void* x, const void* w,
                                        void* ws, ConvDims d, int bn,
                                        int mtiles, int spz, int zeff,
                                        hipStream_t stream) {
    dim3 grid((unsigned)mtiles, (unsigned)(d.K / bn), (unsigned)zeff);
    const unsigned xb = (unsigned)((int64_t)d.N * d.H * d.W * d.C * 2);
    auto xx = (const uint16_t*)x;
    auto ww = (const uint16_t*)w;
    if (bn == 128)
        k_conv_fwd8<128, false, true><<<grid, 512, 0, stream>>>(
            xx, ww, nullptr, (float*)ws, d, xb, spz);
    else
        k_conv_fwd8<64, false, true><<<grid, 512, 0, stream>>>(
            xx, ww, nullptr, (float*)ws, d, xb, spz);
}

// Copyright (c) Flashy-AMD authors.
// Fused flat-buffer optimizers for gfx950.
//
// The framework's FusedSGD/FusedAdam optimizers keep ALL parameters (and
// their gradients / momenta) as views into single contiguous fp32 buffers
// (flashy_amd/optim.py), so one kernel launch updates the whole model:
// perfectly coalesced float4 traffic, grid-stride over <=2048 blocks — the
// memory-bound roofline shape for HBM3E (guidelines G11/G13 of the CDNA4
// guide).  Replaces the per-parameter optimizer loops the reference inherits
// from torch (reference hot-op inventory: SURVEY.md §2.10 SGD/Adam rows).

#include "common.h"

#include <math.h>

// ---------------------------------------------------------------------------
// Per-device "hyper" block: the step's effective learning rate and gradient
// clip coefficient live in device memory, written by k_optim_prepare every
// step and read by the update kernels.  A captured (HIP-graph) step therefore
// follows an LR schedule and clips by global norm with no re-capture and no
// host sync — the same idea as Adam's on-device step counter.
// ---------------------------------------------------------------------------

enum { HYPER_LR = 0, HYPER_COEF = 1, HYPER_NORM = 2, HYPER_SIZE = 4 };

// ---------------------------------------------------------------------------
// SGD (torch.optim.SGD semantics):
//   d = g + wd * p
//   if momentum: m = mu * m + d ; d = nesterov ? d + mu * m : m
//   p -= lr * d
// ---------------------------------------------------------------------------

struct SgdArgs {
    float* __restrict__ p;
    const float* __restrict__ g;
    float* __restrict__ m;          // momentum buffer (null = no momentum)
    uint16_t* __restrict__ p_bf16;  // optional bf16 mirror of p (may be null)
    int64_t n;
    float lr, momentum, wd, grad_scale;
    int nesterov;
    const float* hyper;  // device lr / clip coef (null = use lr by value)
};

__device__ __forceinline__ float sgd_one(const SgdArgs& a, float p, float g,
                                         float& m) {
    g = g * a.grad_scale + a.wd * p;
    if (a.momentum != 0.f) {
        m = m * a.momentum + g;
        g = a.nesterov ? g + a.momentum * m : m;
    }
    return p - a.lr * g;
}

template <bool HAS_M, bool HAS_BF16>
__global__ void __launch_bounds__(256)
k_fused_sgd(SgdArgs a) {
    if (a.hyper != nullptr) {
        a.lr = a.hyper[HYPER_LR];
        a.grad_scale *= a.hyper[HYPER_COEF];
    }
    const int64_t n4 = a.n / 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float4* p4 = reinterpret_cast<float4*>(a.p);
    const float4* g4 = reinterpret_cast<const float4*>(a.g);
    float4* m4 = reinterpret_cast<float4*>(a.m);
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 p = p4[i];
        float4 g = g4[i];
        float4 m = HAS_M ? m4[i] : float4{0, 0, 0, 0};
        p.x = sgd_one(a, p.x, g.x, m.x);
        p.y = sgd_one(a, p.y, g.y, m.y);
        p.z = sgd_one(a, p.z, g.z, m.z);
        p.w = sgd_one(a, p.w, g.w, m.w);
        p4[i] = p;
        if (HAS_M) m4[i] = m;
        if (HAS_BF16) {
            ushort4 b;
            b.x = f32_to_bf16(p.x); b.y = f32_to_bf16(p.y);
            b.z = f32_to_bf16(p.z); b.w = f32_to_bf16(p.w);
            reinterpret_cast<ushort4*>(a.p_bf16)[i] = b;
        }
    }
    // scalar tail
    for (int64_t i = n4 * 4 + blockIdx.x * blockDim.x + threadIdx.x; i < a.n;
         i += stride) {
        float m = HAS_M ? a.m[i] : 0.f;
        float p = sgd_one(a, a.p[i], a.g[i], m);
        a.p[i] = p;
        if (HAS_M) a.m[i] = m;
        if (HAS_BF16) a.p_bf16[i] = f32_to_bf16(p);
    }
}

extern "C" void launch_fused_sgd(void* p, const void* g, void* m, void* p_bf16,
                                 int64_t n, float lr, float momentum, float wd,
                                 float grad_scale, int nesterov,
                                 const void* hyper, hipStream_t stream) {
    SgdArgs a{(float*)p, (const float*)g, (float*)m, (uint16_t*)p_bf16,
              n, lr, momentum, wd, grad_scale, nesterov, (const float*)hyper};
    int grid = ew_grid(n / 4 + 1, 256, 1);
    if (m != nullptr && p_bf16 != nullptr)
        k_fused_sgd<true, true><<<grid, 256, 0, stream>>>(a);
    else if (m != nullptr)
        k_fused_sgd<true, false><<<grid, 256, 0, stream>>>(a);
    else if (p_bf16 != nullptr)
        k_fused_sgd<false, true><<<grid, 256, 0, stream>>>(a);
    else
        k_fused_sgd<false, false><<<grid, 256, 0, stream>>>(a);
}

// ---------------------------------------------------------------------------
// Adam / AdamW (torch.optim semantics with bias correction):
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2
//   p -= lr * (m/bc1) / (sqrt(v/bc2) + eps)   [+ decoupled or L2 wd]
// ---------------------------------------------------------------------------

struct AdamArgs {
    float* __restrict__ p;
    const float* __restrict__ g;
    float* __restrict__ m;
    float* __restrict__ v;
    uint16_t* __restrict__ p_bf16;
    const long long* step_ptr;  // device step (graph-safe); null -> use bc1/bc2
    const float* hyper;         // device lr / clip coef (null = use lr by value)
    int64_t n;
    float lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale;
    int adamw;  // 1: decoupled weight decay, 0: L2 into grad
};

__device__ __forceinline__ float adam_one(const AdamArgs& a, float p, float g,
                                          float& m, float& v) {
    g *= a.grad_scale;
    if (!a.adamw) g += a.wd * p;
    else p *= (1.f - a.lr * a.wd);
    m = a.beta1 * m + (1.f - a.beta1) * g;
    v = a.beta2 * v + (1.f - a.beta2) * g * g;
    return p - a.lr * (m / a.bc1) / (sqrtf(v / a.bc2) + a.eps);
}

template <bool HAS_BF16>
__global__ void __launch_bounds__(256)
k_fused_adam(AdamArgs a) {
    if (a.step_ptr != nullptr) {
        const float t = (float)*a.step_ptr;
        a.bc1 = 1.f - powf(a.beta1, t);
        a.bc2 = 1.f - powf(a.beta2, t);
    }
    if (a.hyper != nullptr) {
        a.lr = a.hyper[HYPER_LR];
        a.grad_scale *= a.hyper[HYPER_COEF];
    }
    const int64_t n4 = a.n / 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float4* p4 = reinterpret_cast<float4*>(a.p);
    const float4* g4 = reinterpret_cast<const float4*>(a.g);
    float4* m4 = reinterpret_cast<float4*>(a.m);
    float4* v4 = reinterpret_cast<float4*>(a.v);
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 p = p4[i];
        float4 g = g4[i];
        float4 m = m4[i];
        float4 v = v4[i];
        p.x = adam_one(a, p.x, g.x, m.x, v.x);
        p.y = adam_one(a, p.y, g.y, m.y, v.y);
        p.z = adam_one(a, p.z, g.z, m.z, v.z);
        p.w = adam_one(a, p.w, g.w, m.w, v.w);
        p4[i] = p;
        m4[i] = m;
        v4[i] = v;
        if (HAS_BF16) {
            ushort4 b;
            b.x = f32_to_bf16(p.x); b.y = f32_to_bf16(p.y);
            b.z = f32_to_bf16(p.z); b.w = f32_to_bf16(p.w);
            reinterpret_cast<ushort4*>(a.p_bf16)[i] = b;
        }
    }
    for (int64_t i = n4 * 4 + blockIdx.x * blockDim.x + threadIdx.x; i < a.n;
         i += stride) {
        float m = a.m[i], v = a.v[i];
        float p = adam_one(a, a.p[i], a.g[i], m, v);
        a.p[i] = p;
        a.m[i] = m;
        a.v[i] = v;
        if (HAS_BF16) a.p_bf16[i] = f32_to_bf16(p);
    }
}

__global__ void k_step_inc(long long* p) {
    if (threadIdx.x == 0 && blockIdx.x == 0) ++(*p);
}

extern "C" void launch_adam_step_inc(void* p, hipStream_t stream) {
    k_step_inc<<<1, 1, 0, stream>>>((long long*)p);
}

extern "C" void launch_fused_adam(void* p, const void* g, void* m, void* v,
                                  void* p_bf16, void* step_dev, int64_t n,
                                  float lr, float beta1, float beta2, float eps,
                                  float wd, int64_t step, float grad_scale,
                                  int adamw, const void* hyper,
                                  hipStream_t stream) {
    AdamArgs a{(float*)p, (const float*)g, (float*)m, (float*)v,
               (uint16_t*)p_bf16, (const long long*)step_dev,
               (const float*)hyper, n, lr, beta1,
               beta2, eps, wd,
               1.f - powf(beta1, (float)step), 1.f - powf(beta2, (float)step),
               grad_scale, adamw};
    int grid = ew_grid(n / 4 + 1, 256, 1);
    if (p_bf16 != nullptr)
        k_fused_adam<true><<<grid, 256, 0, stream>>>(a);
    else
        k_fused_adam<false><<<grid, 256, 0, stream>>>(a);
}

// ---------------------------------------------------------------------------
// Global gradient norm, pass 1: sum of squares of a flat fp32 buffer into one
// partial per block.  Same float4 grid-stride shape and scalar tail as the
// update kernels; no atomics and no pre-zeroing, so the result is
// deterministic for a given n.  Each thread keeps four running sums (one per
// float4 lane), so a running fp32 sum sees n / (4 * grid * 256) terms.
// ---------------------------------------------------------------------------

static inline int grad_sqsum_grid(int64_t n) {
    return ew_grid(n / 4 + 1, 256, 1);
}

extern "C" int grad_sqsum_blocks(int64_t n) { return grad_sqsum_grid(n); }

__global__ void __launch_bounds__(256)
k_grad_sqsum(const float* __restrict__ g, int64_t n,
             float* __restrict__ partials) {
    const int64_t n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4 acc{0.f, 0.f, 0.f, 0.f};
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 v = g4[i];
        acc.x += v.x * v.x;
        acc.y += v.y * v.y;
        acc.z += v.z * v.z;
        acc.w += v.w * v.w;
    }
    // scalar tail
    for (int64_t i = n4 * 4 + blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const float v = g[i];
        acc.x += v * v;
    }
    float sum = wave_sum((acc.x + acc.y) + (acc.z + acc.w));
    __shared__ float wave_part[256 / WAVE_SIZE];
    if ((threadIdx.x & (WAVE_SIZE - 1)) == 0)
        wave_part[threadIdx.x / WAVE_SIZE] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        partials[blockIdx.x] = (wave_part[0] + wave_part[1]) +
                               (wave_part[2] + wave_part[3]);
}

extern "C" void launch_grad_sqsum(const void* g, int64_t n, void* partials,
                                  hipStream_t stream) {
    k_grad_sqsum<<<grad_sqsum_grid(n), 256, 0, stream>>>(
        (const float*)g, n, (float*)partials);
}

// ---------------------------------------------------------------------------
// Pass 2 (one block): sum the partials of every group on this device in
// fixed order in fp64, derive the clip coefficient
//   coef = min(1, max_norm / (norm + 1e-6))      (torch clip_grad_norm_)
// and evaluate the LR schedule in closed form at the device step counter.
// The schedule's parameters are constants of the run, so they travel by
// value (frozen at graph capture, correctly).  The scalar math is fp64 in
// one thread; only the stored lr / coef / norm are rounded to fp32.
//
//   warm(s)  = start + (1 - start) * s / W                   for s < W
//   cosine   : floor + (1 - floor) * (1 + cos(pi * x)) / 2   x = (min(s,T)-W)/(T-W)
//   linear   : floor + (1 - floor) * (1 - x)
//   multistep: warm(s) * gamma ^ #{milestones <= s}
// ---------------------------------------------------------------------------

enum { SCHED_CONSTANT = 0, SCHED_COSINE = 1, SCHED_LINEAR = 2,
       SCHED_MULTISTEP = 3 };

#define SCHED_MAX_MILESTONES 8

struct SchedArgs {
    int kind;
    int n_milestones;
    long long warmup_steps;
    long long total_steps;
    long long milestones[SCHED_MAX_MILESTONES];
    double base_lr, start_factor, min_ratio, gamma;
};

__device__ __forceinline__ double sched_factor(const SchedArgs& s,
                                               long long step) {
    if (s.kind == SCHED_CONSTANT) return 1.0;
    if (step < 0) step = 0;
    const bool in_warmup = step < s.warmup_steps;
    const double warm = in_warmup
        ? s.start_factor + (1.0 - s.start_factor) *
              ((double)step / (double)s.warmup_steps)
        : 1.0;
    if (s.kind == SCHED_MULTISTEP) {
        int passed = 0;
        for (int i = 0; i < s.n_milestones; ++i)
            passed += s.milestones[i] <= step ? 1 : 0;
        return warm * pow(s.gamma, (double)passed);
    }
    if (in_warmup) return warm;
    const long long t = (step < s.total_steps ? step : s.total_steps) -
                        s.warmup_steps;
    const double x = (double)t / (double)(s.total_steps - s.warmup_steps);
    const double decay = s.kind == SCHED_COSINE
        ? 0.5 * (1.0 + cos(3.14159265358979323846 * x))
        : 1.0 - x;
    return s.min_ratio + (1.0 - s.min_ratio) * decay;
}

__global__ void __launch_bounds__(256)
k_optim_prepare(float* __restrict__ hyper, const float* __restrict__ partials,
                int n_partials, const long long* __restrict__ step_ptr,
                double max_norm, SchedArgs s) {
    __shared__ double red[256];
    double sq = 0.0;
    if (partials != nullptr) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < n_partials; i += 256)
            acc += (double)partials[i];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off)
                red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        sq = red[0];
    }
    if (threadIdx.x != 0) return;
    double norm = 0.0, coef = 1.0;
    if (partials != nullptr) {
        norm = sqrt(sq);
        const double c = max_norm / (norm + 1e-6);
        coef = c > 1.0 ? 1.0 : c;  // a NaN norm stays NaN, as in torch
    }
    // the counter holds the 1-based number of the step about to run; the
    // schedule is indexed from 0 (torch: scheduler.step() after optim.step())
    const long long step = step_ptr != nullptr ? *step_ptr - 1 : 0;
    hyper[HYPER_LR] = (float)(s.base_lr * sched_factor(s, step));
    hyper[HYPER_COEF] = (float)coef;
    hyper[HYPER_NORM] = (float)norm;
}

extern "C" void launch_optim_prepare(void* hyper, const void* partials,
                                     int n_partials, const void* step_dev,
                                     double max_norm, int kind, double base_lr,
                                     int64_t warmup_steps, double start_factor,
                                     int64_t total_steps, double min_ratio,
                                     const int64_t* milestones,
                                     int n_milestones, double gamma,
                                     hipStream_t stream) {
    SchedArgs s{};
    s.kind = kind;
    s.n_milestones = n_milestones < SCHED_MAX_MILESTONES
        ? n_milestones : SCHED_MAX_MILESTONES;
    s.warmup_steps = warmup_steps;
    s.total_steps = total_steps;
    for (int i = 0; i < s.n_milestones; ++i) s.milestones[i] = milestones[i];
    s.base_lr = base_lr;
    s.start_factor = start_factor;
    s.min_ratio = min_ratio;
    s.gamma = gamma;
    k_optim_prepare<<<1, 256, 0, stream>>>(
        (float*)hyper, (const float*)partials, n_partials,
        (const long long*)step_dev, max_norm, s);
}

// ---------------------------------------------------------------------------
// Segmented path: per-tensor weight decay / lr scale / LARS trust ratio.
//
// The flat kernels above do not know where one tensor ends.  The host cuts
// the arena once into CHUNKS: the intersection of a fixed window of
// SEG_CHUNK elements (window w covers [w * SEG_CHUNK, (w + 1) * SEG_CHUNK) of
// the flat index) with one tensor.  A chunk never crosses a tensor boundary,
// an edge between two chunks of one tensor is a window edge (a multiple of 4),
// and there are at most ceil(n / SEG_CHUNK) + T - 1 of them.  One block walks
// one chunk at a time: scalar head up to 16-byte alignment, float4 body,
// scalar tail.  The flat layout itself is untouched.
//
//   LARS (timm's Lars, trust_clip off), per tensor with lars on:
//     g' = grad_scale * clip_coef * g
//     ratio = eta * |p| / (|g'| + wd_t * |p| + eps)   if |p| > 0 and |g'| > 0
//             1                                        otherwise
//     d = ratio * (g' + wd_t * p)   then momentum as above, then
//     p -= lr * lr_scale_t * d
//   ratio = 1 is the plain SGD formula, so sgd_one is shared: the kernel
//   hands it grad_scale * ratio and wd_t * ratio.
// ---------------------------------------------------------------------------

#define SEG_THREADS 256

struct SegChunk {
    long long start;  // flat index of the first element
    int len;          // 1 .. SEG_CHUNK
    int tensor;       // index into the per-tensor arrays
};
static_assert(sizeof(SegChunk) == 16, "one 16-byte table entry per chunk");

struct SegArgs {
    const SegChunk* __restrict__ chunks;
    int n_chunks;
    const float* __restrict__ wd;        // [T]
    const float* __restrict__ lr_scale;  // [T]
    const float* __restrict__ ratio;     // [T] trust ratios (null = all 1)
};

static inline int seg_grid(int n_chunks) {
    return n_chunks < 1 ? 1 : (n_chunks > 2048 ? 2048 : n_chunks);
}

// `one(i)` handles flat element i, `four(i)` the aligned elements i .. i + 3
template <typename One, typename Four>
__device__ __forceinline__ void seg_walk(const SegChunk& c, One one,
                                         Four four) {
    const int to_align = (int)((4 - (c.start & 3)) & 3);
    const int head = to_align < c.len ? to_align : c.len;
    const int body4 = (c.len - head) >> 2;
    const int tail = c.len - head - body4 * 4;
    const int64_t body = c.start + head;
    if ((int)threadIdx.x < head) one(c.start + threadIdx.x);
#pragma unroll 4
    for (int i = threadIdx.x; i < body4; i += SEG_THREADS)
        four(body + 4 * (int64_t)i);
    if ((int)threadIdx.x < tail)
        one(body + 4 * (int64_t)body4 + threadIdx.x);
}

// (sum p^2, sum g^2) of every chunk.  No atomics, no pre-zeroing: every slot
// is overwritten, deterministic for a given table.  A running fp32 sum sees at
// most 6 terms (head, 4 float4 lanes at SEG_CHUNK = 4096, tail), then 2 lane,
// 6 wave and 2 block steps.
__global__ void __launch_bounds__(SEG_THREADS)
k_seg_sqsum(const float* __restrict__ p, const float* __restrict__ g,
            const SegChunk* __restrict__ chunks, int n_chunks,
            float2* __restrict__ partials) {
    __shared__ float2 wave_part[SEG_THREADS / WAVE_SIZE];
    for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        const SegChunk c = chunks[ci];
        float4 ap{0.f, 0.f, 0.f, 0.f}, ag{0.f, 0.f, 0.f, 0.f};
        seg_walk(c,
            [&](int64_t i) {
                const float x = p[i], y = g[i];
                ap.x += x * x;
                ag.x += y * y;
            },
            [&](int64_t i) {
                const float4 x = *reinterpret_cast<const float4*>(p + i);
                const float4 y = *reinterpret_cast<const float4*>(g + i);
                ap.x += x.x * x.x; ap.y += x.y * x.y;
                ap.z += x.z * x.z; ap.w += x.w * x.w;
                ag.x += y.x * y.x; ag.y += y.y * y.y;
                ag.z += y.z * y.z; ag.w += y.w * y.w;
            });
        const float sp = wave_sum((ap.x + ap.y) + (ap.z + ap.w));
        const float sg = wave_sum((ag.x + ag.y) + (ag.z + ag.w));
        if ((threadIdx.x & (WAVE_SIZE - 1)) == 0)
            wave_part[threadIdx.x / WAVE_SIZE] = float2{sp, sg};
        __syncthreads();
        if (threadIdx.x == 0) {
            const float2 w0 = wave_part[0], w1 = wave_part[1];
            const float2 w2 = wave_part[2], w3 = wave_part[3];
            partials[ci] = float2{(w0.x + w1.x) + (w2.x + w3.x),
                                  (w0.y + w1.y) + (w2.y + w3.y)};
        }
        __syncthreads();  // wave_part is reused by the next chunk
    }
}

extern "C" void launch_seg_sqsum(const void* p, const void* g,
                                 const void* chunks, int n_chunks,
                                 void* partials, hipStream_t stream) {
    k_seg_sqsum<<<seg_grid(n_chunks), SEG_THREADS, 0, stream>>>(
        (const float*)p, (const float*)g, (const SegChunk*)chunks, n_chunks,
        (float2*)partials);
}

// One wave per tensor: sum the tensor's chunk partials (chunks
// tensor_chunk[t] .. tensor_chunk[t + 1]) in fixed order in fp64 and write the
// trust ratio.  Runs after k_optim_prepare: the clip coefficient comes from the
// hyper block, so clipping composes with LARS under graph replay.
__global__ void __launch_bounds__(256)
k_lars_prepare(const float2* __restrict__ partials,
               const int* __restrict__ tensor_chunk,
               const float* __restrict__ wd, const int* __restrict__ lars_on,
               float* __restrict__ ratio, int n_tensors,
               const float* __restrict__ hyper, float grad_scale, double eta,
               double eps) {
    const int t = blockIdx.x * (256 / WAVE_SIZE) + threadIdx.x / WAVE_SIZE;
    const int lane = threadIdx.x & (WAVE_SIZE - 1);
    if (t >= n_tensors) return;  // wave-uniform
    const bool on = lars_on[t] != 0;
    double sp = 0.0, sg = 0.0;
    if (on) {
        const int end = tensor_chunk[t + 1];
        for (int c = tensor_chunk[t] + lane; c < end; c += WAVE_SIZE) {
            const float2 v = partials[c];
            sp += (double)v.x;
            sg += (double)v.y;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sp += __shfl_down(sp, off, WAVE_SIZE);
            sg += __shfl_down(sg, off, WAVE_SIZE);
        }
    }
    if (lane != 0) return;
    double r = 1.0;
    if (on) {
        const double coef = hyper != nullptr ? (double)hyper[HYPER_COEF] : 1.0;
        const double wn = sqrt(sp);
        const double gn = fabs((double)grad_scale * coef) * sqrt(sg);
        if (wn > 0.0 && gn > 0.0)
            r = eta * wn / (gn + (double)wd[t] * wn + eps);
    }
    ratio[t] = (float)r;
}

extern "C" void launch_lars_prepare(const void* partials,
                                    const void* tensor_chunk, const void* wd,
                                    const void* lars_on, void* ratio,
                                    int n_tensors, const void* hyper,
                                    float grad_scale, double eta, double eps,
                                    hipStream_t stream) {
    const int per_block = 256 / WAVE_SIZE;
    k_lars_prepare<<<(n_tensors + per_block - 1) / per_block, 256, 0, stream>>>(
        (const float2*)partials, (const int*)tensor_chunk, (const float*)wd,
        (const int*)lars_on, (float*)ratio, n_tensors, (const float*)hyper,
        grad_scale, eta, eps);
}

template <bool HAS_M, bool HAS_BF16>
__global__ void __launch_bounds__(SEG_THREADS)
k_fused_sgd_seg(SgdArgs a, SegArgs s) {
    if (a.hyper != nullptr) {
        a.lr = a.hyper[HYPER_LR];
        a.grad_scale *= a.hyper[HYPER_COEF];
    }
    const float lr = a.lr, grad_scale = a.grad_scale;
    for (int ci = blockIdx.x; ci < s.n_chunks; ci += gridDim.x) {
        const SegChunk c = s.chunks[ci];
        const float r = s.ratio != nullptr ? s.ratio[c.tensor] : 1.f;
        a.lr = lr * s.lr_scale[c.tensor];
        a.wd = s.wd[c.tensor] * r;
        a.grad_scale = grad_scale * r;
        seg_walk(c,
            [&](int64_t i) {
                float m = HAS_M ? a.m[i] : 0.f;
                const float p = sgd_one(a, a.p[i], a.g[i], m);
                a.p[i] = p;
                if (HAS_M) a.m[i] = m;
                if (HAS_BF16) a.p_bf16[i] = f32_to_bf16(p);
            },
            [&](int64_t i) {
                float4 p = *reinterpret_cast<float4*>(a.p + i);
                const float4 g = *reinterpret_cast<const float4*>(a.g + i);
                float4 m = HAS_M ? *reinterpret_cast<float4*>(a.m + i)
                                 : float4{0, 0, 0, 0};
                p.x = sgd_one(a, p.x, g.x, m.x);
                p.y = sgd_one(a, p.y, g.y, m.y);
                p.z = sgd_one(a, p.z, g.z, m.z);
                p.w = sgd_one(a, p.w, g.w, m.w);
                *reinterpret_cast<float4*>(a.p + i) = p;
                if (HAS_M) *reinterpret_cast<float4*>(a.m + i) = m;
                if (HAS_BF16) {
                    ushort4 b;
                    b.x = f32_to_bf16(p.x); b.y = f32_to_bf16(p.y);
                    b.z = f32_to_bf16(p.z); b.w = f32_to_bf16(p.w);
                    *reinterpret_cast<ushort4*>(a.p_bf16 + i) = b;
                }
            });
    }
}

extern "C" void launch_fused_sgd_seg(void* p, const void* g, void* m,
                                     void* p_bf16, int64_t n, float lr,
                                     float momentum, float grad_scale,
                                     int nesterov, const void* hyper,
                                     const void* chunks, int n_chunks,
                                     const void* wd, const void* lr_scale,
                                     const void* ratio, hipStream_t stream) {
    SgdArgs a{(float*)p, (const float*)g, (float*)m, (uint16_t*)p_bf16,
              n, lr, momentum, 0.f, grad_scale, nesterov, (const float*)hyper};
    SegArgs s{(const SegChunk*)chunks, n_chunks, (const float*)wd,
              (const float*)lr_scale, (const float*)ratio};
    const int grid = seg_grid(n_chunks);
    if (m != nullptr && p_bf16 != nullptr)
        k_fused_sgd_seg<true, true><<<grid, SEG_THREADS, 0, stream>>>(a, s);
    else if (m != nullptr)
        k_fused_sgd_seg<true, false><<<grid, SEG_THREADS, 0, stream>>>(a, s);
    else if (p_bf16 != nullptr)
        k_fused_sgd_seg<false, true><<<grid, SEG_THREADS, 0, stream>>>(a, s);
    else
        k_fused_sgd_seg<false, false><<<grid, SEG_THREADS, 0, stream>>>(a, s);
}

template <bool HAS_BF16>
__global__ void __launch_bounds__(SEG_THREADS)
k_fused_adam_seg(AdamArgs a, SegArgs s) {
    if (a.step_ptr != nullptr) {
        const float t = (float)*a.step_ptr;
        a.bc1 = 1.f - powf(a.beta1, t);
        a.bc2 = 1.f - powf(a.beta2, t);
    }
    if (a.hyper != nullptr) {
        a.lr = a.hyper[HYPER_LR];
        a.grad_scale *= a.hyper[HYPER_COEF];
    }
    const float lr = a.lr;
    for (int ci = blockIdx.x; ci < s.n_chunks; ci += gridDim.x) {
        const SegChunk c = s.chunks[ci];
        a.lr = lr * s.lr_scale[c.tensor];
        a.wd = s.wd[c.tensor];
        seg_walk(c,
            [&](int64_t i) {
                float m = a.m[i], v = a.v[i];
                const float p = adam_one(a, a.p[i], a.g[i], m, v);
                a.p[i] = p;
                a.m[i] = m;
                a.v[i] = v;
                if (HAS_BF16) a.p_bf16[i] = f32_to_bf16(p);
            },
            [&](int64_t i) {
                float4 p = *reinterpret_cast<float4*>(a.p + i);
                const float4 g = *reinterpret_cast<const float4*>(a.g + i);
                float4 m = *reinterpret_cast<float4*>(a.m + i);
                float4 v = *reinterpret_cast<float4*>(a.v + i);
                p.x = adam_one(a, p.x, g.x, m.x, v.x);
                p.y = adam_one(a, p.y, g.y, m.y, v.y);
                p.z = adam_one(a, p.z, g.z, m.z, v.z);
                p.w = adam_one(a, p.w, g.w, m.w, v.w);
                *reinterpret_cast<float4*>(a.p + i) = p;
                *reinterpret_cast<float4*>(a.m + i) = m;
                *reinterpret_cast<float4*>(a.v + i) = v;
                if (HAS_BF16) {
                    ushort4 b;
                    b.x = f32_to_bf16(p.x); b.y = f32_to_bf16(p.y);
                    b.z = f32_to_bf16(p.z); b.w = f32_to_bf16(p.w);
                    *reinterpret_cast<ushort4*>(a.p_bf16 + i) = b;
                }
            });
    }
}

extern "C" void launch_fused_adam_seg(void* p, const void* g, void* m, void* v,
                                      void* p_bf16, void* step_dev, int64_t n,
                                      float lr, float beta1, float beta2,
                                      float eps, int64_t step,
                                      float grad_scale, int adamw,
                                      const void* hyper, const void* chunks,
                                      int n_chunks, const void* wd,
                                      const void* lr_scale,
                                      hipStream_t stream) {
    AdamArgs a{(float*)p, (const float*)g, (float*)m, (float*)v,
               (uint16_t*)p_bf16, (const long long*)step_dev,
               (const float*)hyper, n, lr, beta1,
               beta2, eps, 0.f,
               1.f - powf(beta1, (float)step), 1.f - powf(beta2, (float)step),
               grad_scale, adamw};
    SegArgs s{(const SegChunk*)chunks, n_chunks, (const float*)wd,
              (const float*)lr_scale, nullptr};
    const int grid = seg_grid(n_chunks);
    if (p_bf16 != nullptr)
        k_fused_adam_seg<true><<<grid, SEG_THREADS, 0, stream>>>(a, s);
    else
        k_fused_adam_seg<false><<<grid, SEG_THREADS, 0, stream>>>(a, s);
}

// Copyright (c) Flashy-AMD authors.
// pybind11 bindings for the gfx950 kernels.  Torch-ABI-free by design: the
// Python wrappers (flashy_amd/ops/__init__.py) pass raw device pointers
// (tensor.data_ptr()) and the current HIP stream handle
// (torch.cuda.current_stream().cuda_stream); all launches go onto that
// stream, so they are captured by HIP graphs like any other kernel.

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "conv8.h"   // ConvDims + the 8-wave plan/launch prototypes

namespace py = pybind11;

extern "C" {
void launch_conv_fwd(const void* x, const void* w, void* y, ConvDims d,
                     int relu, void* bn_ws, hipStream_t stream);
int conv_fwd_msplit(ConvDims d);
void launch_stem_pad_x(const void* x, void* xp, int64_t N, int H, int W,
                       int Hp, int Wp, int pad, hipStream_t stream);
void launch_stem_pad_w(const void* w, void* wp, int K, int R, int S,
                       hipStream_t stream);
void launch_stem_unpad_dw(const void* dwp, void* dw, int K, int R, int S,
                          hipStream_t stream);
void launch_conv_stem_fwd(const void* x, const void* w, void* y, ConvDims d,
                          hipStream_t stream);
void launch_conv_stem_wgrad(const void* x, const void* dout, void* dw,
                            ConvDims d, hipStream_t stream);
void launch_conv_stem_dgrad(const void* dout, const void* w, void* dx,
                            ConvDims d, hipStream_t stream);
void launch_conv_dgrad(const void* dout, const void* w_rsck, void* dx,
                       ConvDims d, hipStream_t stream);
void launch_conv_fwd_splitk(const void* x, const void* w, void* ws, ConvDims d,
                            int zn, hipStream_t stream);
void launch_conv_dgrad_splitk(const void* dout, const void* w_rsck, void* ws,
                              ConvDims d, int zn, hipStream_t stream);
void launch_splitk_combine(const void* ws, void* out, int64_t total, int zn,
                           int relu, hipStream_t stream);
void launch_splitk_combine_stats(const void* ws, void* out, void* partials,
                                 int64_t M, int K, int zn, int msplit,
                                 hipStream_t stream);
void launch_pool_fc_fwd(const void* x, const void* w, const void* b,
                        void* pooled, void* y, int N, int HW, int C, int O,
                        hipStream_t stream);
void launch_head_dw(const void* pooled, const void* dy, void* dw, void* db,
                    int B, int C, int O, hipStream_t stream);
void launch_head_dx(const void* dy, const void* w, void* dx, int N, int HW,
                    int C, int O, hipStream_t stream);
void launch_weight_transpose(const void* w, void* wt, int K, int rsc,
                             hipStream_t stream);
void launch_weight_transpose_batched(const void* src, void* dst,
                                     const void* meta, int n_convs,
                                     int64_t max_elems, hipStream_t stream);
void launch_conv_wgrad(const void* x, const void* dout, void* dw, ConvDims d,
                       int n_splits, hipStream_t stream);
void launch_bn_stats(const void* x, void* partials, int64_t M, int C,
                     int msplit, hipStream_t stream);
void launch_bn_finalize(const void* partials, int msplit, const void* gamma,
                        const void* beta, void* running_mean,
                        void* running_var, void* work, int64_t M, int C,
                        float eps, float momentum, int update_running,
                        hipStream_t stream);
void launch_bn_apply(const void* x, const void* res, void* y, const void* work,
                     int64_t M, int C, int relu, float slope,
                     hipStream_t stream);
void launch_bn_bwd_reduce(const void* dy, const void* y, const void* x,
                          const void* work, void* dz_out, void* partials,
                          int64_t M, int C, int msplit, int relu, float slope,
                          hipStream_t stream);
void launch_bn_bwd_grads(const void* partials, int msplit, void* bsums,
                         void* dgamma, void* dbeta, int C, hipStream_t stream);
void launch_bn_bwd_apply(const void* dz, const void* x, const void* work,
                         const void* bsums, void* dx, int64_t M, int C,
                         hipStream_t stream);
void bn_small_plan(int64_t M, int C, int* fwd_form, int* bwd_form);
int launch_bn_fwd_small(const void* partials, int msplit, const void* gamma,
                        const void* beta, void* running_mean,
                        void* running_var, void* work, const void* x,
                        const void* res, void* y, int64_t M, int C, float eps,
                        float momentum, int update_running, int relu,
                        float slope, int form, hipStream_t stream);
int launch_bn_bwd_small(const void* dy, const void* y, const void* x,
                        const void* work, void* dz, void* dgamma, void* dbeta,
                        void* dx, int64_t M, int C, int relu, float slope,
                        int write_dz, int form, hipStream_t stream);
void launch_fused_sgd(void* p, const void* g, void* m, void* p_bf16, int64_t n,
                      float lr, float momentum, float wd, float grad_scale,
                      int nesterov, const void* hyper, hipStream_t stream);
void launch_fused_adam(void* p, const void* g, void* m, void* v, void* p_bf16,
                       void* step_dev, int64_t n, float lr, float beta1,
                       float beta2, float eps, float wd, int64_t step,
                       float grad_scale, int adamw, const void* hyper,
                       hipStream_t stream);
void launch_adam_step_inc(void* p, hipStream_t stream);
int grad_sqsum_blocks(int64_t n);
void launch_grad_sqsum(const void* g, int64_t n, void* partials,
                       hipStream_t stream);
void launch_optim_prepare(void* hyper, const void* partials, int n_partials,
                          const void* step_dev, double max_norm, int kind,
                          double base_lr, int64_t warmup_steps,
                          double start_factor, int64_t total_steps,
                          double min_ratio, const int64_t* milestones,
                          int n_milestones, double gamma, hipStream_t stream);
void launch_seg_sqsum(const void* p, const void* g, const void* chunks,
                      int n_chunks, void* partials, hipStream_t stream);
void launch_lars_prepare(const void* partials, const void* tensor_chunk,
                         const void* wd, const void* lars_on, void* ratio,
                         int n_tensors, const void* hyper, float grad_scale,
                         double eta, double eps, hipStream_t stream);
void launch_fused_sgd_seg(void* p, const void* g, void* m, void* p_bf16,
                          int64_t n, float lr, float momentum,
                          float grad_scale, int nesterov, const void* hyper,
                          const void* chunks, int n_chunks, const void* wd,
                          const void* lr_scale, const void* ratio,
                          hipStream_t stream);
void launch_fused_adam_seg(void* p, const void* g, void* m, void* v,
                           void* p_bf16, void* step_dev, int64_t n, float lr,
                           float beta1, float beta2, float eps, int64_t step,
                           float grad_scale, int adamw, const void* hyper,
                           const void* chunks, int n_chunks, const void* wd,
                           const void* lr_scale, hipStream_t stream);
void launch_image_ingest(const void* src, void* out, const void* step_dev,
                         int N, int H, int W, int OH, int OW, int pad,
                         uint64_t seed, uint32_t flip_thresh,
                         const float* scale, const float* bias, int fill,
                         int train, hipStream_t stream);
void launch_resized_crop_draw(void* boxes, const void* tables,
                              const void* step_dev, int N, int H, int W,
                              int OH, int OW, uint64_t seed, uint64_t root_hw,
                              uint32_t flip_thresh, uint32_t r0, uint32_t r1,
                              uint32_t eval_crop, int train,
                              hipStream_t stream);
void launch_resized_crop(const void* src, void* out, const void* boxes, int N,
                         int H, int W, int OH, int OW, const float* scale,
                         const float* bias, hipStream_t stream);
void launch_batch_mix_draw(void* row, const void* lam_table,
                           const void* sq_table, const void* step_dev, int H,
                           int W, uint64_t seed, uint32_t prob_thresh,
                           uint32_t switch_thresh, int mixup, int cutmix,
                           hipStream_t stream);
void launch_batch_mix(void* x, const void* row, int N, int H, int W, int C,
                      hipStream_t stream);
void launch_cross_entropy_mix(const void* logits, const void* target,
                              const void* target_b, const void* lam,
                              void* dlogits, void* loss_sum, int64_t B,
                              int64_t C, float eps, float loss_scale,
                              float grad_scale, int is_bf16,
                              hipStream_t stream);
void launch_maxpool_fwd(const void* x, void* y, void* argmax, ConvDims d,
                        hipStream_t stream);
void launch_maxpool_bwd(const void* dy, const void* argmax, void* dx,
                        ConvDims d, hipStream_t stream);
void launch_cross_entropy(const void* logits, const void* target, void* dlogits,
                          void* loss_sum, int64_t B, int64_t C,
                          float loss_scale, float grad_scale, int is_bf16,
                          hipStream_t stream);
void launch_mse(const void* x, const void* t, void* dx, void* loss_sum,
                int64_t n, float loss_scale, float grad_scale, int is_bf16,
                hipStream_t stream);
void launch_accuracy(const void* logits, const void* target, void* out,
                     int64_t B, int64_t C, int is_bf16, hipStream_t stream);
void launch_linear_fwd(const void* x, const void* w, const void* b, void* y,
                       int64_t B, int64_t I, int64_t O, hipStream_t stream);
void launch_linear_dx(const void* dy, const void* w, void* dx, int64_t B,
                      int64_t I, int64_t O, hipStream_t stream);
void launch_linear_dw(const void* x, const void* dy, void* dw, void* db,
                      int64_t B, int64_t I, int64_t O, hipStream_t stream);
void launch_bce_logits(const void* x, void* dx, void* loss_sum, int64_t n,
                       float target, float loss_scale, float grad_scale,
                       int is_bf16, hipStream_t stream);
}

static void check_last() {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        throw std::runtime_error(std::string("HIP launch failed: ") +
                                 hipGetErrorString(err));
}

static hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

static ConvDims make_dims(int N, int H, int W, int C, int K, int R, int S,
                          int Ho, int Wo, int stride, int pad) {
    return ConvDims{N, H, W, C, K, R, S, Ho, Wo, stride, pad};
}

PYBIND11_MODULE(_hip_ops, m) {
    m.doc() = "flashy_amd gfx950 kernels";
    m.attr("ARCH") = "gfx950";

    m.def("conv_fwd",
          [](uintptr_t x, uintptr_t w, uintptr_t y, int N, int H, int W, int C,
             int K, int R, int S, int Ho, int Wo, int stride, int pad,
             bool relu, uintptr_t bn_ws, uintptr_t stream) {
              launch_conv_fwd((const void*)x, (const void*)w, (void*)y,
                              make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                              relu ? 1 : 0, (void*)bn_ws, as_stream(stream));
              check_last();
          });
    m.def("conv_fwd8_direct",
          [](uintptr_t x, uintptr_t w, uintptr_t y, int N, int H, int W,
             int C, int K, int R, int S, int Ho, int Wo, int stride, int pad,
             bool relu, uintptr_t bn_ws, int bn, int mtiles,
             uintptr_t stream) {
              launch_conv_fwd8((const void*)x, (const void*)w, (void*)y,
                               make_dims(N, H, W, C, K, R, S, Ho, Wo, stride,
                                         pad),
                               relu, (void*)bn_ws, bn, mtiles,
                               as_stream(stream));
              check_last();
          });

    m.def("stem_pad_x",
          [](uintptr_t x, uintptr_t xp, int64_t N, int H, int W, int Hp,
             int Wp, int pad, uintptr_t stream) {
              launch_stem_pad_x((const void*)x, (void*)xp, N, H, W, Hp, Wp,
                                pad, as_stream(stream));
              check_last();
          });

    m.def("stem_pad_w",
          [](uintptr_t w, uintptr_t wp, int K, int R, int S,
             uintptr_t stream) {
              launch_stem_pad_w((const void*)w, (void*)wp, K, R, S,
                                as_stream(stream));
              check_last();
          });

    m.def("stem_unpad_dw",
          [](uintptr_t dwp, uintptr_t dw, int K, int R, int S,
             uintptr_t stream) {
              launch_stem_unpad_dw((const void*)dwp, (void*)dw, K, R, S,
                                   as_stream(stream));
              check_last();
          });

    m.def("conv8_eligible",
          [](int N, int H, int W, int C, int K, int R, int S, int Ho, int Wo,
             int stride, int pad, bool dgrad) {
              int bn = 0;
              ConvDims d = make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad);
              return (dgrad ? conv_dgrad8_plan(d, &bn)
                            : conv_fwd8_plan(d, &bn)) > 0;
          });

    m.def("conv_fwd_msplit",
          [](int N, int H, int W, int C, int K, int R, int S, int Ho, int Wo,
             int stride, int pad) {
              return conv_fwd_msplit(
                  make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad));
          });
    m.def("conv_stem_fwd",
          [](uintptr_t x, uintptr_t w, uintptr_t y, int N, int H, int W, int C,
             int K, int R, int S, int Ho, int Wo, int stride, int pad,
             uintptr_t stream) {
              launch_conv_stem_fwd((const void*)x, (const void*)w, (void*)y,
                                   make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                   as_stream(stream));
              check_last();
          });
    m.def("conv_stem_wgrad",
          [](uintptr_t x, uintptr_t dout, uintptr_t dw, int N, int H, int W,
             int C, int K, int R, int S, int Ho, int Wo, int stride, int pad,
             uintptr_t stream) {
              launch_conv_stem_wgrad((const void*)x, (const void*)dout,
                                     (void*)dw,
                                     make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                     as_stream(stream));
              check_last();
          });
    m.def("conv_stem_dgrad",
          [](uintptr_t dout, uintptr_t w, uintptr_t dx, int N, int H, int W,
             int C, int K, int R, int S, int Ho, int Wo, int stride, int pad,
             uintptr_t stream) {
              launch_conv_stem_dgrad((const void*)dout, (const void*)w,
                                     (void*)dx,
                                     make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                     as_stream(stream));
              check_last();
          });
    m.def("conv_dgrad",
          [](uintptr_t dout, uintptr_t w_rsck, uintptr_t dx, int N, int H,
             int W, int C, int K, int R, int S, int Ho, int Wo, int stride,
             int pad, uintptr_t stream) {
              launch_conv_dgrad((const void*)dout, (const void*)w_rsck,
                                (void*)dx,
                                make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                as_stream(stream));
              check_last();
          });
    // stride-2 dgrad: the plan's (form, tile), and one form launched by name
    // (tests and scripts/dgrad_s2_sweep.py; form 0 = the generic kernels)
    m.def("conv_dgrad_s2_plan",
          [](int N, int H, int W, int C, int K, int R, int S, int Ho, int Wo,
             int stride, int pad) {
              int tile = 0;
              const int form = conv_dgrad_s2_plan(
                  make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad), &tile);
              return py::make_tuple(form, tile);
          });
    m.def("conv_dgrad_s2_form",
          [](uintptr_t dout, uintptr_t w_rsck, uintptr_t dx, int N, int H,
             int W, int C, int K, int R, int S, int Ho, int Wo, int stride,
             int pad, int form, int tile, uintptr_t stream) {
              if (!launch_conv_dgrad_s2_form(
                      (const void*)dout, (const void*)w_rsck, (void*)dx,
                      make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                      form, tile, as_stream(stream)))
                  throw std::invalid_argument(
                      "conv_dgrad_s2_form: form/tile cannot run this shape");
              check_last();
          });
    m.def("conv_fwd_splitk",
          [](uintptr_t x, uintptr_t w, uintptr_t ws, int N, int H, int W,
             int C, int K, int R, int S, int Ho, int Wo, int stride, int pad,
             int zn, uintptr_t stream) {
              launch_conv_fwd_splitk((const void*)x, (const void*)w, (void*)ws,
                                     make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                     zn, as_stream(stream));
              check_last();
          });
    m.def("conv_dgrad_splitk",
          [](uintptr_t dout, uintptr_t w_rsck, uintptr_t ws, int N, int H,
             int W, int C, int K, int R, int S, int Ho, int Wo, int stride,
             int pad, int zn, uintptr_t stream) {
              launch_conv_dgrad_splitk((const void*)dout, (const void*)w_rsck,
                                       (void*)ws,
                                       make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                       zn, as_stream(stream));
              check_last();
          });
    m.def("splitk_combine",
          [](uintptr_t ws, uintptr_t out, int64_t total, int zn, bool relu,
             uintptr_t stream) {
              launch_splitk_combine((const void*)ws, (void*)out, total, zn,
                                    relu ? 1 : 0, as_stream(stream));
              check_last();
          });
    m.def("splitk_combine_stats",
          [](uintptr_t ws, uintptr_t out, uintptr_t partials, int64_t M, int K,
             int zn, int msplit, uintptr_t stream) {
              launch_splitk_combine_stats((const void*)ws, (void*)out,
                                          (void*)partials, M, K, zn, msplit,
                                          as_stream(stream));
              check_last();
          });
    m.def("weight_transpose",
          [](uintptr_t w, uintptr_t wt, int K, int rsc, uintptr_t stream) {
              launch_weight_transpose((const void*)w, (void*)wt, K, rsc,
                                      as_stream(stream));
              check_last();
          });
    m.def("weight_transpose_batched",
          [](uintptr_t src, uintptr_t dst, uintptr_t meta, int n_convs,
             int64_t max_elems, uintptr_t stream) {
              launch_weight_transpose_batched((const void*)src, (void*)dst,
                                              (const void*)meta, n_convs,
                                              max_elems, as_stream(stream));
              check_last();
          });
    m.def("conv_wgrad",
          [](uintptr_t x, uintptr_t dout, uintptr_t dw, int N, int H, int W,
             int C, int K, int R, int S, int Ho, int Wo, int stride, int pad,
             int n_splits, uintptr_t stream) {
              launch_conv_wgrad((const void*)x, (const void*)dout, (void*)dw,
                                make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                n_splits, as_stream(stream));
              check_last();
          });
    m.def("bn_stats",
          [](uintptr_t x, uintptr_t partials, int64_t M, int C, int msplit,
             uintptr_t stream) {
              launch_bn_stats((const void*)x, (void*)partials, M, C, msplit,
                              as_stream(stream));
              check_last();
          });
    m.def("bn_finalize",
          [](uintptr_t partials, int msplit, uintptr_t gamma, uintptr_t beta,
             uintptr_t rmean, uintptr_t rvar, uintptr_t work, int64_t M, int C,
             float eps, float momentum, bool update_running, uintptr_t stream) {
              launch_bn_finalize((const void*)partials, msplit,
                                 (const void*)gamma, (const void*)beta,
                                 (void*)rmean, (void*)rvar, (void*)work, M, C,
                                 eps, momentum, update_running ? 1 : 0,
                                 as_stream(stream));
              check_last();
          });
    m.def("bn_apply",
          [](uintptr_t x, uintptr_t res, uintptr_t y, uintptr_t work, int64_t M,
             int C, bool relu, float slope, uintptr_t stream) {
              launch_bn_apply((const void*)x, (const void*)res, (void*)y,
                              (const void*)work, M, C, relu ? 1 : 0, slope,
                              as_stream(stream));
              check_last();
          });
    m.def("bn_bwd_reduce",
          [](uintptr_t dy, uintptr_t y, uintptr_t x, uintptr_t work,
             uintptr_t dz_out, uintptr_t partials, int64_t M, int C,
             int msplit, bool relu, float slope, uintptr_t stream) {
              launch_bn_bwd_reduce((const void*)dy, (const void*)y,
                                   (const void*)x, (const void*)work,
                                   (void*)dz_out, (void*)partials, M, C,
                                   msplit, relu ? 1 : 0, slope,
                                   as_stream(stream));
              check_last();
          });
    m.def("bn_bwd_grads",
          [](uintptr_t partials, int msplit, uintptr_t bsums, uintptr_t dgamma,
             uintptr_t dbeta, int C, uintptr_t stream) {
              launch_bn_bwd_grads((const void*)partials, msplit, (void*)bsums,
                                  (void*)dgamma, (void*)dbeta, C,
                                  as_stream(stream));
              check_last();
          });
    m.def("bn_bwd_apply",
          [](uintptr_t dz, uintptr_t x, uintptr_t work, uintptr_t bsums,
             uintptr_t dx, int64_t M, int C, uintptr_t stream) {
              launch_bn_bwd_apply((const void*)dz, (const void*)x,
                                  (const void*)work, (const void*)bsums,
                                  (void*)dx, M, C, as_stream(stream));
              check_last();
          });
    // small-M single-kernel BatchNorm: the plan's (fwd form, bwd form), and
    // one form launched by name (tests and scripts/bn_small_sweep.py)
    m.def("bn_small_plan", [](int64_t M, int C) {
        int fwd = 0, bwd = 0;
        bn_small_plan(M, C, &fwd, &bwd);
        return py::make_tuple(fwd, bwd);
    });
    m.def("bn_fwd_small",
          [](uintptr_t partials, int msplit, uintptr_t gamma, uintptr_t beta,
             uintptr_t rmean, uintptr_t rvar, uintptr_t work, uintptr_t x,
             uintptr_t res, uintptr_t y, int64_t M, int C, float eps,
             float momentum, bool update_running, bool relu, float slope,
             int form, uintptr_t stream) {
              if (!launch_bn_fwd_small(
                      (const void*)partials, msplit, (const void*)gamma,
                      (const void*)beta, (void*)rmean, (void*)rvar,
                      (void*)work, (const void*)x, (const void*)res, (void*)y,
                      M, C, eps, momentum, update_running ? 1 : 0,
                      relu ? 1 : 0, slope, form, as_stream(stream)))
                  throw std::invalid_argument(
                      "bn_fwd_small: form cannot run this shape");
              check_last();
          });
    m.def("bn_bwd_small",
          [](uintptr_t dy, uintptr_t y, uintptr_t x, uintptr_t work,
             uintptr_t dz, uintptr_t dgamma, uintptr_t dbeta, uintptr_t dx,
             int64_t M, int C, bool relu, float slope, bool write_dz, int form,
             uintptr_t stream) {
              if (!launch_bn_bwd_small(
                      (const void*)dy, (const void*)y, (const void*)x,
                      (const void*)work, (void*)dz, (void*)dgamma,
                      (void*)dbeta, (void*)dx, M, C, relu ? 1 : 0, slope,
                      write_dz ? 1 : 0, form, as_stream(stream)))
                  throw std::invalid_argument(
                      "bn_bwd_small: form cannot run this shape");
              check_last();
          });

    // `hyper` (trailing, default 0): device block written by optim_prepare;
    // when set, the kernel reads lr and the clip coefficient from it.
    m.def("fused_sgd",
          [](uintptr_t p, uintptr_t g, uintptr_t mom, uintptr_t p_bf16,
             int64_t n, float lr, float momentum, float wd, float grad_scale,
             bool nesterov, uintptr_t stream, uintptr_t hyper) {
              launch_fused_sgd((void*)p, (const void*)g, (void*)mom,
                               (void*)p_bf16, n, lr, momentum, wd, grad_scale,
                               nesterov ? 1 : 0, (const void*)hyper,
                               as_stream(stream));
              check_last();
          },
          py::arg("p"), py::arg("g"), py::arg("mom"), py::arg("p_bf16"),
          py::arg("n"), py::arg("lr"), py::arg("momentum"), py::arg("wd"),
          py::arg("grad_scale"), py::arg("nesterov"), py::arg("stream"),
          py::arg("hyper") = (uintptr_t)0);

    m.def("fused_adam",
          [](uintptr_t p, uintptr_t g, uintptr_t mom, uintptr_t var,
             uintptr_t p_bf16, uintptr_t step_dev, int64_t n, float lr,
             float beta1, float beta2, float eps, float wd, int64_t step,
             float grad_scale, bool adamw, uintptr_t stream,
             uintptr_t hyper) {
              launch_fused_adam((void*)p, (const void*)g, (void*)mom,
                                (void*)var, (void*)p_bf16, (void*)step_dev, n,
                                lr, beta1, beta2, eps, wd, step, grad_scale,
                                adamw ? 1 : 0, (const void*)hyper,
                                as_stream(stream));
              check_last();
          },
          py::arg("p"), py::arg("g"), py::arg("mom"), py::arg("var"),
          py::arg("p_bf16"), py::arg("step_dev"), py::arg("n"), py::arg("lr"),
          py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("wd"),
          py::arg("step"), py::arg("grad_scale"), py::arg("adamw"),
          py::arg("stream"), py::arg("hyper") = (uintptr_t)0);
    m.def("adam_step_inc", [](uintptr_t p, uintptr_t stream) {
        launch_adam_step_inc((void*)p, as_stream(stream));
        check_last();
    });
    m.def("grad_sqsum_blocks", [](int64_t n) { return grad_sqsum_blocks(n); });
    m.def("grad_sqsum",
          [](uintptr_t g, int64_t n, uintptr_t partials, uintptr_t stream) {
              launch_grad_sqsum((const void*)g, n, (void*)partials,
                                as_stream(stream));
              check_last();
          });
    m.def("optim_prepare",
          [](uintptr_t hyper, uintptr_t partials, int n_partials,
             uintptr_t step_dev, double max_norm, int kind, double base_lr,
             int64_t warmup_steps, double start_factor, int64_t total_steps,
             double min_ratio, const std::vector<int64_t>& milestones,
             double gamma, uintptr_t stream) {
              if (milestones.size() > 8)
                  throw std::invalid_argument("at most 8 milestones");
              launch_optim_prepare((void*)hyper, (const void*)partials,
                                   n_partials, (const void*)step_dev, max_norm,
                                   kind, base_lr, warmup_steps, start_factor,
                                   total_steps, min_ratio, milestones.data(),
                                   (int)milestones.size(), gamma,
                                   as_stream(stream));
              check_last();
          });
    // segmented path (per-tensor wd / lr scale / LARS): `chunks` is the
    // device chunk table, 16 bytes per entry; wd / lr_scale / lars_on / ratio
    // are per-tensor arrays; tensor_chunk has one more entry than tensors
    m.def("seg_sqsum",
          [](uintptr_t p, uintptr_t g, uintptr_t chunks, int n_chunks,
             uintptr_t partials, uintptr_t stream) {
              launch_seg_sqsum((const void*)p, (const void*)g,
                               (const void*)chunks, n_chunks, (void*)partials,
                               as_stream(stream));
              check_last();
          });
    m.def("lars_prepare",
          [](uintptr_t partials, uintptr_t tensor_chunk, uintptr_t wd,
             uintptr_t lars_on, uintptr_t ratio, int n_tensors,
             uintptr_t hyper, float grad_scale, double eta, double eps,
             uintptr_t stream) {
              launch_lars_prepare((const void*)partials,
                                  (const void*)tensor_chunk, (const void*)wd,
                                  (const void*)lars_on, (void*)ratio,
                                  n_tensors, (const void*)hyper, grad_scale,
                                  eta, eps, as_stream(stream));
              check_last();
          });
    m.def("fused_sgd_seg",
          [](uintptr_t p, uintptr_t g, uintptr_t mom, uintptr_t p_bf16,
             int64_t n, float lr, float momentum, float grad_scale,
             bool nesterov, uintptr_t hyper, uintptr_t chunks, int n_chunks,
             uintptr_t wd, uintptr_t lr_scale, uintptr_t ratio,
             uintptr_t stream) {
              launch_fused_sgd_seg((void*)p, (const void*)g, (void*)mom,
                                   (void*)p_bf16, n, lr, momentum, grad_scale,
                                   nesterov ? 1 : 0, (const void*)hyper,
                                   (const void*)chunks, n_chunks,
                                   (const void*)wd, (const void*)lr_scale,
                                   (const void*)ratio, as_stream(stream));
              check_last();
          });
    m.def("fused_adam_seg",
          [](uintptr_t p, uintptr_t g, uintptr_t mom, uintptr_t var,
             uintptr_t p_bf16, uintptr_t step_dev, int64_t n, float lr,
             float beta1, float beta2, float eps, int64_t step,
             float grad_scale, bool adamw, uintptr_t hyper, uintptr_t chunks,
             int n_chunks, uintptr_t wd, uintptr_t lr_scale,
             uintptr_t stream) {
              launch_fused_adam_seg((void*)p, (const void*)g, (void*)mom,
                                    (void*)var, (void*)p_bf16, (void*)step_dev,
                                    n, lr, beta1, beta2, eps, step, grad_scale,
                                    adamw ? 1 : 0, (const void*)hyper,
                                    (const void*)chunks, n_chunks,
                                    (const void*)wd, (const void*)lr_scale,
                                    as_stream(stream));
              check_last();
          });
    // uint8 NHWC -> bf16 NHWC crop / flip / normalize (csrc/ingest.hip);
    // step_dev = 0 is allowed in eval mode only (train = false)
    m.def("image_ingest",
          [](uintptr_t src, uintptr_t out, uintptr_t step_dev, int N, int H,
             int W, int OH, int OW, int pad, uint64_t seed,
             uint32_t flip_thresh, const std::vector<float>& scale,
             const std::vector<float>& bias, int fill, bool train,
             uintptr_t stream) {
              if (scale.size() != 3 || bias.size() != 3)
                  throw std::invalid_argument("scale and bias take 3 values");
              if (train && step_dev == 0)
                  throw std::invalid_argument("train mode needs step_dev");
              launch_image_ingest((const void*)src, (void*)out,
                                  (const void*)step_dev, N, H, W, OH, OW, pad,
                                  seed, flip_thresh, scale.data(), bias.data(),
                                  fill, train, as_stream(stream));
              check_last();
          });
    // random resized crop (csrc/ingest.hip): the per-sample boxes, int32
    // [N, 8], then the bilinear resample that reads them
    m.def("resized_crop_draw",
          [](uintptr_t boxes, uintptr_t tables, uintptr_t step_dev, int N,
             int H, int W, int OH, int OW, uint64_t seed, uint64_t root_hw,
             uint32_t flip_thresh, uint32_t r0, uint32_t r1,
             uint32_t eval_crop, bool train, uintptr_t stream) {
              if (train && step_dev == 0)
                  throw std::invalid_argument("train mode needs step_dev");
              if (boxes == 0 || boxes % 16 != 0 || tables == 0)
                  throw std::invalid_argument(
                      "boxes must be 16-byte aligned, tables non-null");
              if (N < 1 || OH < 1 || OW < 1 || H < 1 || W < 1 ||
                  H > 32767 || W > 32767 || r0 == 0 || r1 == 0)
                  throw std::invalid_argument("resized_crop_draw: bad sizes");
              launch_resized_crop_draw((void*)boxes, (const void*)tables,
                                       (const void*)step_dev, N, H, W, OH, OW,
                                       seed, root_hw, flip_thresh, r0, r1,
                                       eval_crop, train, as_stream(stream));
              check_last();
          });
    m.def("resized_crop",
          [](uintptr_t src, uintptr_t out, uintptr_t boxes, int N, int H,
             int W, int OH, int OW, const std::vector<float>& scale,
             const std::vector<float>& bias, uintptr_t stream) {
              if (scale.size() != 3 || bias.size() != 3)
                  throw std::invalid_argument("scale and bias take 3 values");
              if (boxes == 0 || boxes % 16 != 0)
                  throw std::invalid_argument("boxes must be 16-byte aligned");
              if (N < 1 || OH < 1 || OW < 1 || H < 1 || W < 1 ||
                  H > 32767 || W > 32767)
                  throw std::invalid_argument("resized_crop: bad sizes");
              launch_resized_crop((const void*)src, (void*)out,
                                  (const void*)boxes, N, H, W, OH, OW,
                                  scale.data(), bias.data(),
                                  as_stream(stream));
              check_last();
          });
    // Mixup / CutMix (csrc/mix.hip): the batch's mix row, int32 [8], then
    // the in-place blend or box swap that reads it
    m.def("batch_mix_draw",
          [](uintptr_t row, uintptr_t lam_table, uintptr_t sq_table,
             uintptr_t step_dev, int H, int W, uint64_t seed,
             uint32_t prob_thresh, uint32_t switch_thresh, bool mixup,
             bool cutmix, uintptr_t stream) {
              if (row == 0 || row % 16 != 0 || step_dev == 0)
                  throw std::invalid_argument(
                      "row must be 16-byte aligned, step_dev non-null");
              if ((mixup && lam_table == 0) || (cutmix && sq_table == 0))
                  throw std::invalid_argument(
                      "an enabled mode needs its table");
              if (H < 1 || W < 1 || H > 32767 || W > 32767)
                  throw std::invalid_argument("batch_mix_draw: bad sizes");
              launch_batch_mix_draw((void*)row, (const void*)lam_table,
                                    (const void*)sq_table,
                                    (const void*)step_dev, H, W, seed,
                                    prob_thresh, switch_thresh, mixup ? 1 : 0,
                                    cutmix ? 1 : 0, as_stream(stream));
              check_last();
          });
    m.def("batch_mix",
          [](uintptr_t x, uintptr_t row, int N, int H, int W, int C,
             uintptr_t stream) {
              if (x == 0 || x % 16 != 0 || row == 0 || row % 16 != 0)
                  throw std::invalid_argument(
                      "x and row must be 16-byte aligned");
              if (N < 1 || H < 1 || W < 1 || C < 1 || H > 32767 || W > 32767)
                  throw std::invalid_argument("batch_mix: bad sizes");
              launch_batch_mix((void*)x, (const void*)row, N, H, W, C,
                               as_stream(stream));
              check_last();
          });
    m.def("maxpool_fwd",
          [](uintptr_t x, uintptr_t y, uintptr_t argmax, int N, int H, int W,
             int C, int K, int R, int S, int Ho, int Wo, int stride, int pad,
             uintptr_t stream) {
              launch_maxpool_fwd((const void*)x, (void*)y, (void*)argmax,
                                 make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                 as_stream(stream));
              check_last();
          });
    m.def("maxpool_bwd",
          [](uintptr_t dy, uintptr_t argmax, uintptr_t dx, int N, int H, int W,
             int C, int K, int R, int S, int Ho, int Wo, int stride, int pad,
             uintptr_t stream) {
              launch_maxpool_bwd((const void*)dy, (const void*)argmax,
                                 (void*)dx,
                                 make_dims(N, H, W, C, K, R, S, Ho, Wo, stride, pad),
                                 as_stream(stream));
              check_last();
          });

    m.def("cross_entropy",
          [](uintptr_t logits, uintptr_t target, uintptr_t dlogits,
             uintptr_t loss_sum, int64_t B, int64_t C, float loss_scale,
             float grad_scale, bool is_bf16, uintptr_t stream) {
              launch_cross_entropy((const void*)logits, (const void*)target,
                                   (void*)dlogits, (void*)loss_sum, B, C,
                                   loss_scale, grad_scale, is_bf16 ? 1 : 0,
                                   as_stream(stream));
              check_last();
          });

    // target_b = 0: same as target; lam = 0 (null): 1
    m.def("cross_entropy_mix",
          [](uintptr_t logits, uintptr_t target, uintptr_t target_b,
             uintptr_t lam, uintptr_t dlogits, uintptr_t loss_sum, int64_t B,
             int64_t C, float eps, float loss_scale, float grad_scale,
             bool is_bf16, uintptr_t stream) {
              launch_cross_entropy_mix((const void*)logits,
                                       (const void*)target,
                                       (const void*)target_b,
                                       (const void*)lam, (void*)dlogits,
                                       (void*)loss_sum, B, C, eps, loss_scale,
                                       grad_scale, is_bf16 ? 1 : 0,
                                       as_stream(stream));
              check_last();
          });

    m.def("bce_logits",
          [](uintptr_t x, uintptr_t dx, uintptr_t loss_sum, int64_t n,
             float target, float loss_scale, float grad_scale, bool is_bf16,
             uintptr_t stream) {
              launch_bce_logits((const void*)x, (void*)dx, (void*)loss_sum, n,
                                target, loss_scale, grad_scale,
                                is_bf16 ? 1 : 0, as_stream(stream));
              check_last();
          });

    m.def("mse",
          [](uintptr_t x, uintptr_t t, uintptr_t dx, uintptr_t loss_sum,
             int64_t n, float loss_scale, float grad_scale, bool is_bf16,
             uintptr_t stream) {
              launch_mse((const void*)x, (const void*)t, (void*)dx,
                         (void*)loss_sum, n, loss_scale, grad_scale,
                         is_bf16 ? 1 : 0, as_stream(stream));
              check_last();
          });

    m.def("accuracy",
          [](uintptr_t logits, uintptr_t target, uintptr_t out, int64_t B,
             int64_t C, bool is_bf16, uintptr_t stream) {
              launch_accuracy((const void*)logits, (const void*)target,
                              (void*)out, B, C, is_bf16 ? 1 : 0,
                              as_stream(stream));
              check_last();
          });

    m.def("linear_fwd",
          [](uintptr_t x, uintptr_t w, uintptr_t b, uintptr_t y, int64_t B,
             int64_t I, int64_t O, uintptr_t stream) {
              launch_linear_fwd((const void*)x, (const void*)w,
                                (const void*)b, (void*)y, B, I, O,
                                as_stream(stream));
              check_last();
          });

    m.def("linear_dx",
          [](uintptr_t dy, uintptr_t w, uintptr_t dx, int64_t B, int64_t I,
             int64_t O, uintptr_t stream) {
              launch_linear_dx((const void*)dy, (const void*)w, (void*)dx, B,
                               I, O, as_stream(stream));
              check_last();
          });

    m.def("linear_dw",
          [](uintptr_t x, uintptr_t dy, uintptr_t dw, uintptr_t db, int64_t B,
             int64_t I, int64_t O, uintptr_t stream) {
              launch_linear_dw((const void*)x, (const void*)dy, (void*)dw,
                               (void*)db, B, I, O, as_stream(stream));
              check_last();
          });

    m.def("pool_fc_fwd",
          [](uintptr_t x, uintptr_t w, uintptr_t b, uintptr_t pooled,
             uintptr_t y, int N, int HW, int C, int O, uintptr_t stream) {
              launch_pool_fc_fwd((const void*)x, (const void*)w,
                                 (const void*)b, (void*)pooled, (void*)y, N,
                                 HW, C, O, as_stream(stream));
              check_last();
          });

    m.def("head_dw",
          [](uintptr_t pooled, uintptr_t dy, uintptr_t dw, uintptr_t db,
             int B, int C, int O, uintptr_t stream) {
              launch_head_dw((const void*)pooled, (const void*)dy, (void*)dw,
                             (void*)db, B, C, O, as_stream(stream));
              check_last();
          });

    m.def("head_dx",
          [](uintptr_t dy, uintptr_t w, uintptr_t dx, int N, int HW, int C,
             int O, uintptr_t stream) {
              launch_head_dx((const void*)dy, (const void*)w, (void*)dx, N,
                             HW, C, O, as_stream(stream));
              check_last();
          });
}

// optimizer_kernels_f32.h -- the optimizers' and the loss's kernels with float as the value type: the reference's Optimizer<float> /
// Loss<float> (what it instantiates without half precision).  ONE float weight vector -- with T = float the reference's `weights[i] = (T)w`
// is the identity and its trainer lets both pointers name the same buffer --, float gradients, float wrapper state.  The per-parameter
// arithmetic is that of the 16-bit kernels (adam_device.h, optimizer_device.h, loss_device.h), in the same fp32 order (build with
// -ffp-contract=off).  Buffers are device pointers over the whole parameter vector; [begin, end) selects the parameters of a call (begin a
// multiple of 4: a lane takes four consecutive floats, 16 bytes).
#pragma once
#include "elementwise_kernels.h"
#include "optimizer_kernels.h"

namespace tcnn_hip {

// optimizers/adam.h:48-127, 158-199 (adam_one); per-parameter step counters in the counter form.  current_step: the step AFTER the increment.
void adam_step_f32(hipStream_t stream, const AdamHyper& h, uint32_t n, uint32_t n_matrix_weights, float loss_scale, uint32_t current_step, float* weights,
                   const float* gradients, float* m1, float* m2, uint32_t* param_steps, uint32_t begin = 0, uint32_t end = 0xFFFFFFFFu);
// optimizers/sgd.h:44-69
void sgd_step_f32(hipStream_t stream, uint32_t n, float loss_scale, float learning_rate, float l2_reg, float* weights, const float* gradients, uint32_t begin = 0,
                  uint32_t end = 0xFFFFFFFFu);
// optimizers/novograd.h:45-90, 121-165: the two launches, the partial sums and the layer table of novograd_step (optimizer_kernels.h)
void novograd_step_f32(hipStream_t stream, NovogradLayers layers, const NovogradHyper& h, float loss_scale, bool first_step, float* weights, const float* gradients,
                       float* first_moments, const float* second_moments_in, float* second_moments_out, float* partials);
// optimizers/ema.h:45-141 (the average itself is fp32: no shadow copy)
void ema_step_f32(hipStream_t stream, uint32_t n, float ema_decay, uint32_t current_step, const float* weights, float* weights_ema, uint32_t begin = 0,
                  uint32_t end = 0xFFFFFFFFu);
// optimizers/lookahead.h:45-58: the weights and the slow weights both take slow * (1 - alpha) + weight * alpha
void lookahead_step_f32(hipStream_t stream, uint32_t n, float alpha, float* weights, float* weights_lookahead, uint32_t begin = 0, uint32_t end = 0xFFFFFFFFu);
// optimizers/average.h:45-58
void average_step_f32(hipStream_t stream, uint32_t n, uint32_t n_samples, const float* weights, float* weights_current_sample, float* weights_average,
                      uint32_t begin = 0, uint32_t end = 0xFFFFFFFFu);
// optimizers/batched.h:46-61, :84 (cast<float>: a copy of the pool for the nested optimizer)
void batched_accumulate_f32(hipStream_t stream, uint32_t n, bool first, uint32_t batch_size_multiplier, const float* gradients, float* pool, uint32_t begin = 0,
                            uint32_t end = 0xFFFFFFFFu);
void batched_cast_f32(hipStream_t stream, uint32_t n, const float* pool, float* gradients, uint32_t begin = 0, uint32_t end = 0xFFFFFFFFu);

// loss_evaluate (elementwise_kernels.h) with float prediction / gradients [n][stride]; values (may be null) fp32 [n][stride]
void loss_evaluate_f32(hipStream_t stream, LossType type, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale, const float* prediction, const float* target,
                       const float* data_pdf, float* values, float* gradients, uint32_t n_total);

}  // namespace tcnn_hip

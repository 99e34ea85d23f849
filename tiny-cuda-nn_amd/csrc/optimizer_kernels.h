// optimizer_kernels.h -- the streaming kernels of the optimizers besides Adam and Ema (those live in elementwise_kernels.h): SGD, Novograd,
// and the wrappers Lookahead, Average, Batched.  Each restates the reference's kernel operation by operation in the same fp32 order
// (build with -ffp-contract=off); reference lines are cited per function.  Buffers are device pointers over the whole parameter vector;
// [begin, end) selects the parameters of this call (begin a multiple of 8), as adam_step / ema_step do.
#pragma once
#include "tcnn_device.h"

namespace tcnn_hip {

// optimizers/sgd.h:44-69.  Every parameter is stepped (no matrix / non-matrix distinction, no skip of zero gradients).
void sgd_step(hipStream_t stream, uint32_t n, float loss_scale, float learning_rate, float l2_reg, float* weights_fp32, half_t* weights, const half_t* gradients,
              uint32_t begin = 0, uint32_t end = 0xFFFFFFFFu);

// optimizers/novograd.h:45-90, 121-165.  The layers are consecutive runs of the parameter vector ([begin[l], begin[l + 1])); parameters
// outside them are not touched.  Passed BY VALUE to both kernels (as the composite encoding's part table is).
constexpr uint32_t NOVOGRAD_MAX_LAYERS = 32;
constexpr uint32_t NOVOGRAD_REDUCE_BLOCKS = 16;  // partial sums per layer
struct NovogradLayers {
	uint32_t n_layers = 0;
	uint32_t begin[NOVOGRAD_MAX_LAYERS + 1] = {};        // in parameters
	uint32_t block_begin[NOVOGRAD_MAX_LAYERS + 1] = {};  // first workgroup of the step launch that works on the layer (set by novograd_step)
};
struct NovogradHyper {  // novograd.h:247-254 defaults
	float learning_rate = 1e-3f, beta1 = 0.9f, beta2 = 0.999f, epsilon = 1e-8f, relative_weight_decay = 0.0f, absolute_weight_decay = 0.0f;
};
// One optimizer step in two launches for all layers: (1) per layer, NOVOGRAD_REDUCE_BLOCKS partial sums of (float)g * (float)g into
// `partials` (n_layers * NOVOGRAD_REDUCE_BLOCKS floats), every sum in a fixed order; (2) the step: every workgroup adds its layer's
// partials in index order, forms the layer's new second moment from second_moments_in[layer] (novograd.h:84) and steps its weights with
// it; the layer's first workgroup stores the moment to second_moments_out[layer].  in / out are two buffers (the caller swaps them per
// step): a workgroup may still be reading the old moment when another one writes the new.  first_step: beta1 and beta2 enter as 0.
void novograd_step(hipStream_t stream, NovogradLayers layers, const NovogradHyper& h, float loss_scale, bool first_step, float* weights_fp32, half_t* weights,
                   const half_t* gradients, float* first_moments, const float* second_moments_in, float* second_moments_out, float* partials);

// optimizers/lookahead.h:45-58: slow <- slow * (1 - alpha) + master * alpha; master, the 16-bit weights and the slow weights all take it
void lookahead_step(hipStream_t stream, uint32_t n, float alpha, float* weights_fp32, half_t* weights, half_t* weights_lookahead, uint32_t begin = 0,
                    uint32_t end = 0xFFFFFFFFu);

// optimizers/average.h:45-58: average += (weight - sample) / n_samples through float, sample <- weight
void average_step(hipStream_t stream, uint32_t n, uint32_t n_samples, const half_t* weights, half_t* weights_current_sample, half_t* weights_average,
                  uint32_t begin = 0, uint32_t end = 0xFFFFFFFFu);

// optimizers/batched.h:46-61: pool (+)= (float)gradient / batch_size_multiplier (`first`: the pool restarts from 0)
void batched_accumulate(hipStream_t stream, uint32_t n, bool first, uint32_t batch_size_multiplier, const half_t* gradients, float* pool, uint32_t begin = 0,
                        uint32_t end = 0xFFFFFFFFu);
// batched.h:84 cast<T>: the pool as 16-bit gradients for the nested optimizer
void batched_cast(hipStream_t stream, uint32_t n, const float* pool, half_t* gradients, uint32_t begin = 0, uint32_t end = 0xFFFFFFFFu);

}  // namespace tcnn_hip

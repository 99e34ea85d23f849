// emu_driver_optimizers_f32.cpp -- csrc/optimizer_kernels_f32.hip (the optimizers' and the loss's kernels with float as the value type) on
// the host SIMT emulator, as a small library of its own (tests/emu/emu_optimizers_f32.py builds it with emu.py's compile and link
// commands); csrc/elementwise_kernels.hip rides along for make_adam_core and the 16-bit loss the fp32 one is compared with.
// TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#include "emu_driver.h"
#include "../../tiny-cuda-nn_amd/csrc/elementwise_kernels.hip"
#include "../../tiny-cuda-nn_amd/csrc/optimizer_kernels_f32.hip"

using namespace tcnn_hip;

#define EMU_EXPORT extern "C" __attribute__((visibility("default")))

// (the layout of emu.py's EmuAdam)
struct EmuAdamF32 {
	float learning_rate, beta1, beta2, epsilon, l2_reg, non_matrix_l2_reg, relative_weight_decay, absolute_weight_decay, weight_clipping_magnitude,
		gradient_clipping_magnitude, non_matrix_learning_rate_factor;
	int adabound, optimize_matrix_params, optimize_non_matrix_params, skip_zero_grad_non_matrix_params;
};

EMU_EXPORT int emuf_adam_step(const EmuAdamF32* e, uint32_t n, uint32_t n_matrix, float loss_scale, uint32_t current_step, float* weights, const float* gradients, float* m1,
                              float* m2, uint32_t* steps, uint32_t begin, uint32_t end) {
	return emu_call(__func__, [&] {
		AdamHyper h;
		h.learning_rate = e->learning_rate;
		h.beta1 = e->beta1;
		h.beta2 = e->beta2;
		h.epsilon = e->epsilon;
		h.l2_reg = e->l2_reg;
		h.non_matrix_l2_reg = e->non_matrix_l2_reg;
		h.relative_weight_decay = e->relative_weight_decay;
		h.absolute_weight_decay = e->absolute_weight_decay;
		h.weight_clipping_magnitude = e->weight_clipping_magnitude;
		h.gradient_clipping_magnitude = e->gradient_clipping_magnitude;
		h.non_matrix_learning_rate_factor = e->non_matrix_learning_rate_factor;
		h.adabound = e->adabound != 0;
		h.optimize_matrix_params = e->optimize_matrix_params != 0;
		h.optimize_non_matrix_params = e->optimize_non_matrix_params != 0;
		h.skip_zero_grad_non_matrix_params = e->skip_zero_grad_non_matrix_params != 0;
		adam_step_f32(nullptr, h, n, n_matrix, loss_scale, current_step, weights, gradients, m1, m2, steps, begin, end);
	});
}
EMU_EXPORT int emuf_sgd_step(uint32_t n, float loss_scale, float learning_rate, float l2_reg, float* weights, const float* gradients, uint32_t begin, uint32_t end) {
	return emu_call(__func__, [&] { sgd_step_f32(nullptr, n, loss_scale, learning_rate, l2_reg, weights, gradients, begin, end); });
}
// begins: n_layers + 1 ascending parameter offsets; hyper: {learning_rate, beta1, beta2, epsilon, relative_decay, absolute_decay};
// second_moments_in / _out: n_layers floats each; partials: n_layers * NOVOGRAD_REDUCE_BLOCKS floats
EMU_EXPORT int emuf_novograd_step(uint32_t n_layers, const uint32_t* begins, const float* hyper, float loss_scale, int first_step, float* weights, const float* gradients,
                                  float* first_moments, const float* second_moments_in, float* second_moments_out, float* partials) {
	return emu_call(__func__, [&]() -> int {
		if (n_layers > NOVOGRAD_MAX_LAYERS) return 2;
		NovogradLayers layers;
		layers.n_layers = n_layers;
		for (uint32_t l = 0; l <= n_layers; ++l) layers.begin[l] = begins[l];
		NovogradHyper h;
		h.learning_rate = hyper[0];
		h.beta1 = hyper[1];
		h.beta2 = hyper[2];
		h.epsilon = hyper[3];
		h.relative_weight_decay = hyper[4];
		h.absolute_weight_decay = hyper[5];
		novograd_step_f32(nullptr, layers, h, loss_scale, first_step != 0, weights, gradients, first_moments, second_moments_in, second_moments_out, partials);
		return 0;
	});
}
EMU_EXPORT uint32_t emuf_novograd_reduce_blocks(void) { return NOVOGRAD_REDUCE_BLOCKS; }
EMU_EXPORT int emuf_ema_step(uint32_t n, float decay, uint32_t current_step, const float* weights, float* weights_ema) {
	return emu_call(__func__, [&] { ema_step_f32(nullptr, n, decay, current_step, weights, weights_ema); });
}
EMU_EXPORT int emuf_lookahead_step(uint32_t n, float alpha, float* weights, float* weights_lookahead) {
	return emu_call(__func__, [&] { lookahead_step_f32(nullptr, n, alpha, weights, weights_lookahead); });
}
EMU_EXPORT int emuf_average_step(uint32_t n, uint32_t n_samples, const float* weights, float* weights_current_sample, float* weights_average) {
	return emu_call(__func__, [&] { average_step_f32(nullptr, n, n_samples, weights, weights_current_sample, weights_average); });
}
EMU_EXPORT int emuf_batched_accumulate(uint32_t n, int first, uint32_t batch_size_multiplier, const float* gradients, float* pool) {
	return emu_call(__func__, [&] { batched_accumulate_f32(nullptr, n, first != 0, batch_size_multiplier, gradients, pool); });
}
EMU_EXPORT int emuf_batched_cast(uint32_t n, const float* pool, float* gradients) {
	return emu_call(__func__, [&] { batched_cast_f32(nullptr, n, pool, gradients); });
}
EMU_EXPORT int emuf_loss(int loss_type, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale, const float* prediction, const float* target, const float* data_pdf,
                         float* values, float* gradients) {
	return emu_call(__func__, [&] { loss_evaluate_f32(nullptr, (LossType)loss_type, n, stride, dims, loss_scale, prediction, target, data_pdf, values, gradients, n * dims); });
}
// the 16-bit kernel on the same case (prediction / gradients: bit patterns of the build's 16-bit type)
EMU_EXPORT int emuf_loss_half(int loss_type, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale, const void* prediction, const float* target, const float* data_pdf,
                              float* values, void* gradients) {
	return emu_call(__func__, [&] {
		loss_evaluate(nullptr, (LossType)loss_type, n, stride, dims, loss_scale, (const half_t*)prediction, target, data_pdf, values, (half_t*)gradients, nullptr, n * dims);
	});
}

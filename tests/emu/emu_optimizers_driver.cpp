// emu_optimizers_driver.cpp -- the kernels of csrc/optimizer_kernels.hip (SGD, Novograd, Lookahead, Average, Batched) built for the host under
// the SIMT emulator (hip_emu.h), behind a flat C interface (host pointers only).  A library of its own next to emu_driver.cpp's.
// TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#define TCNN_HOST_EMU 1
#include "../../tiny-cuda-nn_amd/csrc/optimizer_kernels.hip"

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

int emuo_sgd_step(uint32_t n, float loss_scale, float learning_rate, float l2_reg, float* weights_fp32, void* weights, const void* gradients, uint32_t begin, uint32_t end) {
	try {
		sgd_step(nullptr, n, loss_scale, learning_rate, l2_reg, weights_fp32, (half_t*)weights, (const half_t*)gradients, begin, end);
	} catch (const std::exception&) {
		return 1;
	}
	return 0;
}
// begins: n_layers + 1 ascending parameter offsets; hyper: {learning_rate, beta1, beta2, epsilon, relative_decay, absolute_decay};
// second_moments_in / _out: n_layers floats each; partials: n_layers * NOVOGRAD_REDUCE_BLOCKS floats
int emuo_novograd_step(uint32_t n_layers, const uint32_t* begins, const float* hyper, float loss_scale, int first_step, float* weights_fp32, void* weights,
                       const void* gradients, float* first_moments, const float* second_moments_in, float* second_moments_out, float* partials) {
	try {
		if (n_layers > NOVOGRAD_MAX_LAYERS) return 2;
		NovogradLayers layers;
		layers.n_layers = n_layers;
		for (uint32_t l = 0; l <= n_layers; ++l) layers.begin[l] = begins[l];
		const NovogradHyper h = {hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5]};
		novograd_step(nullptr, layers, h, loss_scale, first_step != 0, weights_fp32, (half_t*)weights, (const half_t*)gradients, first_moments, second_moments_in,
		              second_moments_out, partials);
	} catch (const std::exception&) {
		return 1;
	}
	return 0;
}
uint32_t emuo_novograd_reduce_blocks(void) { return NOVOGRAD_REDUCE_BLOCKS; }
int emuo_lookahead_step(uint32_t n, float alpha, float* weights_fp32, void* weights, void* weights_lookahead) {
	lookahead_step(nullptr, n, alpha, weights_fp32, (half_t*)weights, (half_t*)weights_lookahead);
	return 0;
}
int emuo_average_step(uint32_t n, uint32_t n_samples, const void* weights, void* weights_current_sample, void* weights_average) {
	average_step(nullptr, n, n_samples, (const half_t*)weights, (half_t*)weights_current_sample, (half_t*)weights_average);
	return 0;
}
int emuo_batched_accumulate(uint32_t n, int first, uint32_t batch_size_multiplier, const void* gradients, float* pool) {
	batched_accumulate(nullptr, n, first != 0, batch_size_multiplier, (const half_t*)gradients, pool);
	return 0;
}
int emuo_batched_cast(uint32_t n, const float* pool, void* gradients) {
	batched_cast(nullptr, n, pool, (half_t*)gradients);
	return 0;
}

}  // extern "C"
#pragma GCC visibility pop

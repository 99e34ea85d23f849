// emu_driver_misc.cpp -- the rest of the emulator's driver (emu_driver.h): the elementwise kernels (loss, Adam, RNG, casts, the
// parameter-free encodings), csrc/composite_kernels.hip, csrc/optimizer_kernels.hip and the trainer snapshot
// (host-only code of the product: csrc/snapshot_msgpack.h).  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#include "emu_driver.h"
#include "../../tiny-cuda-nn_amd/csrc/elementwise_kernels.hip"
#include "../../tiny-cuda-nn_amd/csrc/composite_kernels.hip"
#include "../../tiny-cuda-nn_amd/csrc/optimizer_kernels.hip"
#include "../../tiny-cuda-nn_amd/csrc/snapshot_msgpack.h"

#include <cstring>
#include <vector>

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

// ---- elementwise kernels ------------------------------------------------------------------------------------------------------
int emu_loss(int type, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale, const uint16_t* prediction, const float* target,
             const float* data_pdf, float* values, uint16_t* gradients, float* loss_sum, uint32_t n_total) {
	std::vector<float> block_sums(loss_n_blocks(n, stride));
	std::vector<float> ws(1024);
	loss_evaluate(nullptr, (LossType)type, n, stride, dims, loss_scale, (const half_t*)prediction, target, data_pdf, values,
	              (half_t*)gradients, block_sums.data(), n_total);
	if (loss_sum) reduce_sum(nullptr, block_sums.data(), block_sums.size(), ws.data(), loss_sum);
	return 0;
}

struct EmuAdam {
	float learning_rate, beta1, beta2, epsilon, l2_reg, non_matrix_l2_reg, relative_weight_decay, absolute_weight_decay;
	float weight_clipping_magnitude, gradient_clipping_magnitude, non_matrix_learning_rate_factor;
	int adabound, optimize_matrix_params, optimize_non_matrix_params, skip_zero_grad_non_matrix_params;
};

int emu_adam_flip_steps(uint32_t n, uint32_t steps_done, uint32_t* steps) {
	adam_flip_step_representation(nullptr, n, steps_done, steps);
	return 0;
}

// any AdamStepsForm -> any other, in place (deficits8: n bytes, needed when the byte form is involved)
int emu_adam_convert_steps(uint32_t n, uint32_t steps_done, uint32_t* steps, uint8_t* deficits8, int from, int to) {
	adam_convert_step_representation(nullptr, n, steps_done, steps, deficits8, from, to);
	return 0;
}

// half_follows_master: AdamCore::half_follows_master of this call
int emu_adam_step(const EmuAdam* e, uint32_t n, uint32_t n_matrix, float loss_scale, uint32_t current_step, float* w32, uint16_t* w16,
                  const uint16_t* grads, float* m1, float* m2, uint32_t* steps, int steps_form, uint8_t* deficits8, int half_follows_master) {
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
	adam_step(nullptr, h, n, n_matrix, loss_scale, current_step, w32, (half_t*)w16, (half_t*)grads, m1, m2, steps, nullptr, nullptr, 0, 0xFFFFFFFFu,
	          steps_form, deficits8, half_follows_master != 0);
	return 0;
}

// rng state is passed in and written back
int emu_generate_random_uniform(uint64_t* state, uint64_t* inc, uint64_t n, float* out, float lower, float upper) {
	Pcg32 r;
	r.state = *state;
	r.inc = *inc;
	generate_random_uniform(nullptr, r, (size_t)n, out, lower, upper);
	*state = r.state;
	*inc = r.inc;
	return 0;
}

int emu_cast_f32_to_f16(uint64_t n, const float* in, uint16_t* out) {
	cast_f32_to_f16(nullptr, (size_t)n, in, (half_t*)out);
	return 0;
}

int emu_identity_forward(uint32_t n, uint32_t n_dims, uint32_t padded, const float* in, uint16_t* out_soa) {
	identity_forward(nullptr, n, n_dims, padded, 1.0f, 0.0f, in, n_dims, 1, (half_t*)out_soa, n, 1);
	return 0;
}

int emu_frequency_forward(uint32_t n, uint32_t n_dims, uint32_t n_frequencies, uint32_t padded, const float* in, uint16_t* out_soa) {
	frequency_forward(nullptr, n, n_dims, n_frequencies, padded, in, n_dims, 1, (half_t*)out_soa, n, 1);
	return 0;
}
int emu_frequency_backward(uint32_t n, uint32_t n_dims, uint32_t n_frequencies, const uint16_t* dL_dy_soa, const float* in, float* dL_dx) {
	frequency_backward(nullptr, n, n_dims, n_frequencies, (const half_t*)dL_dy_soa, n, 1, in, n_dims, 1, dL_dx, n_dims, 1);
	return 0;
}
// one-blob encoding: feature-major output (as the network consumes it) and dL/dinput
int emu_oneblob_forward(uint32_t n, uint32_t n_dims, uint32_t n_bins, uint32_t padded, const float* in, uint16_t* out_soa) {
	oneblob_forward(nullptr, n, n_dims, n_bins, padded, in, n_dims, 1, (half_t*)out_soa, n, 1);
	return 0;
}
int emu_oneblob_backward(uint32_t n, uint32_t n_dims, uint32_t n_bins, const uint16_t* dL_dy_soa, const float* in, float* dL_dx) {
	oneblob_backward(nullptr, n, n_dims, n_bins, (const half_t*)dL_dy_soa, n, 1, in, n_dims, 1, dL_dx, n_dims, 1);
	return 0;
}

int emu_trim_and_cast(uint32_t n, uint32_t padded, uint32_t dims, const uint16_t* in, float* out) {
	trim_and_cast(nullptr, n, padded, dims, (const half_t*)in, out, dims, 1);
	return 0;
}

// ---- csrc/composite_kernels.hip: triangle wave, the fused parameter-free parts of a Composite encoding, the Sum / Product reductions ----
// value matrices are feature-major [rows][n] when soa, sample-major [n][rows] otherwise; fp32: float values instead of the 16-bit type
int emuc_triangle_wave_forward(uint32_t n, uint32_t n_dims, uint32_t n_frequencies, uint32_t padded, const float* in, void* out, int soa, int fp32) {
	const uint32_t sk = soa ? n : 1u, si = soa ? 1u : padded;
	if (fp32) triangle_wave_forward(nullptr, n, n_dims, n_frequencies, padded, in, n_dims, 1, (float*)out, sk, si);
	else triangle_wave_forward(nullptr, n, n_dims, n_frequencies, padded, in, n_dims, 1, (half_t*)out, sk, si);
	return 0;
}
int emuc_triangle_wave_backward(uint32_t n, uint32_t n_dims, uint32_t n_frequencies, uint32_t padded, const void* dL_dy, int soa, int fp32, const float* in, float* dL_dx) {
	const uint32_t sk = soa ? n : 1u, si = soa ? 1u : padded;
	if (fp32) triangle_wave_backward(nullptr, n, n_dims, n_frequencies, (const float*)dL_dy, sk, si, in, n_dims, 1, dL_dx, n_dims, 1);
	else triangle_wave_backward(nullptr, n, n_dims, n_frequencies, (const half_t*)dL_dy, sk, si, in, n_dims, 1, dL_dx, n_dims, 1);
	return 0;
}
// table: n_parts rows of {kind, in_row, in_width, out_row, padded_width, param}
static EncodingParts make_parts(uint32_t n_parts, const uint32_t* table) {
	EncodingParts parts;
	for (uint32_t p = 0; p < n_parts; ++p) {
		const uint32_t* t = table + 6 * p;
		parts.add(EncodingPart{t[0], t[1], t[2], t[3], t[4], t[5], 1.0f, 0.0f});
	}
	return parts;
}
int emuc_parts_forward(uint32_t n_parts, const uint32_t* table, uint32_t n, uint32_t n_input_dims, uint32_t width, const float* in, void* out, int soa, int fp32) {
	const uint32_t sk = soa ? n : 1u, si = soa ? 1u : width;
	return emu_call(__func__, [&] {
		const EncodingParts parts = make_parts(n_parts, table);
		if (fp32) encoding_parts_forward(nullptr, parts, n, in, n_input_dims, 1, (float*)out, sk, si);
		else encoding_parts_forward(nullptr, parts, n, in, n_input_dims, 1, (half_t*)out, sk, si);
	});
}
int emuc_parts_backward(uint32_t n_parts, const uint32_t* table, uint32_t n, uint32_t n_input_dims, uint32_t width, const void* dL_dy, int soa, int fp32, const float* in,
                        float* dL_dx) {
	const uint32_t sk = soa ? n : 1u, si = soa ? 1u : width;
	return emu_call(__func__, [&] {
		const EncodingParts parts = make_parts(n_parts, table);
		if (fp32) encoding_parts_backward(nullptr, parts, n, n_input_dims, (const float*)dL_dy, sk, si, in, n_input_dims, 1, dL_dx, n_input_dims, 1);
		else encoding_parts_backward(nullptr, parts, n, n_input_dims, (const half_t*)dL_dy, sk, si, in, n_input_dims, 1, dL_dx, n_input_dims, 1);
	});
}
int emuc_reduce_forward(int product, uint32_t n, uint32_t width, uint32_t n_to_reduce, const void* to_reduce, void* reduced, int soa, int fp32) {
	const uint32_t sk = soa ? n : 1u;
	if (fp32) reduce_forward(nullptr, product != 0, n, width, n_to_reduce, (const float*)to_reduce, sk, soa ? 1u : width * n_to_reduce, (float*)reduced, sk, soa ? 1u : width);
	else reduce_forward(nullptr, product != 0, n, width, n_to_reduce, (const half_t*)to_reduce, sk, soa ? 1u : width * n_to_reduce, (half_t*)reduced, sk, soa ? 1u : width);
	return 0;
}
int emuc_reduce_backward(int product, uint32_t n, uint32_t width, uint32_t n_to_reduce, const void* to_reduce, void* dL_dunreduced, const void* dL_dreduced, int soa, int fp32) {
	const uint32_t sk = soa ? n : 1u;
	if (fp32) {
		reduce_backward(nullptr, product != 0, n, width, n_to_reduce, (const float*)to_reduce, (float*)dL_dunreduced, sk, soa ? 1u : width * n_to_reduce, (const float*)dL_dreduced, sk,
		                soa ? 1u : width);
	} else {
		reduce_backward(nullptr, product != 0, n, width, n_to_reduce, (const half_t*)to_reduce, (half_t*)dL_dunreduced, sk, soa ? 1u : width * n_to_reduce, (const half_t*)dL_dreduced,
		                sk, soa ? 1u : width);
	}
	return 0;
}

// ---- csrc/optimizer_kernels.hip: SGD, Novograd, Lookahead, Average, Batched ----------------------------------------------------------
int emuo_sgd_step(uint32_t n, float loss_scale, float learning_rate, float l2_reg, float* weights_fp32, void* weights, const void* gradients, uint32_t begin, uint32_t end) {
	return emu_call(__func__, [&] { sgd_step(nullptr, n, loss_scale, learning_rate, l2_reg, weights_fp32, (half_t*)weights, (const half_t*)gradients, begin, end); });
}
// begins: n_layers + 1 ascending parameter offsets; hyper: {learning_rate, beta1, beta2, epsilon, relative_decay, absolute_decay};
// second_moments_in / _out: n_layers floats each; partials: n_layers * NOVOGRAD_REDUCE_BLOCKS floats
int emuo_novograd_step(uint32_t n_layers, const uint32_t* begins, const float* hyper, float loss_scale, int first_step, float* weights_fp32, void* weights,
                       const void* gradients, float* first_moments, const float* second_moments_in, float* second_moments_out, float* partials) {
	return emu_call(__func__, [&]() -> int {
		if (n_layers > NOVOGRAD_MAX_LAYERS) return 2;
		NovogradLayers layers;
		layers.n_layers = n_layers;
		for (uint32_t l = 0; l <= n_layers; ++l) layers.begin[l] = begins[l];
		const NovogradHyper h = {hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5]};
		novograd_step(nullptr, layers, h, loss_scale, first_step != 0, weights_fp32, (half_t*)weights, (const half_t*)gradients, first_moments, second_moments_in,
		              second_moments_out, partials);
		return 0;
	});
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

// ---- trainer snapshot --------------------------------------------------------------------------------------------------------
// Encodes a snapshot from host arrays; returns the byte count (call with out == nullptr to size the buffer).
long emu_snapshot_encode(uint64_t n_params, const void* params_fp16, int with_optimizer, uint32_t current_step, float base_lr,
                         const float* m1, const float* m2, const uint32_t* steps, uint8_t* out, size_t capacity) {
	try {
		Snapshot s;
		s.n_params = n_params;
		s.params.data = (const uint8_t*)params_fp16;
		s.params.size = n_params * 2;
		s.has_optimizer = with_optimizer != 0;
		s.current_step = current_step;
		s.base_learning_rate = base_lr;
		s.first_moments.data = (const uint8_t*)m1; s.first_moments.size = n_params * 4;
		s.second_moments.data = (const uint8_t*)m2; s.second_moments.size = n_params * 4;
		s.param_steps.data = (const uint8_t*)steps; s.param_steps.size = n_params * 4;
		const size_t needed = snapshot_encoded_size(s);
		if (!out) return (long)needed;
		const std::vector<uint8_t> bytes = snapshot_encode(s);
		if (bytes.size() != needed || capacity < needed) return -2;
		std::memcpy(out, bytes.data(), bytes.size());
		return (long)needed;
	} catch (const std::exception&) { return -1; }
}

// Decodes; copies each blob into the caller's array when non-null.  meta = {n_params, has_optimizer, current_step,
// params_bytes, m1_bytes, m2_bytes, steps_bytes, params_is_float}.
int emu_snapshot_decode(const uint8_t* data, size_t size, uint64_t* meta, float* base_lr, void* params, void* m1, void* m2, void* steps) {
	try {
		const Snapshot s = snapshot_decode(data, size);
		meta[0] = s.n_params; meta[1] = s.has_optimizer; meta[2] = s.current_step; meta[3] = s.params.size;
		meta[4] = s.first_moments.size; meta[5] = s.second_moments.size; meta[6] = s.param_steps.size; meta[7] = s.params_type == "float";
		*base_lr = s.base_learning_rate;
		if (params) std::memcpy(params, s.params.data, s.params.size);
		if (m1 && s.first_moments.present()) std::memcpy(m1, s.first_moments.data, s.first_moments.size);
		if (m2 && s.second_moments.present()) std::memcpy(m2, s.second_moments.data, s.second_moments.size);
		if (steps && s.param_steps.present()) std::memcpy(steps, s.param_steps.data, s.param_steps.size);
		return 0;
	} catch (const std::exception&) { return -1; }
}

}  // extern "C"
#pragma GCC visibility pop

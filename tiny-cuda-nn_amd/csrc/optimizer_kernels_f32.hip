// optimizer_kernels_f32.hip -- see optimizer_kernels_f32.h.  Pure HBM streams in the shape of optimizer_kernels.hip: a lane takes 4
// consecutive parameters, reads each buffer with one 16-byte load, ISSUES EVERY LOAD BEFORE ITS FIRST STORE, computes in registers and
// stores 16 bytes at a time.  The last lane of a range (fewer than 4 parameters left) and calls whose buffers are not 16-byte aligned (a
// ring slot of the Average optimizer when the parameter count is no multiple of 4) take the scalar form of the same arithmetic.
// Build with -ffp-contract=off: every operation rounds as written.
#include "optimizer_kernels_f32.h"

#include <cmath>
#include <stdexcept>
#include <string>

#include "adam_device.h"
#include "optimizer_device.h"

namespace tcnn_hip {

constexpr uint32_t OKF_THREADS = 256;
constexpr uint32_t OKF_PER_LANE = 4;

static bool okf_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0u; }

// the parameter range of a call: clamps it, checks its start; false if it is empty
static bool okf_clamp_range(const char* what, uint32_t n, uint32_t& begin, uint32_t& end) {
	if (end > n) end = n;
	if (begin >= end) return false;
	if (begin % OKF_PER_LANE != 0u) throw std::runtime_error(std::string(what) + ": a parameter range must start at a multiple of 4");
	return true;
}
static dim3 okf_range_grid(uint32_t begin, uint32_t end) { return dim3(div_round_up(div_round_up(end - begin, OKF_PER_LANE), OKF_THREADS)); }

// ------------------------------------------------------------------------------------------ Adam
struct AdamArgsF32 : AdamCore {
	uint32_t begin, n_elements;  // parameters [begin, n_elements) are stepped (begin % 4 == 0)
};
// 16 B of gradients decide whether the state loads happen at all: a lane whose four parameters are all skipped (untouched hash-table
// entries, adam.h:79-82) reads nothing else.  A lane that steps some of its four stores all of them: the skipped ones keep the bits it loaded.
__global__ void __launch_bounds__(OKF_THREADS) k_adam_step_f32(const AdamArgsF32 a, uint32_t vec, float* __restrict__ weights, const float* __restrict__ gradients,
                                                               float* __restrict__ first_moments, float* __restrict__ second_moments,
                                                               uint32_t* __restrict__ param_steps) {
	const uint32_t i0 = a.begin + (blockIdx.x * OKF_THREADS + threadIdx.x) * OKF_PER_LANE;
	if (i0 >= a.n_elements) return;
	if (vec && i0 + OKF_PER_LANE <= a.n_elements) {
		const f4 g = *(const f4*)(gradients + i0);
		if (i0 >= a.n_matrix_weights && a.skip_zero_grad_non_matrix_params && g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f && g[3] == 0.0f) return;
		f4 w = *(const f4*)(weights + i0);
		f4 m1 = *(const f4*)(first_moments + i0);
		f4 m2 = *(const f4*)(second_moments + i0);
		u4 st = *(const u4*)(param_steps + i0);
		bool any = false;
#pragma unroll
		for (uint32_t j = 0; j < OKF_PER_LANE; ++j) {
			float wj = w[j], m1j = m1[j], m2j = m2[j];
			uint32_t sj = st[j];
			if (adam_one(a, i0 + j, g[j], wj, m1j, m2j, sj)) {
				w[j] = wj;
				m1[j] = m1j;
				m2[j] = m2j;
				st[j] = sj;
				any = true;
			}
		}
		if (!any) return;
		*(f4*)(weights + i0) = w;
		*(f4*)(first_moments + i0) = m1;
		*(f4*)(second_moments + i0) = m2;
		*(u4*)(param_steps + i0) = st;
	} else {
		for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, a.n_elements); ++i) {
			float wj = weights[i], m1j = first_moments[i], m2j = second_moments[i];
			uint32_t sj = param_steps[i];
			if (!adam_one(a, i, gradients[i], wj, m1j, m2j, sj)) continue;
			weights[i] = wj;
			first_moments[i] = m1j;
			second_moments[i] = m2j;
			param_steps[i] = sj;
		}
	}
}
void adam_step_f32(hipStream_t stream, const AdamHyper& h, uint32_t n, uint32_t n_matrix_weights, float loss_scale, uint32_t current_step, float* weights,
                   const float* gradients, float* m1, float* m2, uint32_t* param_steps, uint32_t begin, uint32_t end) {
	if (!okf_clamp_range("adam_step_f32", n, begin, end)) return;
	AdamArgsF32 a;
	(AdamCore&)a = make_adam_core(h, n_matrix_weights, loss_scale, current_step, ADAM_STEPS_COUNTERS);
	a.begin = begin;
	a.n_elements = end;
	const uint32_t vec = okf_aligned16(weights) && okf_aligned16(gradients) && okf_aligned16(m1) && okf_aligned16(m2) && okf_aligned16(param_steps);
	TCNN_LAUNCH(k_adam_step_f32, okf_range_grid(begin, end), dim3(OKF_THREADS), 0, stream, a, vec, weights, gradients, m1, m2, param_steps);
}

// ------------------------------------------------------------------------------------------ SGD
__global__ void __launch_bounds__(OKF_THREADS) k_sgd_step_f32(uint32_t begin, uint32_t end, uint32_t vec, float loss_scale, float learning_rate, float l2_reg,
                                                              float* __restrict__ weights, const float* __restrict__ gradients) {
	const uint32_t i0 = begin + (blockIdx.x * OKF_THREADS + threadIdx.x) * OKF_PER_LANE;
	if (i0 >= end) return;
	if (vec && i0 + OKF_PER_LANE <= end) {
		f4 w = *(const f4*)(weights + i0);
		const f4 g = *(const f4*)(gradients + i0);
#pragma unroll
		for (uint32_t j = 0; j < OKF_PER_LANE; ++j) w[j] = sgd_one(loss_scale, learning_rate, l2_reg, w[j], g[j]);
		*(f4*)(weights + i0) = w;
	} else {
		for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, end); ++i) weights[i] = sgd_one(loss_scale, learning_rate, l2_reg, weights[i], gradients[i]);
	}
}
void sgd_step_f32(hipStream_t stream, uint32_t n, float loss_scale, float learning_rate, float l2_reg, float* weights, const float* gradients, uint32_t begin,
                  uint32_t end) {
	if (!okf_clamp_range("sgd_step_f32", n, begin, end)) return;
	const uint32_t vec = okf_aligned16(weights) && okf_aligned16(gradients);
	TCNN_LAUNCH(k_sgd_step_f32, okf_range_grid(begin, end), dim3(OKF_THREADS), 0, stream, begin, end, vec, loss_scale, learning_rate, l2_reg, weights, gradients);
}

// ------------------------------------------------------------------------------------------ Novograd
// (1) partials[layer * NOVOGRAD_REDUCE_BLOCKS + x] = sum of g * g over the chunks x, x + NOVOGRAD_REDUCE_BLOCKS, ... of the layer (a chunk =
// 256 lanes x 4 gradients): every lane adds its chunks' squares in ascending order, the workgroup's 256 sums meet in a fixed tree -- the
// same bits on every run.
__global__ void __launch_bounds__(OKF_THREADS) k_novograd_reduce_f32(const NovogradLayers layers, uint32_t vec, const float* __restrict__ gradients,
                                                                     float* __restrict__ partials) {
	__shared__ float red[OKF_THREADS];
	const uint32_t layer = blockIdx.y;
	const uint32_t layer_begin = layers.begin[layer], layer_end = layers.begin[layer + 1];
	const bool vector = vec && layer_begin % OKF_PER_LANE == 0u;
	float s = 0.0f;
	for (uint32_t i0 = layer_begin + (blockIdx.x * OKF_THREADS + threadIdx.x) * OKF_PER_LANE; i0 < layer_end; i0 += NOVOGRAD_REDUCE_BLOCKS * OKF_THREADS * OKF_PER_LANE) {
		if (vector && i0 + OKF_PER_LANE <= layer_end) {
			const f4 g = *(const f4*)(gradients + i0);
#pragma unroll
			for (uint32_t j = 0; j < OKF_PER_LANE; ++j) s += g[j] * g[j];
		} else {
			for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, layer_end); ++i) s += gradients[i] * gradients[i];
		}
	}
	red[threadIdx.x] = s;
	__syncthreads();
	for (uint32_t k = OKF_THREADS / 2; k > 0; k >>= 1) {
		if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
		__syncthreads();
	}
	if (threadIdx.x == 0) partials[layer * NOVOGRAD_REDUCE_BLOCKS + blockIdx.x] = red[0];
}
// (2) the step of every layer: workgroups [block_begin[l], block_begin[l + 1]) work on layer l
__global__ void __launch_bounds__(OKF_THREADS) k_novograd_step_f32(const NovogradLayers layers, const NovogradArgs a, uint32_t vec, float* __restrict__ weights,
                                                                   const float* __restrict__ gradients, float* __restrict__ first_moments,
                                                                   const float* __restrict__ second_moments_in, float* __restrict__ second_moments_out,
                                                                   const float* __restrict__ partials) {
	uint32_t layer = 0;
	while (layer + 1u < layers.n_layers && blockIdx.x >= layers.block_begin[layer + 1]) ++layer;
	const uint32_t local_block = blockIdx.x - layers.block_begin[layer];
	const uint32_t layer_begin = layers.begin[layer], layer_end = layers.begin[layer + 1];
	// the layer's squared gradient norm: its partial sums in index order; then novograd.h:84
	float gradient_norm = 0.0f;
	for (uint32_t x = 0; x < NOVOGRAD_REDUCE_BLOCKS; ++x) gradient_norm += partials[layer * NOVOGRAD_REDUCE_BLOCKS + x];
	const float second_moment = novograd_second_moment(a, second_moments_in[layer], gradient_norm);
	if (local_block == 0 && threadIdx.x == 0) second_moments_out[layer] = second_moment;

	const uint32_t i0 = layer_begin + (local_block * OKF_THREADS + threadIdx.x) * OKF_PER_LANE;
	if (i0 >= layer_end) return;
	if (vec && layer_begin % OKF_PER_LANE == 0u && i0 + OKF_PER_LANE <= layer_end) {
		f4 w = *(const f4*)(weights + i0);
		f4 m = *(const f4*)(first_moments + i0);
		const f4 g = *(const f4*)(gradients + i0);
#pragma unroll
		for (uint32_t j = 0; j < OKF_PER_LANE; ++j) {
			float mj = m[j];
			w[j] = novograd_one(a, second_moment, w[j], g[j], mj);
			m[j] = mj;
		}
		*(f4*)(weights + i0) = w;
		*(f4*)(first_moments + i0) = m;
	} else {
		for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, layer_end); ++i) {
			float m = first_moments[i];
			const float new_weight = novograd_one(a, second_moment, weights[i], gradients[i], m);
			first_moments[i] = m;
			weights[i] = new_weight;
		}
	}
}
void novograd_step_f32(hipStream_t stream, NovogradLayers layers, const NovogradHyper& h, float loss_scale, bool first_step, float* weights, const float* gradients,
                       float* first_moments, const float* second_moments_in, float* second_moments_out, float* partials) {
	if (layers.n_layers == 0) return;
	if (layers.n_layers > NOVOGRAD_MAX_LAYERS) throw std::runtime_error("Novograd: more than " + std::to_string(NOVOGRAD_MAX_LAYERS) + " layers are not supported by this build");
	uint32_t blocks = 0;
	for (uint32_t l = 0; l < layers.n_layers; ++l) {
		if (layers.begin[l + 1] < layers.begin[l]) throw std::runtime_error("Novograd: layer table is not ascending");
		layers.block_begin[l] = blocks;
		blocks += div_round_up(div_round_up(layers.begin[l + 1] - layers.begin[l], OKF_PER_LANE), OKF_THREADS);
		if (layers.begin[l + 1] == layers.begin[l]) ++blocks;  // an empty layer still has a second moment to update
	}
	layers.block_begin[layers.n_layers] = blocks;
	const uint32_t vec = okf_aligned16(weights) && okf_aligned16(gradients) && okf_aligned16(first_moments);
	// novograd.h:143,154: the first step takes the gradient's own statistics ("set exact value on first step")
	const NovogradArgs a = {h.relative_weight_decay, h.absolute_weight_decay, loss_scale, h.learning_rate, first_step ? 0.0f : h.beta1, first_step ? 0.0f : h.beta2, h.epsilon};
	TCNN_LAUNCH(k_novograd_reduce_f32, dim3(NOVOGRAD_REDUCE_BLOCKS, layers.n_layers), dim3(OKF_THREADS), 0, stream, layers, vec, gradients, partials);
	TCNN_LAUNCH(k_novograd_step_f32, dim3(blocks), dim3(OKF_THREADS), 0, stream, layers, a, vec, weights, gradients, first_moments, second_moments_in, second_moments_out,
	            partials);
}

// ------------------------------------------------------------------------------------------ EMA of the weights
__global__ void __launch_bounds__(OKF_THREADS) k_ema_step_f32(uint32_t begin, uint32_t end, uint32_t vec, float ema_decay, float ema_debias_old, float ema_debias_new,
                                                              const float* __restrict__ weights, float* __restrict__ weights_ema) {
	const uint32_t i0 = begin + (blockIdx.x * OKF_THREADS + threadIdx.x) * OKF_PER_LANE;
	if (i0 >= end) return;
	if (vec && i0 + OKF_PER_LANE <= end) {
		const f4 w = *(const f4*)(weights + i0);
		f4 e = *(const f4*)(weights_ema + i0);
#pragma unroll
		for (uint32_t j = 0; j < OKF_PER_LANE; ++j) e[j] = ema_one(e[j], w[j], ema_decay, ema_debias_old, ema_debias_new);
		*(f4*)(weights_ema + i0) = e;
	} else {
		for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, end); ++i) weights_ema[i] = ema_one(weights_ema[i], weights[i], ema_decay, ema_debias_old, ema_debias_new);
	}
}
void ema_step_f32(hipStream_t stream, uint32_t n, float ema_decay, uint32_t current_step, const float* weights, float* weights_ema, uint32_t begin, uint32_t end) {
	if (!okf_clamp_range("ema_step_f32", n, begin, end)) return;
	// ema.h:113-114 (float pow through double, as std::pow(float, unsigned) does)
	const float ema_debias_old = 1 - (float)std::pow((double)ema_decay, (double)(current_step - 1));
	const float ema_debias_new = 1.0f / (1 - (float)std::pow((double)ema_decay, (double)current_step));
	const uint32_t vec = okf_aligned16(weights) && okf_aligned16(weights_ema);
	TCNN_LAUNCH(k_ema_step_f32, okf_range_grid(begin, end), dim3(OKF_THREADS), 0, stream, begin, end, vec, ema_decay, ema_debias_old, ema_debias_new, weights, weights_ema);
}

// ------------------------------------------------------------------------------------------ Lookahead
__global__ void __launch_bounds__(OKF_THREADS) k_lookahead_step_f32(uint32_t begin, uint32_t end, uint32_t vec, float alpha, float* __restrict__ weights,
                                                                    float* __restrict__ weights_lookahead) {
	const uint32_t i0 = begin + (blockIdx.x * OKF_THREADS + threadIdx.x) * OKF_PER_LANE;
	if (i0 >= end) return;
	if (vec && i0 + OKF_PER_LANE <= end) {
		f4 w = *(const f4*)(weights + i0);
		const f4 slow = *(const f4*)(weights_lookahead + i0);
#pragma unroll
		for (uint32_t j = 0; j < OKF_PER_LANE; ++j) w[j] = lookahead_one(alpha, slow[j], w[j]);
		*(f4*)(weights + i0) = w;
		*(f4*)(weights_lookahead + i0) = w;
	} else {
		for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, end); ++i) {
			const float new_weight = lookahead_one(alpha, weights_lookahead[i], weights[i]);
			weights_lookahead[i] = weights[i] = new_weight;
		}
	}
}
void lookahead_step_f32(hipStream_t stream, uint32_t n, float alpha, float* weights, float* weights_lookahead, uint32_t begin, uint32_t end) {
	if (!okf_clamp_range("lookahead_step_f32", n, begin, end)) return;
	const uint32_t vec = okf_aligned16(weights) && okf_aligned16(weights_lookahead);
	TCNN_LAUNCH(k_lookahead_step_f32, okf_range_grid(begin, end), dim3(OKF_THREADS), 0, stream, begin, end, vec, alpha, weights, weights_lookahead);
}

// ------------------------------------------------------------------------------------------ Average
__global__ void __launch_bounds__(OKF_THREADS) k_average_step_f32(uint32_t begin, uint32_t end, uint32_t vec, uint32_t n_samples, const float* __restrict__ weights,
                                                                  float* __restrict__ weights_current_sample, float* __restrict__ weights_average) {
	const uint32_t i0 = begin + (blockIdx.x * OKF_THREADS + threadIdx.x) * OKF_PER_LANE;
	if (i0 >= end) return;
	const float samples = (float)n_samples;  // `/ n_samples` with a uint32_t divisor converts it to float
	if (vec && i0 + OKF_PER_LANE <= end) {
		const f4 w = *(const f4*)(weights + i0);
		const f4 s = *(const f4*)(weights_current_sample + i0);
		f4 avg = *(const f4*)(weights_average + i0);
#pragma unroll
		for (uint32_t j = 0; j < OKF_PER_LANE; ++j) avg[j] = average_one<float>(samples, avg[j], w[j], s[j]);
		*(f4*)(weights_average + i0) = avg;
		*(f4*)(weights_current_sample + i0) = w;
	} else {
		for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, end); ++i) {
			const float weight = weights[i];
			weights_average[i] = average_one<float>(samples, weights_average[i], weight, weights_current_sample[i]);
			weights_current_sample[i] = weight;
		}
	}
}
void average_step_f32(hipStream_t stream, uint32_t n, uint32_t n_samples, const float* weights, float* weights_current_sample, float* weights_average, uint32_t begin,
                      uint32_t end) {
	if (!okf_clamp_range("average_step_f32", n, begin, end)) return;
	const uint32_t vec = okf_aligned16(weights) && okf_aligned16(weights_current_sample) && okf_aligned16(weights_average);
	TCNN_LAUNCH(k_average_step_f32, okf_range_grid(begin, end), dim3(OKF_THREADS), 0, stream, begin, end, vec, n_samples, weights, weights_current_sample, weights_average);
}

// ------------------------------------------------------------------------------------------ Batched
__global__ void __launch_bounds__(OKF_THREADS) k_batched_accumulate_f32(uint32_t begin, uint32_t end, uint32_t vec, uint32_t first, uint32_t batch_size_multiplier,
                                                                        const float* __restrict__ gradients, float* __restrict__ pool) {
	const uint32_t i0 = begin + (blockIdx.x * OKF_THREADS + threadIdx.x) * OKF_PER_LANE;
	if (i0 >= end) return;
	const float multiplier = (float)batch_size_multiplier;  // batched.h:60: float / uint32_t
	if (vec && i0 + OKF_PER_LANE <= end) {
		const f4 g = *(const f4*)(gradients + i0);
		f4 p = zero4();  // batched.h:56-58
		if (!first) p = *(const f4*)(pool + i0);
#pragma unroll
		for (uint32_t j = 0; j < OKF_PER_LANE; ++j) p[j] = batched_one(p[j], g[j], multiplier);
		*(f4*)(pool + i0) = p;
	} else {
		for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, end); ++i) pool[i] = batched_one(first ? 0.0f : pool[i], gradients[i], multiplier);
	}
}
void batched_accumulate_f32(hipStream_t stream, uint32_t n, bool first, uint32_t batch_size_multiplier, const float* gradients, float* pool, uint32_t begin, uint32_t end) {
	if (!okf_clamp_range("batched_accumulate_f32", n, begin, end)) return;
	const uint32_t vec = okf_aligned16(gradients) && okf_aligned16(pool);
	TCNN_LAUNCH(k_batched_accumulate_f32, okf_range_grid(begin, end), dim3(OKF_THREADS), 0, stream, begin, end, vec, first ? 1u : 0u, batch_size_multiplier, gradients, pool);
}

__global__ void __launch_bounds__(OKF_THREADS) k_batched_cast_f32(uint32_t begin, uint32_t end, uint32_t vec, const float* __restrict__ pool, float* __restrict__ gradients) {
	const uint32_t i0 = begin + (blockIdx.x * OKF_THREADS + threadIdx.x) * OKF_PER_LANE;
	if (i0 >= end) return;
	if (vec && i0 + OKF_PER_LANE <= end) {
		*(f4*)(gradients + i0) = *(const f4*)(pool + i0);
	} else {
		for (uint32_t i = i0; i < min(i0 + OKF_PER_LANE, end); ++i) gradients[i] = pool[i];
	}
}
void batched_cast_f32(hipStream_t stream, uint32_t n, const float* pool, float* gradients, uint32_t begin, uint32_t end) {
	if (!okf_clamp_range("batched_cast_f32", n, begin, end)) return;
	const uint32_t vec = okf_aligned16(pool) && okf_aligned16(gradients);
	TCNN_LAUNCH(k_batched_cast_f32, okf_range_grid(begin, end), dim3(OKF_THREADS), 0, stream, begin, end, vec, pool, gradients);
}

// ------------------------------------------------------------------------------------------ loss
// One thread per 4 consecutive elements of the [n][stride] float prediction matrix (16-byte accesses; stride a multiple of 8: a lane's
// four lie in one row).  The arithmetic is loss_device.h's with the gradient left in fp32.
__global__ void __launch_bounds__(OKF_THREADS) k_loss_f32(const LossType type, uint32_t n_groups, uint32_t stride, uint32_t dims, float loss_scale,
                                                          const float* __restrict__ predictions, const float* __restrict__ targets,
                                                          const float* __restrict__ data_pdf, float* __restrict__ values, float* __restrict__ gradients,
                                                          uint32_t n_total_u) {
	const uint32_t gidx = blockIdx.x * OKF_THREADS + threadIdx.x;
	if (gidx >= n_groups) return;
	const uint32_t e0 = gidx * OKF_PER_LANE;
	const uint32_t inter = e0 / stride, intra0 = e0 - inter * stride;
	const f4 p4 = *(const f4*)(predictions + e0);
	const float n_total = (float)n_total_u;
	float luminance = 0.0f;
	if (type == LossType::RelativeL2Luminance) {  // relative_l2_luminance.h:68-76: from the first 3 (dims >= 6: 3 + 3) outputs of the row
		const f4 lo = *(const f4*)(predictions + (size_t)inter * stride), hi = *(const f4*)(predictions + (size_t)inter * stride + 4);
		float r = lo[0], g = lo[1], b = lo[2];
		if (dims >= 6) {
			r += lo[3];
			g += hi[0];
			b += hi[1];
		}
		luminance = loss_row_luminance(r, g, b);
	}
	f4 g4 = zero4(), v4 = zero4();
#pragma unroll
	for (uint32_t j = 0; j < OKF_PER_LANE; ++j) {
		const uint32_t intra = intra0 + j;
		if (intra >= dims) continue;  // relative_l2.h:57-61
		const uint32_t target_idx = inter * dims + intra;
		const float pdf = data_pdf ? data_pdf[target_idx] : 1.0f;
		float value;
		g4[j] = type == LossType::RelativeL2Luminance ? loss_element_luminance<float>(p4[j], luminance, targets[target_idx], pdf, n_total, loss_scale, value)
		                                              : loss_element<true, float>(type, p4[j], targets[target_idx], pdf, n_total, loss_scale, value);
		v4[j] = value;
	}
	*(f4*)(gradients + e0) = g4;
	if (values) *(f4*)(values + e0) = v4;
}

void loss_evaluate_f32(hipStream_t stream, LossType type, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale, const float* prediction, const float* target,
                       const float* data_pdf, float* values, float* gradients, uint32_t n_total) {
	if (n == 0) return;
	if (stride % 8 != 0) throw std::runtime_error("loss: padded output width must be a multiple of 8");
	if (type == LossType::RelativeL2Luminance && dims < 3) throw std::runtime_error("RelativeL2Luminance needs at least 3 output dimensions");
	if (!okf_aligned16(prediction) || !okf_aligned16(gradients) || (values && !okf_aligned16(values))) throw std::runtime_error("loss: prediction, gradients and values must be 16-byte aligned");
	const uint32_t n_groups = n * stride / OKF_PER_LANE;
	TCNN_LAUNCH(k_loss_f32, dim3(div_round_up(n_groups, OKF_THREADS)), dim3(OKF_THREADS), 0, stream, type, n_groups, stride, dims, loss_scale, prediction, target, data_pdf,
	            values, gradients, n_total);
}

}  // namespace tcnn_hip

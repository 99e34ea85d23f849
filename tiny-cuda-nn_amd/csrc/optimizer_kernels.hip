// optimizer_kernels.hip -- see optimizer_kernels.h.  Pure HBM streams in k_ema_step's shape: a lane takes 8 consecutive parameters, reads each
// buffer with 16-byte loads (one for the 16-bit type, two for fp32), ISSUES EVERY LOAD BEFORE ITS FIRST STORE, computes in registers and
// stores 16 bytes at a time.  The last lane of a range (fewer than 8 parameters left) and calls whose buffers are not 16-byte aligned
// (a ring slot of the Average optimizer when the parameter count is no multiple of 8) take the scalar form of the same arithmetic.
// Build with -ffp-contract=off: every operation rounds as written.
#include "optimizer_kernels.h"
#include "optimizer_device.h"

#include <stdexcept>
#include <string>

namespace tcnn_hip {

constexpr uint32_t OK_THREADS = 256;
constexpr uint32_t OK_PER_LANE = 8;

// 8 consecutive floats through two 16-byte accesses
struct f8 {
	float v[8];
	TCNN_DEVICE float& operator[](uint32_t j) { return v[j]; }
	TCNN_DEVICE float operator[](uint32_t j) const { return v[j]; }
};
TCNN_DEVICE f8 load_f8(const float* p) {
	const f4 lo = *(const f4*)p, hi = *(const f4*)(p + 4);
	return {{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}};
}
TCNN_DEVICE void store_f8(float* p, const f8& x) {
	*(f4*)p = f4{x.v[0], x.v[1], x.v[2], x.v[3]};
	*(f4*)(p + 4) = f4{x.v[4], x.v[5], x.v[6], x.v[7]};
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0u; }

// the parameter range of a call: clamps it, checks its start; false if it is empty
static bool clamp_range(const char* what, uint32_t n, uint32_t& begin, uint32_t& end) {
	if (end > n) end = n;
	if (begin >= end) return false;
	if (begin % OK_PER_LANE != 0u) throw std::runtime_error(std::string(what) + ": a parameter range must start at a multiple of 8");
	return true;
}
static dim3 range_grid(uint32_t begin, uint32_t end) { return dim3(div_round_up(div_round_up(end - begin, OK_PER_LANE), OK_THREADS)); }

// ------------------------------------------------------------------------------------------ SGD
__global__ void __launch_bounds__(OK_THREADS) k_sgd_step(uint32_t begin, uint32_t end, uint32_t vec, float loss_scale, float learning_rate, float l2_reg,
                                                          float* __restrict__ weights_fp32, half_t* __restrict__ weights, const half_t* __restrict__ gradients) {
	const uint32_t i0 = begin + (blockIdx.x * OK_THREADS + threadIdx.x) * OK_PER_LANE;
	if (i0 >= end) return;
	if (vec && i0 + OK_PER_LANE <= end) {
		f8 w = load_f8(weights_fp32 + i0);
		const h8 g = *(const h8*)(gradients + i0);
		h8 wh;
#pragma unroll
		for (uint32_t j = 0; j < OK_PER_LANE; ++j) {
			w[j] = sgd_one(loss_scale, learning_rate, l2_reg, w[j], g[j]);
			wh[j] = to_half_rn(w[j]);
		}
		store_f8(weights_fp32 + i0, w);
		*(h8*)(weights + i0) = wh;
	} else {
		for (uint32_t i = i0; i < min(i0 + OK_PER_LANE, end); ++i) {
			const float new_weight = sgd_one(loss_scale, learning_rate, l2_reg, weights_fp32[i], gradients[i]);
			weights_fp32[i] = new_weight;
			weights[i] = to_half_rn(new_weight);
		}
	}
}
void sgd_step(hipStream_t stream, uint32_t n, float loss_scale, float learning_rate, float l2_reg, float* weights_fp32, half_t* weights, const half_t* gradients,
              uint32_t begin, uint32_t end) {
	if (!clamp_range("sgd_step", n, begin, end)) return;
	const uint32_t vec = aligned16(weights_fp32) && aligned16(weights) && aligned16(gradients);
	TCNN_LAUNCH(k_sgd_step, range_grid(begin, end), dim3(OK_THREADS), 0, stream, begin, end, vec, loss_scale, learning_rate, l2_reg, weights_fp32, weights, gradients);
}

// ------------------------------------------------------------------------------------------ Novograd
// (1) partials[layer * NOVOGRAD_REDUCE_BLOCKS + x] = sum of (float)g * (float)g over the chunks x, x + NOVOGRAD_REDUCE_BLOCKS, ... of the layer
// (a chunk = 256 lanes x 8 gradients): every lane adds its chunks' squares in ascending order, the workgroup's 256 sums meet in a fixed
// tree -- the same bits on every run.
__global__ void __launch_bounds__(OK_THREADS) k_novograd_reduce(const NovogradLayers layers, uint32_t vec, const half_t* __restrict__ gradients,
                                                                 float* __restrict__ partials) {
	__shared__ float red[OK_THREADS];
	const uint32_t layer = blockIdx.y;
	const uint32_t layer_begin = layers.begin[layer], layer_end = layers.begin[layer + 1];
	const bool vector = vec && layer_begin % OK_PER_LANE == 0u;
	float s = 0.0f;
	for (uint32_t i0 = layer_begin + (blockIdx.x * OK_THREADS + threadIdx.x) * OK_PER_LANE; i0 < layer_end; i0 += NOVOGRAD_REDUCE_BLOCKS * OK_THREADS * OK_PER_LANE) {
		if (vector && i0 + OK_PER_LANE <= layer_end) {
			const h8 g = *(const h8*)(gradients + i0);
#pragma unroll
			for (uint32_t j = 0; j < OK_PER_LANE; ++j) s += (float)g[j] * (float)g[j];
		} else {
			for (uint32_t i = i0; i < min(i0 + OK_PER_LANE, layer_end); ++i) s += (float)gradients[i] * (float)gradients[i];
		}
	}
	red[threadIdx.x] = s;
	__syncthreads();
	for (uint32_t k = OK_THREADS / 2; k > 0; k >>= 1) {
		if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
		__syncthreads();
	}
	if (threadIdx.x == 0) partials[layer * NOVOGRAD_REDUCE_BLOCKS + blockIdx.x] = red[0];
}

// (2) the step of every layer: workgroups [block_begin[l], block_begin[l + 1]) work on layer l
__global__ void __launch_bounds__(OK_THREADS) k_novograd_step(const NovogradLayers layers, const NovogradArgs a, uint32_t vec, float* __restrict__ weights_fp32,
                                                               half_t* __restrict__ weights, const half_t* __restrict__ gradients, float* __restrict__ first_moments,
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

	const uint32_t i0 = layer_begin + (local_block * OK_THREADS + threadIdx.x) * OK_PER_LANE;
	if (i0 >= layer_end) return;
	if (vec && layer_begin % OK_PER_LANE == 0u && i0 + OK_PER_LANE <= layer_end) {
		f8 w = load_f8(weights_fp32 + i0);
		f8 m = load_f8(first_moments + i0);
		const h8 g = *(const h8*)(gradients + i0);
		h8 wh;
#pragma unroll
		for (uint32_t j = 0; j < OK_PER_LANE; ++j) {
			w[j] = novograd_one(a, second_moment, w[j], g[j], m[j]);
			wh[j] = to_half_rn(w[j]);
		}
		store_f8(weights_fp32 + i0, w);
		store_f8(first_moments + i0, m);
		*(h8*)(weights + i0) = wh;
	} else {
		for (uint32_t i = i0; i < min(i0 + OK_PER_LANE, layer_end); ++i) {
			float m = first_moments[i];
			const float new_weight = novograd_one(a, second_moment, weights_fp32[i], gradients[i], m);
			first_moments[i] = m;
			weights_fp32[i] = new_weight;
			weights[i] = to_half_rn(new_weight);
		}
	}
}
void novograd_step(hipStream_t stream, NovogradLayers layers, const NovogradHyper& h, float loss_scale, bool first_step, float* weights_fp32, half_t* weights,
                   const half_t* gradients, float* first_moments, const float* second_moments_in, float* second_moments_out, float* partials) {
	if (layers.n_layers == 0) return;
	if (layers.n_layers > NOVOGRAD_MAX_LAYERS) throw std::runtime_error("Novograd: more than " + std::to_string(NOVOGRAD_MAX_LAYERS) + " layers are not supported by this build");
	uint32_t blocks = 0;
	for (uint32_t l = 0; l < layers.n_layers; ++l) {
		if (layers.begin[l + 1] < layers.begin[l]) throw std::runtime_error("Novograd: layer table is not ascending");
		layers.block_begin[l] = blocks;
		blocks += div_round_up(div_round_up(layers.begin[l + 1] - layers.begin[l], OK_PER_LANE), OK_THREADS);
		if (layers.begin[l + 1] == layers.begin[l]) ++blocks;  // an empty layer still has a second moment to update
	}
	layers.block_begin[layers.n_layers] = blocks;
	const uint32_t vec = aligned16(weights_fp32) && aligned16(weights) && aligned16(gradients) && aligned16(first_moments);
	// novograd.h:143,154: the first step takes the gradient's own statistics ("set exact value on first step")
	const NovogradArgs a = {h.relative_weight_decay, h.absolute_weight_decay, loss_scale, h.learning_rate, first_step ? 0.0f : h.beta1, first_step ? 0.0f : h.beta2, h.epsilon};
	TCNN_LAUNCH(k_novograd_reduce, dim3(NOVOGRAD_REDUCE_BLOCKS, layers.n_layers), dim3(OK_THREADS), 0, stream, layers, vec, gradients, partials);
	TCNN_LAUNCH(k_novograd_step, dim3(blocks), dim3(OK_THREADS), 0, stream, layers, a, vec, weights_fp32, weights, gradients, first_moments, second_moments_in,
	            second_moments_out, partials);
}

// ------------------------------------------------------------------------------------------ Lookahead
__global__ void __launch_bounds__(OK_THREADS) k_lookahead_step(uint32_t begin, uint32_t end, uint32_t vec, float alpha, float* __restrict__ weights_fp32,
                                                                half_t* __restrict__ weights, half_t* __restrict__ weights_lookahead) {
	const uint32_t i0 = begin + (blockIdx.x * OK_THREADS + threadIdx.x) * OK_PER_LANE;
	if (i0 >= end) return;
	if (vec && i0 + OK_PER_LANE <= end) {
		f8 w = load_f8(weights_fp32 + i0);
		h8 slow = *(const h8*)(weights_lookahead + i0);
#pragma unroll
		for (uint32_t j = 0; j < OK_PER_LANE; ++j) {
			w[j] = lookahead_one(alpha, slow[j], w[j]);
			slow[j] = to_half_rn(w[j]);
		}
		store_f8(weights_fp32 + i0, w);
		*(h8*)(weights + i0) = slow;
		*(h8*)(weights_lookahead + i0) = slow;
	} else {
		for (uint32_t i = i0; i < min(i0 + OK_PER_LANE, end); ++i) {
			const float new_weight = lookahead_one(alpha, weights_lookahead[i], weights_fp32[i]);
			weights_fp32[i] = new_weight;
			weights_lookahead[i] = weights[i] = to_half_rn(new_weight);
		}
	}
}
void lookahead_step(hipStream_t stream, uint32_t n, float alpha, float* weights_fp32, half_t* weights, half_t* weights_lookahead, uint32_t begin, uint32_t end) {
	if (!clamp_range("lookahead_step", n, begin, end)) return;
	const uint32_t vec = aligned16(weights_fp32) && aligned16(weights) && aligned16(weights_lookahead);
	TCNN_LAUNCH(k_lookahead_step, range_grid(begin, end), dim3(OK_THREADS), 0, stream, begin, end, vec, alpha, weights_fp32, weights, weights_lookahead);
}

// ------------------------------------------------------------------------------------------ Average
__global__ void __launch_bounds__(OK_THREADS) k_average_step(uint32_t begin, uint32_t end, uint32_t vec, uint32_t n_samples, const half_t* __restrict__ weights,
                                                              half_t* __restrict__ weights_current_sample, half_t* __restrict__ weights_average) {
	const uint32_t i0 = begin + (blockIdx.x * OK_THREADS + threadIdx.x) * OK_PER_LANE;
	if (i0 >= end) return;
	const float samples = (float)n_samples;  // `/ n_samples` with a uint32_t divisor converts it to float
	if (vec && i0 + OK_PER_LANE <= end) {
		const h8 w = *(const h8*)(weights + i0);
		const h8 s = *(const h8*)(weights_current_sample + i0);
		h8 avg = *(const h8*)(weights_average + i0);
#pragma unroll
		for (uint32_t j = 0; j < OK_PER_LANE; ++j) avg[j] = average_one(samples, avg[j], w[j], s[j]);
		*(h8*)(weights_average + i0) = avg;
		*(h8*)(weights_current_sample + i0) = w;
	} else {
		for (uint32_t i = i0; i < min(i0 + OK_PER_LANE, end); ++i) {
			const half_t weight = weights[i];
			weights_average[i] = average_one(samples, weights_average[i], weight, weights_current_sample[i]);
			weights_current_sample[i] = weight;
		}
	}
}
void average_step(hipStream_t stream, uint32_t n, uint32_t n_samples, const half_t* weights, half_t* weights_current_sample, half_t* weights_average, uint32_t begin,
                  uint32_t end) {
	if (!clamp_range("average_step", n, begin, end)) return;
	const uint32_t vec = aligned16(weights) && aligned16(weights_current_sample) && aligned16(weights_average);
	TCNN_LAUNCH(k_average_step, range_grid(begin, end), dim3(OK_THREADS), 0, stream, begin, end, vec, n_samples, weights, weights_current_sample, weights_average);
}

// ------------------------------------------------------------------------------------------ Batched
__global__ void __launch_bounds__(OK_THREADS) k_batched_accumulate(uint32_t begin, uint32_t end, uint32_t vec, uint32_t first, uint32_t batch_size_multiplier,
                                                                    const half_t* __restrict__ gradients, float* __restrict__ pool) {
	const uint32_t i0 = begin + (blockIdx.x * OK_THREADS + threadIdx.x) * OK_PER_LANE;
	if (i0 >= end) return;
	const float multiplier = (float)batch_size_multiplier;  // batched.h:60: float / uint32_t
	if (vec && i0 + OK_PER_LANE <= end) {
		const h8 g = *(const h8*)(gradients + i0);
		f8 p = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};  // batched.h:56-58
		if (!first) p = load_f8(pool + i0);
#pragma unroll
		for (uint32_t j = 0; j < OK_PER_LANE; ++j) p[j] = batched_one(p[j], g[j], multiplier);
		store_f8(pool + i0, p);
	} else {
		for (uint32_t i = i0; i < min(i0 + OK_PER_LANE, end); ++i) {
			float p = first ? 0.0f : pool[i];
			p = batched_one(p, gradients[i], multiplier);
			pool[i] = p;
		}
	}
}
void batched_accumulate(hipStream_t stream, uint32_t n, bool first, uint32_t batch_size_multiplier, const half_t* gradients, float* pool, uint32_t begin, uint32_t end) {
	if (!clamp_range("batched_accumulate", n, begin, end)) return;
	const uint32_t vec = aligned16(gradients) && aligned16(pool);
	TCNN_LAUNCH(k_batched_accumulate, range_grid(begin, end), dim3(OK_THREADS), 0, stream, begin, end, vec, first ? 1u : 0u, batch_size_multiplier, gradients, pool);
}

__global__ void __launch_bounds__(OK_THREADS) k_batched_cast(uint32_t begin, uint32_t end, uint32_t vec, const float* __restrict__ pool, half_t* __restrict__ gradients) {
	const uint32_t i0 = begin + (blockIdx.x * OK_THREADS + threadIdx.x) * OK_PER_LANE;
	if (i0 >= end) return;
	if (vec && i0 + OK_PER_LANE <= end) {
		const f8 p = load_f8(pool + i0);
		h8 g;
#pragma unroll
		for (uint32_t j = 0; j < OK_PER_LANE; ++j) g[j] = (half_t)p[j];
		*(h8*)(gradients + i0) = g;
	} else {
		for (uint32_t i = i0; i < min(i0 + OK_PER_LANE, end); ++i) gradients[i] = (half_t)pool[i];
	}
}
void batched_cast(hipStream_t stream, uint32_t n, const float* pool, half_t* gradients, uint32_t begin, uint32_t end) {
	if (!clamp_range("batched_cast", n, begin, end)) return;
	const uint32_t vec = aligned16(pool) && aligned16(gradients);
	TCNN_LAUNCH(k_batched_cast, range_grid(begin, end), dim3(OK_THREADS), 0, stream, begin, end, vec, pool, gradients);
}

}  // namespace tcnn_hip

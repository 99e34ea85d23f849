// mlp_general_fp32.hip -- the fp32 layer-by-layer network (mlp_kernels.h mlp_f32_*): Gen<float>, the entry points and the fp32 element-wise
// kernels over the templates of mlp_general_impl.h, which describes the kernels.  A unit of its own so that the library keeps one code
// object per precision.
#include "mlp_general_impl.h"

namespace tcnn_hip {

template <>
struct Gen<float> : GenTile<float> {
	typedef f4 vec;
	typedef f4 frag;
	typedef float operand;  // one k of the 16x16x4 shape: sample 4 q + (lane >> 4) of the weight-gradient kernel's step q
	static constexpr uint32_t MFMA_K = 4;
	static constexpr bool PRE_EPILOGUES = false;  // SiLU / Sine go through the general epilogues; forward saves the accumulator into P
	static TCNN_DEVICE vec zero() { return zero4(); }
	static TCNN_DEVICE operand part(vec v, uint32_t j) { return v[j]; }
	static TCNN_DEVICE f4 mfma(operand a, operand b, f4 c) { return mfma_16x16x4_f32(a, b, c); }
	static TCNN_DEVICE operand wg_samples(const float* image, uint32_t q, uint32_t wv, uint32_t b, uint32_t ld, uint32_t, uint32_t lr, uint32_t g) {
		return image[(4 * q + g) * ld + 32 * wv + 16 * b + lr];
	}
	static TCNN_DEVICE operand wg_samples_fm(const float* image, uint32_t q, uint32_t wv, uint32_t b, uint32_t ld, uint32_t, uint32_t lr, uint32_t g) {
		return image[(32 * wv + 16 * b + lr) * ld + 4 * q + g];
	}
	template <bool GENERAL>
	static TCNN_DEVICE frag forward(uint32_t act, f4 x) { return act32_forward4<GENERAL>(act, x); }
	template <bool GENERAL>
	static TCNN_DEVICE frag backward(uint32_t act, f4 v, frag at) { return act32_backward4<GENERAL>(act, v, at); }
	static TCNN_DEVICE frag narrow(f4 v) { return v; }
	static TCNN_DEVICE f4 widen(frag o) { return o; }
};

// ---- the fp32 entry points, and the fp32 network's element-wise kernels: one thread per value (n_params and n * padded_out are multiples
// of 256) ---------------------------------------------------------------------------------------------------------------------------
static void g32_check_shape(const MlpMeta& m, uint32_t n) {
	if (m.width % 16u != 0u || m.width == 0u || m.width > MLP_GENERAL_MAX_WIDTH || m.in_width % 16u != 0u || m.in_width == 0u || m.in_width > MLP_GENERAL_MAX_IN_WIDTH ||
	    m.padded_out % 16u != 0u || m.padded_out == 0u || m.padded_out > MLP_GENERAL_MAX_OUT_WIDTH) {
		throw std::runtime_error("mlp_f32: widths must be multiples of 16 within the layer-by-layer network's limits");
	}
	if (n % GEN_BN != 0u) throw std::runtime_error("mlp_f32: the batch size must be a multiple of 128");
}

void mlp_f32_forward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params, const float* input, float* hidden, float* output, const MlpF32Output& trimmed) {
	g32_check_shape(m, n);
	if (trimmed.out && (hidden || output)) throw std::runtime_error("mlp_f32_forward: the trimmed output is for inference, in place of the padded one");
	if (trimmed.out && (trimmed.dims == 0 || trimmed.dims > m.padded_out)) throw std::runtime_error("mlp_f32_forward: the trimmed output has at most padded_out columns");
	gen_forward<float>(stream, m, n, params, input, hidden, output, trimmed);
}
uint32_t mlp_f32_n_partials(const MlpMeta& m, uint32_t n) { return gen_n_partials<float>(m, n); }
size_t mlp_f32_backward_workspace_bytes(const MlpMeta& m, uint32_t n) { return gen_backward_workspace_bytes<float>(m, n); }
void mlp_f32_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params_t, const float* input, const float* hidden, const float* dL_doutput,
                      float* dL_dinput, float* partials, void* workspace) {
	g32_check_shape(m, n);
	if (!workspace) throw std::runtime_error("mlp_f32_backward: a workspace is required (mlp_f32_backward_workspace_bytes)");
	if (!hidden) throw std::runtime_error("mlp_f32_backward: the saved activations of the forward pass are required");
	gen_backward<float>(stream, m, n, params_t, input, hidden, dL_doutput, dL_dinput, partials, workspace);
}

__global__ void __launch_bounds__(GEN_THREADS) k_mlp_f32_finalize(uint32_t n_params, uint32_t n_partials, const float* partials, float* grads, uint32_t accumulate) {
	const uint32_t i = blockIdx.x * GEN_THREADS + threadIdx.x;
	if (i >= n_params) return;
	float s = partials[i];
	for (uint32_t b = 1; b < n_partials; ++b) s += partials[(size_t)b * n_params + i];
	grads[i] = accumulate ? grads[i] + s : s;
}
__global__ void __launch_bounds__(GEN_THREADS) k_mlp_f32_transpose(const MlpMeta m, const float* params, float* params_t) {
	const uint32_t i = blockIdx.x * GEN_THREADS + threadIdx.x;
	if (i < m.n_params()) params_t[mlp_transposed_index(m, i)] = params[i];
}
__global__ void __launch_bounds__(GEN_THREADS) k_mlp_f32_output_activation_backward(uint32_t n_fragments, uint32_t act, const float* output, const float* dL_doutput, float* dL_dpreact) {
	const uint32_t i = blockIdx.x * GEN_THREADS + threadIdx.x;
	if (i >= n_fragments) return;
	const f4 y = *(const f4*)(output + 4 * (size_t)i), v = *(const f4*)(dL_doutput + 4 * (size_t)i);
	f4 o = act32_backward4_general(act, v, y);
	*(f4*)(dL_dpreact + 4 * (size_t)i) = o;
}

void mlp_f32_transpose_weights(hipStream_t stream, const MlpMeta& m, const float* params, float* params_t) {
	TCNN_LAUNCH(k_mlp_f32_transpose, dim3(div_round_up(m.n_params(), GEN_THREADS)), dim3(GEN_THREADS), 0, stream, m, params, params_t);
}

void mlp_f32_output_activation_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* output, const float* dL_doutput, float* dL_dpreact) {
	const uint64_t fragments = (uint64_t)n * m.padded_out / 4u;
	if (fragments > 0xFFFFFFFFull) throw std::runtime_error("mlp_f32_output_activation_backward: the batch is too large; split it");
	if (fragments == 0) return;
	TCNN_LAUNCH(k_mlp_f32_output_activation_backward, dim3(div_round_up((uint32_t)fragments, GEN_THREADS)), dim3(GEN_THREADS), 0, stream, (uint32_t)fragments,
	            m.output_activation, output, dL_doutput, dL_dpreact);
}

void mlp_f32_finalize_gradients(hipStream_t stream, const MlpMeta& m, uint32_t n_partials, const float* partials, float* grads, bool accumulate) {
	if (n_partials == 0) throw std::runtime_error("mlp_f32_finalize_gradients: no slabs");
	TCNN_LAUNCH(k_mlp_f32_finalize, dim3(div_round_up(m.n_params(), GEN_THREADS)), dim3(GEN_THREADS), 0, stream, m.n_params(), n_partials, partials, grads,
	            accumulate ? 1u : 0u);
}

}  // namespace tcnn_hip

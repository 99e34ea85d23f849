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
	// GEN_EPI_CURVATURE: acc * act'(at) + e * t * act''(at), for the activations with a second derivative
	static TCNN_DEVICE frag curvature(uint32_t act, f4 acc, frag e, frag t, frag at) {
		const f4 first = act32_backward4<true>(act, acc, at);
		f4 et;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) et[j] = e[j] * t[j];
		const f4 second = act32_second4_general(act, et, at);
		f4 o;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) o[j] = first[j] + second[j];
		return o;
	}
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

// ---- the second-order pass (mlp_kernels.h mlp_f32_backward_backward).  Names as in gen_backward, with x the padded encoded input, v the
// incoming dL/d(dL/dinput) padded with zeros, dy the caller's dL/doutput:
//   forward      p_j = W_j a_{j-1}, a_j = act(p_j), y = out_act(W_out a_last)
//   first order  g = dy * out_act'(y), e_j = W_{j+1}^T d_{j+1} (e_last = W_out^T g), d_j = e_j * act'(p_j), dx = W_0^T d_0
//   tangent      t_0 = W_0 v, u_j = t_j * act'(p_j), t_{j+1} = W_{j+1} u_j, t_out = W_out u_last;   dL/d(dy) = t_out * out_act'(y)
//   curvature    c_out = dy * out_act''(y) * t_out, c_j = e_j * t_j * act''(p_j) + (W_{j+1}^T c_{j+1}) * act'(p_j);   dL/dx = W_0^T c_0
//   weights      dW_j = sum_s (d_j (x) u_{j-1} + c_j (x) a_{j-1}) with u_{-1} = v, dW_out = sum_s (g (x) u_last + c_out (x) a_last)
// t / u and e / d come out of ONE launch per layer each (GEN_EPI_DERIVATIVE_RAW, forward resp. transposed weights), c_j out of one
// (GEN_EPI_CURVATURE, written over e_j), each weight matrix out of one (k_mlp_general_wgrad<.., DUAL>).  The caller's `output` is not at
// hand (the C ABI does not pass it): y is the forward pass's last product again, from the saved a_last -- the same launch, the same bits.
// Where both activations are piecewise linear every c is zero: no curvature launches, dL/dx is zeros, the weight gradients are the d (x) u
// products alone.  Where only the hidden one is, c_j = (W^T c_{j+1}) * act'(p_j) is the first-order epilogue (GEN_EPI_BACKWARD).
__global__ void __launch_bounds__(GEN_THREADS) k_mlp_f32_output_curvature(uint32_t n_fragments, uint32_t act, const float* output, const float* dL_doutput, float* t_out) {
	const uint32_t i = blockIdx.x * GEN_THREADS + threadIdx.x;
	if (i >= n_fragments) return;
	const f4 y = *(const f4*)(output + 4 * (size_t)i), v = *(const f4*)(dL_doutput + 4 * (size_t)i), t = *(const f4*)(t_out + 4 * (size_t)i);
	f4 vt;
#pragma unroll
	for (uint32_t j = 0; j < 4; ++j) vt[j] = v[j] * t[j];
	const f4 o = act32_second4_general(act, vt, y);
	*(f4*)(t_out + 4 * (size_t)i) = o;  // c_out over t_out
}

bool mlp_f32_second_order_has_curvature(const MlpMeta& m) { return !act_second_derivative_is_zero(m.activation) || !act_second_derivative_is_zero(m.output_activation); }

// floats per sample: u and d of every hidden layer, y and g; with curvature also t, e (c over it) and t_out (c_out over it)
size_t mlp_f32_backward_backward_workspace_bytes(const MlpMeta& m, uint32_t n) {
	const size_t layers = m.n_hidden_matmuls + 1u, curvature = mlp_f32_second_order_has_curvature(m) ? 1u : 0u;
	return ((2u + 2u * curvature) * layers * m.width + (2u + curvature) * m.padded_out) * (size_t)n * sizeof(float);
}

static void g32_memset(hipStream_t stream, float* p, size_t count) {
	if (hipMemsetAsync(p, 0, count * sizeof(float), stream) != hipSuccess) throw std::runtime_error("mlp_f32_backward_backward: memset failed");
}

void mlp_f32_backward_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params, const float* params_t, const float* input, const float* hidden,
                               const float* v, const float* dL_doutput, float* dL_ddLdoutput, float* dL_dinput, float* partials, void* workspace) {
	g32_check_shape(m, n);
	if (!workspace) throw std::runtime_error("mlp_f32_backward_backward: a workspace is required (mlp_f32_backward_backward_workspace_bytes)");
	if (!hidden || !input || !v || !params) throw std::runtime_error("mlp_f32_backward_backward: the saved activations, the encoded input, v and the parameters are required");
	const uint32_t W = m.width, IN = m.in_width, HM = m.n_hidden_matmuls, OUTP = m.padded_out, L = HM + 1u;
	const uint32_t act = m.activation, out_act = m.output_activation, none = (uint32_t)Activation::None;
	const size_t LW = (size_t)n * W, LO = (size_t)n * OUTP;
	const bool hidden_curves = !act_second_derivative_is_zero(act), output_curves = !act_second_derivative_is_zero(out_act);
	const bool curvature = (hidden_curves || output_curves) && (partials || dL_dinput);
	const bool tangent = dL_ddLdoutput || partials || curvature, first_order = partials || curvature;
	if (first_order && (!dL_doutput || !params_t)) throw std::runtime_error("mlp_f32_backward_backward: dL_doutput and the transposed parameters are required");
	if (!tangent && !first_order) {
		if (dL_dinput) g32_memset(stream, dL_dinput, (size_t)IN * n);
		return;
	}

	float* U = (float*)workspace;   // [L][n][W]
	float* D = U + L * LW;          // [L][n][W]
	float* y = D + L * LW;          // [n][OUTP]
	float* g_buf = y + LO;          // [n][OUTP]
	float* T = g_buf + LO;          // [L][n][W]      (curvature only, like the two below)
	float* E = T + L * LW;          // [L][n][W]      e_j, then c_j
	float* t_out = E + L * LW;      // [n][OUTP]      t_out, then c_out
	const float* w_in = params;                             // [W][IN]
	const float* w_hid = w_in + (size_t)W * IN;             // HM x [W][W]
	const float* w_out = w_hid + (size_t)HM * W * W;        // [OUTP][W]
	const float* wt_in = params_t;                          // [IN][W]
	const float* wt_hid = params_t ? wt_in + (size_t)IN * W : nullptr;
	const float* wt_out = params_t ? wt_hid + (size_t)HM * W * W : nullptr;  // [W][OUTP]
	const float* at = act_needs_preactivation(act) ? hidden + L * LW : hidden;  // where the hidden activation's derivatives are taken
	const float* a_last = hidden + HM * LW;

	auto layer = [](const float* Wm, uint32_t M, uint32_t K, const float* X, float* Y, uint32_t n_, uint32_t act_, const float* F, float* P, const float* Ev, const float* Tv) {
		return GenLayerArgs<float>{n_, M, K, Wm, X, K, Y, M, F, M, act_, P, nullptr, 0u, 0u, 0u, 0u, Ev, Tv};
	};
	if (out_act != none) {  // y, as the forward pass computed it
		gen_launch_layer<float, GEN_EPI_FORWARD, false, false>(stream, layer(w_out, OUTP, W, a_last, y, n, out_act, nullptr, nullptr, nullptr, nullptr));
	}
	if (tangent) {
		const bool keep_t = curvature && hidden_curves;
		gen_launch_layer<float, GEN_EPI_DERIVATIVE_RAW, true, false>(stream, layer(w_in, W, IN, v, U, n, act, at, keep_t ? T : nullptr, nullptr, nullptr));
		for (uint32_t j = 1; j <= HM; ++j) {
			gen_launch_layer<float, GEN_EPI_DERIVATIVE_RAW, false, false>(
				stream, layer(w_hid + (size_t)(j - 1) * W * W, W, W, U + (j - 1) * LW, U + j * LW, n, act, at + j * LW, keep_t ? T + j * LW : nullptr, nullptr, nullptr));
		}
		const bool keep_t_out = curvature && output_curves;
		if (dL_ddLdoutput && out_act != none) {
			gen_launch_layer<float, GEN_EPI_DERIVATIVE_RAW, false, false>(stream, layer(w_out, OUTP, W, U + HM * LW, dL_ddLdoutput, n, out_act, y, keep_t_out ? t_out : nullptr, nullptr, nullptr));
		} else if (dL_ddLdoutput || keep_t_out) {  // (no output activation: nothing curves there, t_out is the result itself)
			gen_launch_layer<float, GEN_EPI_NONE, false, false>(stream, layer(w_out, OUTP, W, U + HM * LW, dL_ddLdoutput ? dL_ddLdoutput : t_out, n, none, nullptr, nullptr, nullptr, nullptr));
		}
	}
	const float* g = dL_doutput;
	if (first_order) {
		if (out_act != none) {
			mlp_f32_output_activation_backward(stream, m, n, y, dL_doutput, g_buf);
			g = g_buf;
		}
		const bool keep_e = curvature && hidden_curves;
		gen_launch_layer<float, GEN_EPI_DERIVATIVE_RAW, false, false>(stream, layer(wt_out, W, OUTP, g, D + HM * LW, n, act, at + HM * LW, keep_e ? E + HM * LW : nullptr, nullptr, nullptr));
		for (uint32_t j = HM; j-- > 0;) {
			gen_launch_layer<float, GEN_EPI_DERIVATIVE_RAW, false, false>(
				stream, layer(wt_hid + (size_t)j * W * W, W, W, D + (j + 1) * LW, D + j * LW, n, act, at + j * LW, keep_e ? E + j * LW : nullptr, nullptr, nullptr));
		}
	}
	if (curvature) {
		if (output_curves) {
			const uint64_t fragments = (uint64_t)LO / 4u;
			if (fragments > 0xFFFFFFFFull) throw std::runtime_error("mlp_f32_backward_backward: the batch is too large; split it");
			TCNN_LAUNCH(k_mlp_f32_output_curvature, dim3(div_round_up((uint32_t)fragments, GEN_THREADS)), dim3(GEN_THREADS), 0, stream, (uint32_t)fragments, out_act, y, dL_doutput, t_out);
		} else {
			g32_memset(stream, t_out, LO);
		}
		auto curvature_layer = [&](uint32_t K, const float* wt, const float* x, uint32_t j) {
			float* c = E + j * LW;
			if (hidden_curves) {
				gen_launch_layer<float, GEN_EPI_CURVATURE, false, false>(stream, layer(wt, W, K, x, c, n, act, at + j * LW, nullptr, c, T + j * LW));
			} else {
				gen_launch_layer<float, GEN_EPI_BACKWARD, false, false>(stream, layer(wt, W, K, x, c, n, act, at + j * LW, nullptr, nullptr, nullptr));
			}
		};
		curvature_layer(OUTP, wt_out, t_out, HM);
		for (uint32_t j = HM; j-- > 0;) curvature_layer(W, wt_hid + (size_t)j * W * W, E + (j + 1) * LW, j);
		if (dL_dinput) {
			GenLayerArgs<float> a = layer(wt_in, IN, W, E, dL_dinput, n, none, nullptr, nullptr, nullptr, nullptr);
			a.ldy = 0u;
			gen_launch_layer<float, GEN_EPI_NONE, false, true>(stream, a);
		}
	} else if (dL_dinput) {
		g32_memset(stream, dL_dinput, (size_t)IN * n);
	}
	if (!partials) return;

	const uint32_t n_slices = gen_n_partials<float>(m, n);
	const size_t slab = m.n_params(), off_hid = (size_t)W * IN, off_out = off_hid + (size_t)HM * W * W;
	const uint32_t lds_bytes = 2u * Gen<float>::WG_STAGE * (uint32_t)sizeof(float);
	auto product = [&](uint32_t WO, uint32_t WI, const float* d, const float* a, const float* d2, const float* a2, bool a_fm, size_t offset) {
		const GenWgradArgs<float> p = {n, WO, WI, d, WO, a, a_fm ? 0u : WI, partials, slab, offset, n_slices};
		GenWgradDualArgs<float> p2;
		(GenWgradArgs<float>&)p2 = p;
		p2.d2 = d2;
		p2.a2 = a2;
		const dim3 grid(gen_wgrad_tiles(WO, WI) * n_slices), block(GEN_THREADS);
		if (a_fm && d2) {
			TCNN_LAUNCH((k_mlp_general_wgrad<float, true, GenWgradDualArgs<float>>), grid, block, lds_bytes, stream, p2);
		} else if (a_fm) {
			TCNN_LAUNCH((k_mlp_general_wgrad<float, true>), grid, block, lds_bytes, stream, p);
		} else if (d2) {
			TCNN_LAUNCH((k_mlp_general_wgrad<float, false, GenWgradDualArgs<float>>), grid, block, lds_bytes, stream, p2);
		} else {
			TCNN_LAUNCH((k_mlp_general_wgrad<float, false>), grid, block, lds_bytes, stream, p);
		}
	};
	const bool out_pair = curvature && output_curves;  // (otherwise c_out is zero)
	product(OUTP, W, g, U + HM * LW, out_pair ? t_out : nullptr, out_pair ? a_last : nullptr, false, off_out);
	for (uint32_t j = 0; j < HM; ++j) {
		product(W, W, D + (j + 1) * LW, U + j * LW, curvature ? E + (j + 1) * LW : nullptr, curvature ? hidden + j * LW : nullptr, false, off_hid + (size_t)j * W * W);
	}
	product(W, IN, D, v, curvature ? E : nullptr, curvature ? input : nullptr, true, 0);
}

}  // namespace tcnn_hip

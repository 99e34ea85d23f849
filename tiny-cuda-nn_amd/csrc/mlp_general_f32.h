// mlp_general_f32.h -- the layer-by-layer network in fp32 (mlp_general_f32.hip): weights, activations, dL_dinput and weight gradients are
// float, the products run on the fp32 MFMA (v_mfma_f32_16x16x4_f32).  Where the reference built without half precision runs its CutlassMLP
// in fp32 (network_precision_t = float, network.cu:51-138) -- here a per-module choice (tcnn_create_network_precision).
// Same parameter layout ([W][IN] | HM x [W][W] | [OUTP][W], row-major, MlpMeta::n_params), transposed scratch (mlp_transposed_index) and
// boundary layouts as the 16-bit networks (mlp_kernels.h):
//   input / dL_dinput  : float, feature-major [in_width][n]
//   output / dL_doutput: float, sample-major  [n][padded_out]
//   hidden (saved)     : float, [n_hidden][n][W] post-activations; SiLU / Sine: followed by the pre-activations (mlp_f32_saved_activation_bytes)
// Every hidden width, input width and padded output count that is a multiple of 16 up to MLP_GENERAL_MAX_*; all ten hidden activations.
#pragma once
#include "mlp_kernels.h"

namespace tcnn_hip {

TCNN_HOST_DEVICE size_t mlp_f32_saved_activation_bytes(const MlpMeta& m, uint32_t n) {
	return (size_t)(act_needs_preactivation(m.activation) ? 2u : 1u) * (m.n_hidden_matmuls + 1u) * n * m.width * sizeof(float);
}

// Forward.  hidden == nullptr: inference (two ping-pong matrices in stream-ordered scratch of the call).  trimmed.out given: inference into
// the caller's trimmed matrix instead of `output` (`hidden` and `output` must be null): element (sample i, output j < dims) at
// out[i * stride_i + j * stride_j], nothing else is written.
void mlp_f32_forward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params, const float* input, float* hidden, float* output,
                     const MlpF32Output& trimmed = {});

void mlp_f32_transpose_weights(hipStream_t stream, const MlpMeta& m, const float* params, float* params_t);

// dL/d(pre-activation of the output layer) from dL/doutput and the output; for output activations other than None.  [n][padded_out] each.
void mlp_f32_output_activation_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* output, const float* dL_doutput, float* dL_dpreact);

// Number of batch slices == fp32 slabs of the weight-gradient products: a function of the network and the batch size alone.
uint32_t mlp_f32_n_partials(const MlpMeta& m, uint32_t n);
size_t mlp_f32_backward_workspace_bytes(const MlpMeta& m, uint32_t n);  // dL/d(pre-activation) of every hidden layer
// dL_doutput: w.r.t. the output layer's pre-activation.  dL_dinput and partials ([mlp_f32_n_partials][n_params]) may be null.
void mlp_f32_backward(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params_t, const float* input, const float* hidden, const float* dL_doutput,
                      float* dL_dinput, float* partials, void* workspace);
// grads[i] = (accumulate ? grads[i] : 0) + (partials[0][i] + partials[1][i] + ...), slabs in ascending order
void mlp_f32_finalize_gradients(hipStream_t stream, const MlpMeta& m, uint32_t n_partials, const float* partials, float* grads, bool accumulate);

}  // namespace tcnn_hip

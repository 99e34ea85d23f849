// emu_driver_mlp.cpp -- the network's part of the emulator's driver (emu_driver.h): the launchers of csrc/mlp_kernels.hip (which brings
// csrc/mlp_general.hip along, the 16-bit layer-by-layer network), its fp32 twin csrc/mlp_general_fp32.hip and the register-resident kernels
// the launchers choose between, as one unit.  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#include "emu_driver.h"
#include "../../tiny-cuda-nn_amd/csrc/mlp_kernels.hip"
#include "../../tiny-cuda-nn_amd/csrc/mlp_general_fp32.hip"
#include "../../tiny-cuda-nn_amd/csrc/mlp_train_wave.hip"
#include "../../tiny-cuda-nn_amd/csrc/mlp_train_wide.hip"
#include "../../tiny-cuda-nn_amd/csrc/elementwise_kernels.h"  // reduce_sum (emu_driver_misc.cpp holds the kernels)

#include <vector>

using namespace tcnn_hip;

namespace {

std::vector<uint16_t> transposed_weights(const MlpMeta& m, const uint16_t* params) {
	std::vector<uint16_t> params_t(m.n_params());
	mlp_transpose_weights(nullptr, m, (const half_t*)params, (half_t*)params_t.data());
	return params_t;
}

// k_mlp_train with a loss (or the caller's dL/doutput in `la`) and either input form; returns prediction, dL_doutput, dL_dinput, grads
// (Overwrite) and the loss sum
void train(const MlpMeta& m, uint32_t n, const uint16_t* params, const uint16_t* input_soa, const MlpF32Input* fin, const MlpLossArgs& la, uint16_t* output,
           uint16_t* dL_doutput, uint16_t* dL_dinput_soa, uint16_t* grads, float* loss_sum) {
	const std::vector<uint16_t> params_t = transposed_weights(m, params);
	const uint32_t np = mlp_train_n_partials(m, n, la.type);
	std::vector<float> partials(grads ? (size_t)np * m.n_params() : 0, -12345.0f), block_sums(np, -777.0f), ws(1024);
	const SlabOrder order = mlp_train(nullptr, m, n, (const half_t*)params, (const half_t*)params_t.data(), (const half_t*)input_soa, la, (half_t*)output, (half_t*)dL_doutput,
	                                  (half_t*)dL_dinput_soa, grads ? partials.data() : nullptr, block_sums.data(), fin);
	if (grads) mlp_finalize_gradients(nullptr, m, np, partials.data(), (half_t*)grads, false, order);
	if (loss_sum) reduce_sum(nullptr, block_sums.data(), block_sums.size(), ws.data(), loss_sum);
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int emu_mlp_forward(const EmuMlp* e, uint32_t n, const uint16_t* params, const uint16_t* input_soa, uint16_t* hidden, uint16_t* output) {
	return emu_call(__func__, [&] { mlp_forward(nullptr, make_mlp(e), n, (const half_t*)params, (const half_t*)input_soa, (half_t*)hidden, (half_t*)output); });
}

// Inference straight into the caller's fp32 matrix (MlpF32Output) with the caller's strides.  input feature-major [in_width][n]; element
// (sample i, output j < dims) goes to out[i * stride_i + j * stride_j].  2: no kernel stores fp32 itself for this network.
int emuwo_mlp_forward_f32(const EmuMlp* e, uint32_t n, const uint16_t* params, const uint16_t* input_soa, float* out, uint32_t dims, uint32_t stride_i, uint32_t stride_j) {
	return emu_call(__func__, [&]() -> int {
		const MlpMeta m = make_mlp(e);
		if (!mlp_forward_f32_supported(m, n)) return 2;
		mlp_forward_f32(nullptr, m, n, (const half_t*)params, (const half_t*)input_soa, MlpF32Output{out, dims, stride_i, stride_j});
		return 0;
	});
}

// the register-resident inference kernel reading an unpadded Identity encoding's fp32 input itself (MlpF32Input); out_half [n][16] or, if
// out_f32 is given, the caller's fp32 matrix [n][dims].  2: no instance.
int emu_mlp_infer_f32_input(const EmuMlp* e, uint32_t n, const uint16_t* params, const float* x, float scale, float offset, uint16_t* out_half, float* out_f32,
                            uint32_t dims) {
	return emu_call(__func__, [&]() -> int {
		const MlpMeta m = make_mlp(e);
		if (!mlp_infer_f32_input_supported(m, n)) return 2;
		MlpF32Input fin;
		fin.x = x;
		fin.scale = scale;
		fin.offset = offset;
		MlpF32Output f32;
		if (out_f32) f32 = {out_f32, dims, dims, 1u};
		mlp_infer_wave(nullptr, m, n, (const half_t*)params, nullptr, (half_t*)out_half, f32, &fin);
		return 0;
	});
}

// grads: half [n_params] (Overwrite unless accumulate); scratch sizes are handled here.
int emu_mlp_backward(const EmuMlp* e, uint32_t n, const uint16_t* params, const uint16_t* input_soa, const uint16_t* hidden,
                     const uint16_t* dL_doutput, uint16_t* dL_dinput_soa, uint16_t* grads, int accumulate, const uint16_t* output) {
	return emu_call(__func__, [&] {
		const MlpMeta m = make_mlp(e);
		const std::vector<uint16_t> params_t = transposed_weights(m, params);
		const uint32_t np = mlp_backward_n_partials(m, n);
		std::vector<float> partials(grads ? (size_t)np * m.n_params() : 0, -12345.0f);
		std::vector<uint16_t> dpre;
		if (m.output_activation != (uint32_t)Activation::None) {
			if (!output) throw std::runtime_error("output required");
			dpre.resize((size_t)n * m.padded_out);
			mlp_output_activation_backward(nullptr, m, n, (const half_t*)output, (const half_t*)dL_doutput, (half_t*)dpre.data());
			dL_doutput = dpre.data();
		}
		std::vector<unsigned char> deep(mlp_backward_workspace_bytes(m, n) + 16, 0xCD);
		mlp_backward(nullptr, m, n, (const half_t*)params_t.data(), (const half_t*)input_soa, (const half_t*)hidden,
		             (const half_t*)dL_doutput, (half_t*)dL_dinput_soa, grads ? partials.data() : nullptr, deep.data());
		if (grads) mlp_finalize_gradients(nullptr, m, np, partials.data(), (half_t*)grads, accumulate != 0);
	});
}

// fused forward + loss + backward (train() above).  external_dL_doutput [n][16]: no loss is evaluated.  2: no instance takes the network.
int emu_mlp_train(const EmuMlp* e, uint32_t n, const uint16_t* params, const uint16_t* input_soa, int loss_type, const float* target,
                  const float* data_pdf, uint32_t dims, float loss_scale, uint32_t n_total, uint16_t* output, uint16_t* dL_doutput,
                  uint16_t* dL_dinput_soa, uint16_t* grads, float* loss_sum, const uint16_t* external_dL_doutput) {
	return emu_call(__func__, [&]() -> int {
		const MlpMeta m = make_mlp(e);
		if (!mlp_train_supported(m)) return 2;
		MlpLossArgs la = {external_dL_doutput ? LossType::L2 : (LossType)loss_type, target, data_pdf, dims, loss_scale, n_total};
		la.external_dL_doutput = (const half_t*)external_dL_doutput;
		train(m, n, params, input_soa, nullptr, la, output, dL_doutput, dL_dinput_soa, grads, loss_sum);
		return 0;
	});
}

// the same with the network kernel loading an unpadded Identity encoding's fp32 input itself (MlpF32Input); 2: no instance offers it.
// enc_out [in_width][n] receives the encoded input the kernel leaves behind.
int emu_mlp_train_f32_input(const EmuMlp* e, uint32_t n, const uint16_t* params, const float* x, float scale, float offset, int loss_type, const float* target,
                            const float* data_pdf, uint32_t dims, float loss_scale, uint32_t n_total, uint16_t* output, uint16_t* dL_doutput,
                            uint16_t* dL_dinput_soa, uint16_t* grads, float* loss_sum, uint16_t* enc_out) {
	return emu_call(__func__, [&]() -> int {
		const MlpMeta m = make_mlp(e);
		if (!mlp_train_supported(m) || !mlp_train_f32_input_supported(m, n, (LossType)loss_type)) return 2;
		MlpF32Input fin;
		fin.x = x;
		fin.scale = scale;
		fin.offset = offset;
		fin.enc_out = (half_t*)enc_out;
		train(m, n, params, nullptr, &fin, MlpLossArgs{(LossType)loss_type, target, data_pdf, dims, loss_scale, n_total}, output, dL_doutput, dL_dinput_soa, grads, loss_sum);
		return 0;
	});
}

// ---- the fp32 network (mlp_general_fp32.hip; these entry points do not depend on -DTCNN_BF16) ----
// input feature-major [in_width][n].  hidden: the saved stack (mlp_f32_saved_activation_bytes) or null (inference); output [n][padded_out],
// or -- trimmed given (inference only) -- element (sample i, output j < dims) at trimmed[i * stride_i + j * stride_j].
int emuf32_mlp_forward(const EmuMlp* e, uint32_t n, const float* params, const float* input_fm, float* hidden, float* output, float* trimmed, uint32_t dims,
                       uint32_t stride_i, uint32_t stride_j) {
	return emu_call(__func__, [&] {
		MlpF32Output t;
		if (trimmed) t = {trimmed, dims, stride_i, stride_j};
		mlp_f32_forward(nullptr, make_mlp(e), n, params, input_fm, hidden, trimmed ? nullptr : output, t);
	});
}

uint64_t emuf32_saved_activation_floats(const EmuMlp* e, uint32_t n) { return mlp_f32_saved_activation_bytes(make_mlp(e), n) / sizeof(float); }
uint32_t emuf32_n_partials(const EmuMlp* e, uint32_t n) { return mlp_f32_n_partials(make_mlp(e), n); }

// grads: float [n_params], overwritten unless `accumulate`; `output` is needed when the output activation is not None
int emuf32_mlp_backward(const EmuMlp* e, uint32_t n, const float* params, const float* input_fm, const float* hidden, const float* dL_doutput, float* dL_dinput_fm, float* grads,
                        int accumulate, const float* output) {
	return emu_call(__func__, [&] {
		const MlpMeta m = make_mlp(e);
		std::vector<float> params_t(m.n_params(), -777.0f);
		mlp_f32_transpose_weights(nullptr, m, params, params_t.data());
		const uint32_t np = mlp_f32_n_partials(m, n);
		std::vector<float> partials(grads ? (size_t)np * m.n_params() : 0, -12345.0f), dpre;
		if (m.output_activation != (uint32_t)Activation::None) {
			if (!output) throw std::runtime_error("output required");
			dpre.resize((size_t)n * m.padded_out);
			mlp_f32_output_activation_backward(nullptr, m, n, output, dL_doutput, dpre.data());
			dL_doutput = dpre.data();
		}
		std::vector<float> workspace(mlp_f32_backward_workspace_bytes(m, n) / sizeof(float), -4321.0f);
		mlp_f32_backward(nullptr, m, n, params_t.data(), input_fm, hidden, dL_doutput, dL_dinput_fm, grads ? partials.data() : nullptr, workspace.data());
		if (grads) mlp_f32_finalize_gradients(nullptr, m, np, partials.data(), grads, accumulate != 0);
	});
}

}  // extern "C"
#pragma GCC visibility pop

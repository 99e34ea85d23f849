// emu_driver_mlp_second_order.cpp -- the second-order pass of the fp32 network (csrc/mlp_general_fp32.hip mlp_f32_backward_backward) on the
// host emulator: a driver part of its own, built into a library of its own by emu_mlp_second_order.py with emu.py's command lines.  The
// fp32 unit holds no 16-bit type, so one build serves.  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#include "emu_driver.h"
#include "../../tiny-cuda-nn_amd/csrc/mlp_general_fp32.hip"

#include <vector>

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

uint32_t emumso_has_curvature(const EmuMlp* e) { return mlp_f32_second_order_has_curvature(make_mlp(e)) ? 1u : 0u; }
uint64_t emumso_workspace_floats(const EmuMlp* e, uint32_t n) { return mlp_f32_backward_backward_workspace_bytes(make_mlp(e), n) / sizeof(float); }

// input, v and dL_dinput feature-major [in_width][n]; hidden: the saved stack of emuf32_mlp_forward; dL_doutput / dL_ddLdoutput
// [n][padded_out]; grads [n_params], overwritten.  Each of the three results may be null.
int emumso_backward_backward(const EmuMlp* e, uint32_t n, const float* params, const float* input_fm, const float* hidden, const float* v_fm, const float* dL_doutput,
                             float* dL_ddLdoutput, float* dL_dinput_fm, float* grads) {
	return emu_call(__func__, [&] {
		const MlpMeta m = make_mlp(e);
		std::vector<float> params_t(m.n_params(), -777.0f);
		mlp_f32_transpose_weights(nullptr, m, params, params_t.data());
		const uint32_t np = mlp_f32_n_partials(m, n);
		std::vector<float> partials(grads ? (size_t)np * m.n_params() : 0, -12345.0f);
		std::vector<float> workspace(mlp_f32_backward_backward_workspace_bytes(m, n) / sizeof(float), -4321.0f);
		mlp_f32_backward_backward(nullptr, m, n, params, params_t.data(), input_fm, hidden, v_fm, dL_doutput, dL_ddLdoutput, dL_dinput_fm, grads ? partials.data() : nullptr,
		                          workspace.data());
		if (grads) mlp_f32_finalize_gradients(nullptr, m, np, partials.data(), grads, false);
	});
}

}  // extern "C"
#pragma GCC visibility pop

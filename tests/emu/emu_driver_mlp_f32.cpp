// emu_driver_mlp_f32.cpp -- the fp32 network's part of the emulator's driver: csrc/mlp_general_f32.hip on the host SIMT emulator, with the
// fp32 MFMA it needs defined here ahead of the kernel source (hip_emu.h has the 16-bit shapes only).  Built into a small library of its own
// by emu_mlp_f32.py with emu.py's compile and link lines; folding it into the single builder's part list is a later clean-up.
// TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#include "emu_driver.h"

#include <cmath>
#include <cstring>

namespace tcnn_hip {
// v_mfma_f32_16x16x4_f32: one float per lane and operand.  A[i][k]: lane = i + 16 k;  B[k][n]: lane = n + 16 k;  D[row][col]: lane = col +
// 16 (row / 4), element row % 4.  A k-ordered chain of fused multiply-adds, as on the device.
inline f4 mfma_16x16x4_f32(float a, float b, f4 c) {
	const unsigned lane = ::emu::g.cur->tidx.x & 63u;
	::emu::Wave& w = ::emu::g.waves[::emu::g.cur->tidx.x / 64];
	memcpy(&w.a[lane], &a, sizeof(float));
	memcpy(&w.b[lane], &b, sizeof(float));
	::emu::wave_barrier();
	f4 d = c;
	const unsigned col = lane & 15u, g = lane >> 4;
	for (unsigned r = 0; r < 4; ++r) {
		const unsigned row = 4 * g + r;
		float s = c[r];
		for (unsigned k = 0; k < 4; ++k) {
			float av, bv;
			memcpy(&av, &w.a[row + 16 * k], sizeof(float));
			memcpy(&bv, &w.b[col + 16 * k], sizeof(float));
			s = fmaf(av, bv, s);
		}
		d[r] = s;
	}
	::emu::wave_barrier();
	return d;
}
}  // namespace tcnn_hip

#include "../../tiny-cuda-nn_amd/csrc/mlp_general_f32.hip"

#include <vector>

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

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

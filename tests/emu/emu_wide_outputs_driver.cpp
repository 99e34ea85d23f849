// emu_wide_outputs_driver.cpp -- the network launchers (csrc/mlp_kernels.hip, which brings csrc/mlp_general.hip along, and the
// register-resident kernels they choose between) built for the host under the SIMT emulator (hip_emu.h), behind the one entry point emu_driver.cpp does not have: inference straight into the caller's fp32
// matrix (mlp_forward_f32, MlpF32Output) with the caller's strides.  A library of its own next to emu_driver.cpp's.
// TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#define TCNN_HOST_EMU 1
#include "../../tiny-cuda-nn_amd/csrc/mlp_kernels.hip"
#include "../../tiny-cuda-nn_amd/csrc/mlp_train_wave.hip"
#include "../../tiny-cuda-nn_amd/csrc/mlp_train_wide.hip"

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

// (the layout of emu.py's EmuMlp)
struct EmuMlp {
	uint32_t in_width, width, padded_out, n_hidden_matmuls, activation, output_activation;
};

// input feature-major [in_width][n]; element (sample i, output j < dims) goes to out[i * stride_i + j * stride_j].  2: no kernel stores
// fp32 itself for this network.
int emuwo_mlp_forward_f32(const EmuMlp* e, uint32_t n, const uint16_t* params, const uint16_t* input_soa, float* out, uint32_t dims, uint32_t stride_i, uint32_t stride_j) {
	try {
		const MlpMeta m = {e->in_width, e->width, e->padded_out, e->n_hidden_matmuls, e->activation, e->output_activation};
		if (!mlp_forward_f32_supported(m, n)) return 2;
		const MlpF32Output f32 = {out, dims, stride_i, stride_j};
		mlp_forward_f32(nullptr, m, n, (const half_t*)params, (const half_t*)input_soa, f32);
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuwo_mlp_forward_f32: %s\n", ex.what());
		return 1;
	}
	return 0;
}

}  // extern "C"
#pragma GCC visibility pop

// emu_half_input_driver.cpp -- the kernels of csrc/half_input_kernels.hip (the pad / un-pad streams between a caller's 16-bit matrix and the
// network kernels' feature-major matrices) built for the host under the SIMT emulator (hip_emu.h), behind a flat C interface (host pointers
// only).  A library of its own next to emu_driver.cpp's; the kernels move 16-bit words, so one build serves both 16-bit types.
// TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#define TCNN_HOST_EMU 1
#include "../../tiny-cuda-nn_amd/csrc/half_input_kernels.hip"

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

// in: [n][n_dims] sample-major; out: [padded][n] feature-major
int emuh_pad(uint32_t n, uint32_t n_dims, uint32_t padded, const uint16_t* in, uint16_t* out, uint32_t pad_bits) {
	try {
		half_input_pad(nullptr, n, n_dims, padded, in, out, (uint16_t)pad_bits);
	} catch (const std::exception&) {
		return 1;
	}
	return 0;
}
// dL_dy: [padded][n] feature-major (any padded >= n_dims: the rows behind n_dims are not read); dL_dx: [n][n_dims] sample-major
int emuh_unpad(uint32_t n, uint32_t n_dims, const uint16_t* dL_dy, uint16_t* dL_dx) {
	half_input_unpad(nullptr, n, n_dims, dL_dy, dL_dx);
	return 0;
}

}  // extern "C"
#pragma GCC visibility pop

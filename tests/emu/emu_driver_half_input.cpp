// emu_driver_half_input.cpp -- csrc/half_input_kernels.hip's part of the emulator's driver (emu_driver.h): the pad / un-pad streams between
// a caller's 16-bit matrix and the network kernels' feature-major matrices.  A unit of its own because its file-local helpers carry names
// that csrc/optimizer_kernels.hip also uses.  The kernels move 16-bit words whatever they encode; the padding's bit pattern is an argument.
// TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#include "emu_driver.h"
#include "../../tiny-cuda-nn_amd/csrc/half_input_kernels.hip"

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

// in: [n][n_dims] sample-major; out: [padded][n] feature-major
int emuh_pad(uint32_t n, uint32_t n_dims, uint32_t padded, const uint16_t* in, uint16_t* out, uint32_t pad_bits) {
	return emu_call(__func__, [&] { half_input_pad(nullptr, n, n_dims, padded, in, out, (uint16_t)pad_bits); });
}
// dL_dy: [padded][n] feature-major (any padded >= n_dims: the rows behind n_dims are not read); dL_dx: [n][n_dims] sample-major
int emuh_unpad(uint32_t n, uint32_t n_dims, const uint16_t* dL_dy, uint16_t* dL_dx) {
	half_input_unpad(nullptr, n, n_dims, dL_dy, dL_dx);
	return 0;
}

}  // extern "C"
#pragma GCC visibility pop

// emu_composite_driver.cpp -- the kernels of csrc/composite_kernels.hip (triangle wave, the fused parameter-free parts of a Composite
// encoding, the Sum / Product reductions) built for the host under the SIMT emulator (hip_emu.h), behind a flat C interface (host
// pointers only).  A library of its own next to emu_driver.cpp's.  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#define TCNN_HOST_EMU 1
#include "../../tiny-cuda-nn_amd/csrc/composite_kernels.hip"

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

// value matrices are feature-major [rows][n] when soa, sample-major [n][rows] otherwise; fp32: float values instead of the 16-bit type
int emuc_triangle_wave_forward(uint32_t n, uint32_t n_dims, uint32_t n_frequencies, uint32_t padded, const float* in, void* out, int soa, int fp32) {
	const uint32_t sk = soa ? n : 1u, si = soa ? 1u : padded;
	if (fp32) triangle_wave_forward(nullptr, n, n_dims, n_frequencies, padded, in, n_dims, 1, (float*)out, sk, si);
	else triangle_wave_forward(nullptr, n, n_dims, n_frequencies, padded, in, n_dims, 1, (half_t*)out, sk, si);
	return 0;
}
int emuc_triangle_wave_backward(uint32_t n, uint32_t n_dims, uint32_t n_frequencies, uint32_t padded, const void* dL_dy, int soa, int fp32, const float* in, float* dL_dx) {
	const uint32_t sk = soa ? n : 1u, si = soa ? 1u : padded;
	if (fp32) triangle_wave_backward(nullptr, n, n_dims, n_frequencies, (const float*)dL_dy, sk, si, in, n_dims, 1, dL_dx, n_dims, 1);
	else triangle_wave_backward(nullptr, n, n_dims, n_frequencies, (const half_t*)dL_dy, sk, si, in, n_dims, 1, dL_dx, n_dims, 1);
	return 0;
}
// table: n_parts rows of {kind, in_row, in_width, out_row, padded_width, param}
static EncodingParts make_parts(uint32_t n_parts, const uint32_t* table) {
	EncodingParts parts;
	for (uint32_t p = 0; p < n_parts; ++p) {
		const uint32_t* t = table + 6 * p;
		parts.add(EncodingPart{t[0], t[1], t[2], t[3], t[4], t[5], 1.0f, 0.0f});
	}
	return parts;
}
int emuc_parts_forward(uint32_t n_parts, const uint32_t* table, uint32_t n, uint32_t n_input_dims, uint32_t width, const float* in, void* out, int soa, int fp32) {
	const uint32_t sk = soa ? n : 1u, si = soa ? 1u : width;
	try {
		const EncodingParts parts = make_parts(n_parts, table);
		if (fp32) encoding_parts_forward(nullptr, parts, n, in, n_input_dims, 1, (float*)out, sk, si);
		else encoding_parts_forward(nullptr, parts, n, in, n_input_dims, 1, (half_t*)out, sk, si);
	} catch (const std::exception&) {
		return 1;
	}
	return 0;
}
int emuc_parts_backward(uint32_t n_parts, const uint32_t* table, uint32_t n, uint32_t n_input_dims, uint32_t width, const void* dL_dy, int soa, int fp32, const float* in,
                        float* dL_dx) {
	const uint32_t sk = soa ? n : 1u, si = soa ? 1u : width;
	try {
		const EncodingParts parts = make_parts(n_parts, table);
		if (fp32) encoding_parts_backward(nullptr, parts, n, n_input_dims, (const float*)dL_dy, sk, si, in, n_input_dims, 1, dL_dx, n_input_dims, 1);
		else encoding_parts_backward(nullptr, parts, n, n_input_dims, (const half_t*)dL_dy, sk, si, in, n_input_dims, 1, dL_dx, n_input_dims, 1);
	} catch (const std::exception&) {
		return 1;
	}
	return 0;
}
int emuc_reduce_forward(int product, uint32_t n, uint32_t width, uint32_t n_to_reduce, const void* to_reduce, void* reduced, int soa, int fp32) {
	const uint32_t sk = soa ? n : 1u;
	if (fp32) reduce_forward(nullptr, product != 0, n, width, n_to_reduce, (const float*)to_reduce, sk, soa ? 1u : width * n_to_reduce, (float*)reduced, sk, soa ? 1u : width);
	else reduce_forward(nullptr, product != 0, n, width, n_to_reduce, (const half_t*)to_reduce, sk, soa ? 1u : width * n_to_reduce, (half_t*)reduced, sk, soa ? 1u : width);
	return 0;
}
int emuc_reduce_backward(int product, uint32_t n, uint32_t width, uint32_t n_to_reduce, const void* to_reduce, void* dL_dunreduced, const void* dL_dreduced, int soa, int fp32) {
	const uint32_t sk = soa ? n : 1u;
	if (fp32) {
		reduce_backward(nullptr, product != 0, n, width, n_to_reduce, (const float*)to_reduce, (float*)dL_dunreduced, sk, soa ? 1u : width * n_to_reduce, (const float*)dL_dreduced, sk,
		                soa ? 1u : width);
	} else {
		reduce_backward(nullptr, product != 0, n, width, n_to_reduce, (const half_t*)to_reduce, (half_t*)dL_dunreduced, sk, soa ? 1u : width * n_to_reduce, (const half_t*)dL_dreduced,
		                sk, soa ? 1u : width);
	}
	return 0;
}

}  // extern "C"
#pragma GCC visibility pop

// encoding_device.h -- the per-element arithmetic of the encodings without parameters (identity, frequency, one-blob, triangle wave), written
// once: the stand-alone kernels (elementwise_kernels.hip, composite_kernels.hip) and the fused kernels that run all such parts of a
// Composite encoding in one launch (composite_kernels.hip) call these functions, so a slice of a Composite holds the stand-alone
// encoding's bits.  fp32 throughout, every expression in the order the reference writes it; build with -ffp-contract=off.
#pragma once
#include <cmath>
#include <type_traits>

#include "tcnn_device.h"

namespace tcnn_hip {

// The element-wise encodings write their value type VAL_T: the library's 16-bit type (rounded to nearest even, as the reference's
// (T) casts do), or float for the fp32 encodings of create_encoding(..., Precision::Fp32) (Encoding<float>, cpp_api.cu:165-168).
template <typename VAL_T>
TCNN_DEVICE VAL_T encoded_value(float v) {
	if constexpr (std::is_same<VAL_T, float>::value) return v;
	else return to_half_rn(v);
}

// ------------------------------------------------------------------------------------------ identity (identity.h:46-84)
TCNN_DEVICE float identity_value(float x, float scale, float offset) {
	float t = x * scale;
	t = t + offset;
	return t;
}
// identity.h:83: (T)((float)dL_dy * scale) -- rounded through the value type, then widened to the fp32 dL_dx
template <typename VAL_T>
TCNN_DEVICE float identity_dL_dx(VAL_T dL_dy, float scale) { return (float)encoded_value<VAL_T>((float)dL_dy * scale); }

// ------------------------------------------------------------------------------------------ frequency (frequency.h:46-104)
#define TCNN_PI_F 3.14159265358979323846f
// output k < 2 n_frequencies of one input dimension: sin(2^(k / 2) pi x + (k & 1) pi / 2)
TCNN_DEVICE float frequency_argument(float x0, uint32_t k) {
	const uint32_t log2_frequency = k / 2u;
	const float phase_shift = (float)(k % 2u) * (TCNN_PI_F / 2);
	const float x = __builtin_scalbnf(x0, (int)log2_frequency);
	return x * TCNN_PI_F + phase_shift;
}
TCNN_DEVICE float frequency_value(float x0, uint32_t k) { return sinf(frequency_argument(x0, k)); }
// dL_dy: the gradient of this dimension's first output for this sample, the following outputs stride_k elements apart
template <typename VAL_T>
TCNN_DEVICE float frequency_dL_dx(const VAL_T* __restrict__ dL_dy, size_t stride_k, uint32_t n_frequencies, float x0) {
	float result = 0;
	for (uint32_t k = 0; k < n_frequencies * 2u; ++k) {
		const float dy_dx = __builtin_scalbnf(1.0f, (int)(k / 2u)) * TCNN_PI_F * cosf(frequency_argument(x0, k));  // what the reference's forward pass stores
		result += (float)dL_dy[(size_t)k * stride_k] * dy_dx;
	}
	return result;
}

// ------------------------------------------------------------------------------------------ one-blob (oneblob.h:84-164, common_device.h:1076-1095)
TCNN_DEVICE float quartic(float x, float inv_radius) {
	const float u = x * inv_radius;
	const float tmp = __builtin_fmaxf(1 - u * u, 0.0f);
	return ((float)15 / 16) * tmp * tmp;
}
TCNN_DEVICE float quartic_cdf_deriv(float x, float inv_radius) { return quartic(x, inv_radius) * inv_radius; }
TCNN_DEVICE float quartic_cdf(float x, float inv_radius) {
	const float u = x * inv_radius;
	const float u2 = u * u;
	const float u4 = u2 * u2;
	return __builtin_fmaxf(0.0f, __builtin_fminf(1.0f, ((float)15 / 16) * u * (1 - ((float)2 / 3) * u2 + ((float)1 / 5) * u4) + 0.5f));
}
// the blob's integral up to a bin boundary, wrapped around [0, 1): t = boundary - x
TCNN_DEVICE float oneblob_cdf(float t, float n_bins) { return quartic_cdf(t, n_bins) + quartic_cdf(t - 1.0f, n_bins) + quartic_cdf(t + 1.0f, n_bins); }
TCNN_DEVICE float oneblob_cdf_deriv(float t, float n_bins) { return quartic_cdf_deriv(t, n_bins) + quartic_cdf_deriv(t - 1.0f, n_bins) + quartic_cdf_deriv(t + 1.0f, n_bins); }
// t of boundary b (bin b's left, bin b - 1's right) as the loop over the bins forms it: -x for the first, b / n_bins - x after it
TCNN_DEVICE float oneblob_boundary(float x, uint32_t b, float inv_bins) { return b == 0u ? -x : (float)b * inv_bins - x; }  // scalbnf(b, -log2_bins) == b * inv_bins exactly
// bin b of one dimension on its own (the fused kernel: one thread per output)
TCNN_DEVICE float oneblob_value(float x, uint32_t b, uint32_t n_bins) {
	const float nb = (float)n_bins, inv_bins = 1.0f / nb;
	const float left_cdf = oneblob_cdf(oneblob_boundary(x, b, inv_bins), nb);
	const float right_cdf = oneblob_cdf(oneblob_boundary(x, b + 1u, inv_bins), nb);
	return right_cdf - left_cdf;
}
template <typename VAL_T>
TCNN_DEVICE float oneblob_dL_dx(const VAL_T* __restrict__ dL_dy, size_t stride_k, uint32_t n_bins, float x) {
	const float nb = (float)n_bins, inv_bins = 1.0f / nb;
	float result = 0;
	float left_cdf = oneblob_cdf_deriv(oneblob_boundary(x, 0u, inv_bins), nb);
	for (uint32_t k = 0; k < n_bins; ++k) {
		const float right_cdf = oneblob_cdf_deriv(oneblob_boundary(x, k + 1u, inv_bins), nb);
		const float deriv = left_cdf - right_cdf;
		left_cdf = right_cdf;
		result += (float)dL_dy[(size_t)k * stride_k] * deriv;
	}
	return result;
}

// ------------------------------------------------------------------------------------------ triangle wave (triangle_wave.h:46-108)
// output k < n_frequencies of one input dimension.  Every step is exact or a single rounding: the result is bit-reproducible.
TCNN_DEVICE float triangle_wave_phase(float x0, uint32_t k) {
	const float x = __builtin_scalbnf(x0, (int)k - 1);
	return x + (float)k * 0.25f;  // small frequency-based phase shift (triangle_wave.h:72-73)
}
TCNN_DEVICE float triangle_wave_value(float x0, uint32_t k) {
	const float val = triangle_wave_phase(x0, k);
	return __builtin_fabsf(val - floorf(val) - 0.5f) * 4 - 1;
}
// the derivative the reference's forward pass stores (triangle_wave.h:78), recomputed from the input; summed in ascending k
template <typename VAL_T>
TCNN_DEVICE float triangle_wave_dL_dx(const VAL_T* __restrict__ dL_dy, size_t stride_k, uint32_t n_frequencies, float x0) {
	float result = 0;
	for (uint32_t k = 0; k < n_frequencies; ++k) {
		const float val = triangle_wave_phase(x0, k);
		const float dy_dx = __builtin_scalbnf((int)floorf(val * 2.0f) % 2 == 0 ? -1.0f : 1.0f, (int)k + 1);
		result += (float)dL_dy[(size_t)k * stride_k] * dy_dx;
	}
	return result;
}

}  // namespace tcnn_hip

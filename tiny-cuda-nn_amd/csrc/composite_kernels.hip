// composite_kernels.hip -- see composite_kernels.h.  Pure HBM streams: every workgroup takes 256 consecutive samples, the row it works on
// comes from the block index or a loop counter and is therefore wave-uniform (the part table is read with scalar loads), consecutive
// lanes take consecutive samples (2-byte / 4-byte row stores that coalesce in the feature-major matrix the network reads).
// Build with -ffp-contract=off (the arithmetic of encoding_device.h is checked bit for bit).
#include "composite_kernels.h"

#include <stdexcept>
#include <string>

#include "encoding_device.h"

namespace tcnn_hip {

constexpr uint32_t CK_THREADS = 256;
static_assert(BATCH_SIZE_GRANULARITY % CK_THREADS == 0, "every workgroup is full");

static void check_rows(const char* what, uint32_t n, uint32_t rows) {
	if (n % CK_THREADS != 0) throw std::runtime_error(std::string(what) + ": the batch size must be a multiple of " + std::to_string(CK_THREADS));
	if (rows > 65535u) throw std::runtime_error(std::string(what) + ": more than 65535 rows");
}

// ------------------------------------------------------------------------------------------ triangle wave
// One thread per output element (k-major, i fastest), as k_frequency_forward.
template <typename VAL_T>
__global__ void __launch_bounds__(CK_THREADS) k_triangle_wave_forward(uint32_t n, uint32_t n_dims, uint32_t n_frequencies, uint32_t padded, const float* __restrict__ in,
                                                                      uint32_t in_stride_i, uint32_t in_stride_j, VAL_T* __restrict__ out, uint32_t stride_k,
                                                                      uint32_t stride_i) {
	const uint32_t e = blockIdx.x * CK_THREADS + threadIdx.x;
	if (e >= n * padded) return;
	const uint32_t j = e / n, i = e - j * n;
	VAL_T v = (VAL_T)1.0f;  // triangle_wave.h:64-65
	if (j < n_dims * n_frequencies) {
		const uint32_t d = j / n_frequencies;
		v = encoded_value<VAL_T>(triangle_wave_value(in[(size_t)i * in_stride_i + (size_t)d * in_stride_j], j - d * n_frequencies));
	}
	out[(size_t)j * stride_k + (size_t)i * stride_i] = v;
}
template <typename VAL_T>
__global__ void __launch_bounds__(CK_THREADS) k_triangle_wave_backward(uint32_t n, uint32_t n_dims, uint32_t n_frequencies, const VAL_T* __restrict__ dL_dy,
                                                                       uint32_t stride_k, uint32_t stride_i, const float* __restrict__ in, uint32_t in_stride_i,
                                                                       uint32_t in_stride_j, float* __restrict__ dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_j) {
	const uint32_t e = blockIdx.x * CK_THREADS + threadIdx.x;
	if (e >= n * n_dims) return;
	const uint32_t d = e / n, i = e - d * n;
	const float x0 = in[(size_t)i * in_stride_i + (size_t)d * in_stride_j];
	dL_dx[(size_t)i * dx_stride_i + (size_t)d * dx_stride_j] = triangle_wave_dL_dx<VAL_T>(dL_dy + (size_t)d * n_frequencies * stride_k + (size_t)i * stride_i, stride_k, n_frequencies, x0);
}
template <typename VAL_T>
void triangle_wave_forward(hipStream_t stream, uint32_t n, uint32_t n_dims, uint32_t n_frequencies, uint32_t padded, const float* in, uint32_t in_stride_i,
                           uint32_t in_stride_j, VAL_T* out, uint32_t stride_k, uint32_t stride_i) {
	if (n == 0 || padded == 0) return;
	TCNN_LAUNCH(k_triangle_wave_forward<VAL_T>, dim3(div_round_up(n * padded, CK_THREADS)), dim3(CK_THREADS), 0, stream, n, n_dims, n_frequencies, padded, in, in_stride_i,
	            in_stride_j, out, stride_k, stride_i);
}
template <typename VAL_T>
void triangle_wave_backward(hipStream_t stream, uint32_t n, uint32_t n_dims, uint32_t n_frequencies, const VAL_T* dL_dy, uint32_t stride_k, uint32_t stride_i,
                            const float* in, uint32_t in_stride_i, uint32_t in_stride_j, float* dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_j) {
	if (n == 0 || n_dims == 0) return;
	TCNN_LAUNCH(k_triangle_wave_backward<VAL_T>, dim3(div_round_up(n * n_dims, CK_THREADS)), dim3(CK_THREADS), 0, stream, n, n_dims, n_frequencies, dL_dy, stride_k, stride_i, in,
	            in_stride_i, in_stride_j, dL_dx, dx_stride_i, dx_stride_j);
}
TCNN_INSTANTIATE_VALUE_TYPES(triangle_wave_forward)
TCNN_INSTANTIATE_VALUE_TYPES(triangle_wave_backward)

// ------------------------------------------------------------------------------------------ all parts without parameters in one launch
void EncodingParts::add(const EncodingPart& p) {
	if (n_parts >= ENCODING_MAX_PARTS) {
		throw std::runtime_error("CompositeEncoding: more than " + std::to_string(ENCODING_MAX_PARTS) + " nested encodings without parameters are not supported by this build");
	}
	part[n_parts++] = p;
	n_rows += p.padded_width;
}

// outputs per input dimension
TCNN_DEVICE uint32_t part_fan_out(const EncodingPart& p) {
	return p.kind == PART_IDENTITY ? 1u : p.kind == PART_FREQUENCY ? p.param * 2u : p.param;
}

// Forward.  Workgroup (x, y): samples [256 x, 256 x + 256), rows [PARTS_ROWS y, PARTS_ROWS y + PARTS_ROWS) of the parts' rows laid end to
// end.  The row loop is uniform: part, input dimension and output index of a row live in scalar registers, a lane loads its sample's value
// of an input dimension once for all the consecutive rows that read it, and every row leaves as one 512-byte (16-bit) run per workgroup.
constexpr uint32_t PARTS_ROWS = 16;
template <typename VAL_T>
__global__ void __launch_bounds__(CK_THREADS) k_encoding_parts_forward(const EncodingParts parts, uint32_t n, const float* __restrict__ in, uint32_t in_stride_i,
                                                                       uint32_t in_stride_d, VAL_T* __restrict__ out, uint32_t stride_k, uint32_t stride_i) {
	const uint32_t i = blockIdx.x * CK_THREADS + threadIdx.x;
	if (i >= n) return;
	uint32_t row = blockIdx.y * PARTS_ROWS;
	const uint32_t row_end = min(row + PARTS_ROWS, parts.n_rows);
	uint32_t p = 0, r = row;  // row = row r of part p
	while (p + 1u < parts.n_parts && r >= parts.part[p].padded_width) r -= parts.part[p++].padded_width;
	const float* __restrict__ x_i = in + (size_t)i * in_stride_i;
	VAL_T* __restrict__ out_i = out + (size_t)i * stride_i;
	uint32_t loaded_dim = 0xFFFFFFFFu;
	float x = 0.0f;
	for (; row < row_end; ++row, ++r) {
		while (p + 1u < parts.n_parts && r >= parts.part[p].padded_width) r -= parts.part[p++].padded_width;
		const EncodingPart part = parts.part[p];
		const uint32_t fan_out = part_fan_out(part);
		VAL_T v = (VAL_T)1.0f;  // the padding value of every encoding without parameters
		if (r < part.in_width * fan_out) {
			const uint32_t d = r / fan_out, k = r - d * fan_out;
			if (part.in_row + d != loaded_dim) {
				loaded_dim = part.in_row + d;
				x = x_i[(size_t)loaded_dim * in_stride_d];
			}
			float y;
			switch (part.kind) {
				case PART_ONEBLOB: y = oneblob_value(x, k, part.param); break;
				case PART_FREQUENCY: y = frequency_value(x, k); break;
				case PART_TRIANGLE_WAVE: y = triangle_wave_value(x, k); break;
				default: y = identity_value(x, part.scale, part.offset); break;
			}
			v = encoded_value<VAL_T>(y);
		}
		out_i[(size_t)(part.out_row + r) * stride_k] = v;
	}
}

// Backward.  Workgroup (x, d): samples [256 x, 256 x + 256) of input dimension d -- the part that reads d (if any) is a scalar search.
template <typename VAL_T>
__global__ void __launch_bounds__(CK_THREADS) k_encoding_parts_backward(const EncodingParts parts, uint32_t n, const VAL_T* __restrict__ dL_dy, uint32_t stride_k,
                                                                        uint32_t stride_i, const float* __restrict__ in, uint32_t in_stride_i, uint32_t in_stride_d,
                                                                        float* __restrict__ dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_d) {
	const uint32_t i = blockIdx.x * CK_THREADS + threadIdx.x, d = blockIdx.y;
	if (i >= n) return;
	uint32_t p = 0;
	while (p < parts.n_parts && !(d >= parts.part[p].in_row && d - parts.part[p].in_row < parts.part[p].in_width)) ++p;
	float result = 0.0f;  // a dim no part reads
	if (p < parts.n_parts) {
		const EncodingPart part = parts.part[p];
		const uint32_t local = d - part.in_row;
		const VAL_T* __restrict__ dy = dL_dy + (size_t)(part.out_row + local * part_fan_out(part)) * stride_k + (size_t)i * stride_i;
		if (part.kind == PART_IDENTITY) {
			result = identity_dL_dx<VAL_T>(dy[0], part.scale);
		} else {
			const float x = in[(size_t)i * in_stride_i + (size_t)d * in_stride_d];
			switch (part.kind) {
				case PART_ONEBLOB: result = oneblob_dL_dx<VAL_T>(dy, stride_k, part.param, x); break;
				case PART_FREQUENCY: result = frequency_dL_dx<VAL_T>(dy, stride_k, part.param, x); break;
				default: result = triangle_wave_dL_dx<VAL_T>(dy, stride_k, part.param, x); break;
			}
		}
	}
	dL_dx[(size_t)i * dx_stride_i + (size_t)d * dx_stride_d] = result;
}

template <typename VAL_T>
void encoding_parts_forward(hipStream_t stream, const EncodingParts& parts, uint32_t n, const float* in, uint32_t in_stride_i, uint32_t in_stride_d, VAL_T* out,
                            uint32_t stride_k, uint32_t stride_i) {
	if (n == 0 || parts.n_rows == 0) return;
	check_rows("encoding_parts_forward", n, div_round_up(parts.n_rows, PARTS_ROWS));
	TCNN_LAUNCH(k_encoding_parts_forward<VAL_T>, dim3(n / CK_THREADS, div_round_up(parts.n_rows, PARTS_ROWS)), dim3(CK_THREADS), 0, stream, parts, n, in, in_stride_i, in_stride_d, out,
	            stride_k, stride_i);
}
template <typename VAL_T>
void encoding_parts_backward(hipStream_t stream, const EncodingParts& parts, uint32_t n, uint32_t n_input_dims, const VAL_T* dL_dy, uint32_t stride_k, uint32_t stride_i,
                             const float* in, uint32_t in_stride_i, uint32_t in_stride_d, float* dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_d) {
	if (n == 0 || n_input_dims == 0) return;
	check_rows("encoding_parts_backward", n, n_input_dims);
	TCNN_LAUNCH(k_encoding_parts_backward<VAL_T>, dim3(n / CK_THREADS, n_input_dims), dim3(CK_THREADS), 0, stream, parts, n, dL_dy, stride_k, stride_i, in, in_stride_i, in_stride_d,
	            dL_dx, dx_stride_i, dx_stride_d);
}
TCNN_INSTANTIATE_VALUE_TYPES(encoding_parts_forward)
TCNN_INSTANTIATE_VALUE_TYPES(encoding_parts_backward)

// ------------------------------------------------------------------------------------------ reductions (composite.h:47-133)
// Workgroup (x, j): samples [256 x, 256 x + 256) of feature row j; one thread per (row, sample).
template <typename T, bool PRODUCT>
__global__ void __launch_bounds__(CK_THREADS) k_reduce_forward(uint32_t n, uint32_t width, uint32_t n_to_reduce, const T* __restrict__ to_reduce, uint32_t stride_k,
                                                               uint32_t stride_i, T* __restrict__ reduced, uint32_t reduced_stride_k, uint32_t reduced_stride_i) {
	const uint32_t i = blockIdx.x * CK_THREADS + threadIdx.x, j = blockIdx.y;
	if (i >= n) return;
	float result = PRODUCT ? 1.0f : 0.0f;
	for (uint32_t k = 0; k < n_to_reduce; ++k) {
		const float v = (float)to_reduce[(size_t)(j + width * k) * stride_k + (size_t)i * stride_i];
		if (PRODUCT) result *= v;
		else result += v;
	}
	reduced[(size_t)j * reduced_stride_k + (size_t)i * reduced_stride_i] = encoded_value<T>(result);
}
template <typename T, bool PRODUCT>
__global__ void __launch_bounds__(CK_THREADS) k_reduce_backward(uint32_t n, uint32_t width, uint32_t n_to_reduce, const T* __restrict__ to_reduce, T* __restrict__ dL_dunreduced,
                                                                uint32_t stride_k, uint32_t stride_i, const T* __restrict__ dL_dreduced, uint32_t reduced_stride_k,
                                                                uint32_t reduced_stride_i) {
	const uint32_t i = blockIdx.x * CK_THREADS + threadIdx.x, j = blockIdx.y;
	if (i >= n) return;
	const T dy = dL_dreduced[(size_t)j * reduced_stride_k + (size_t)i * reduced_stride_i];
	for (uint32_t k = 0; k < n_to_reduce; ++k) {
		T v = dy;  // composite.h:79-82: the sum hands its gradient on
		if (PRODUCT) {  // composite.h:119-130: times all OTHER factors, ascending
			float result = (float)dy;
			for (uint32_t l = 0; l + 1u < n_to_reduce; ++l) result *= (float)to_reduce[(size_t)(j + width * (l < k ? l : (l + 1u))) * stride_k + (size_t)i * stride_i];
			v = encoded_value<T>(result);
		}
		dL_dunreduced[(size_t)(j + width * k) * stride_k + (size_t)i * stride_i] = v;
	}
}
template <typename T>
void reduce_forward(hipStream_t stream, bool product, uint32_t n, uint32_t width, uint32_t n_to_reduce, const T* to_reduce, uint32_t stride_k, uint32_t stride_i,
                    T* reduced, uint32_t reduced_stride_k, uint32_t reduced_stride_i) {
	if (n == 0 || width == 0) return;
	check_rows("reduce_forward", n, width);
	const dim3 grid(n / CK_THREADS, width);
	if (product) TCNN_LAUNCH((k_reduce_forward<T, true>), grid, dim3(CK_THREADS), 0, stream, n, width, n_to_reduce, to_reduce, stride_k, stride_i, reduced, reduced_stride_k, reduced_stride_i);
	else TCNN_LAUNCH((k_reduce_forward<T, false>), grid, dim3(CK_THREADS), 0, stream, n, width, n_to_reduce, to_reduce, stride_k, stride_i, reduced, reduced_stride_k, reduced_stride_i);
}
template <typename T>
void reduce_backward(hipStream_t stream, bool product, uint32_t n, uint32_t width, uint32_t n_to_reduce, const T* to_reduce, T* dL_dunreduced, uint32_t stride_k,
                     uint32_t stride_i, const T* dL_dreduced, uint32_t reduced_stride_k, uint32_t reduced_stride_i) {
	if (n == 0 || width == 0) return;
	check_rows("reduce_backward", n, width);
	const dim3 grid(n / CK_THREADS, width);
	if (product) {
		if (!to_reduce) throw std::runtime_error("reduce_backward: the product needs the forward pass's unreduced matrix");
		TCNN_LAUNCH((k_reduce_backward<T, true>), grid, dim3(CK_THREADS), 0, stream, n, width, n_to_reduce, to_reduce, dL_dunreduced, stride_k, stride_i, dL_dreduced, reduced_stride_k, reduced_stride_i);
	} else {
		TCNN_LAUNCH((k_reduce_backward<T, false>), grid, dim3(CK_THREADS), 0, stream, n, width, n_to_reduce, to_reduce, dL_dunreduced, stride_k, stride_i, dL_dreduced, reduced_stride_k, reduced_stride_i);
	}
}
TCNN_INSTANTIATE_VALUE_TYPES(reduce_forward)
TCNN_INSTANTIATE_VALUE_TYPES(reduce_backward)

}  // namespace tcnn_hip

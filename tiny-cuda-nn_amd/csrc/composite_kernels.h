// composite_kernels.h -- what a Composite encoding (composite.h) needs beyond the stand-alone encodings' kernels: the triangle-wave
// encoding, ONE launch for all nested encodings without parameters (identity / one-blob / frequency / triangle wave: the whole NRC input
// encoding), and the Sum / Product reductions.  Streaming kernels; the value type T is the library's 16-bit type or float.
// Addressing as everywhere (elementwise_kernels.h): input element (dim d, sample i) at in[i * in_stride_i + d * in_stride_d], encoded
// element (feature k, sample i) at out[k * stride_k + i * stride_i]; n is a multiple of BATCH_SIZE_GRANULARITY.
#pragma once
#include "tcnn_device.h"

namespace tcnn_hip {

// encodings/triangle_wave.h:46-108: n_frequencies outputs per input dimension, padding value 1; dL/dinput recomputes the derivative the
// reference stores.  (Every launcher here is instantiated for T = half_t and float in composite_kernels.hip.)
template <typename T>
void triangle_wave_forward(hipStream_t stream, uint32_t n, uint32_t n_dims, uint32_t n_frequencies, uint32_t padded, const float* in, uint32_t in_stride_i,
                           uint32_t in_stride_j, T* out, uint32_t stride_k, uint32_t stride_i);
template <typename T>
void triangle_wave_backward(hipStream_t stream, uint32_t n, uint32_t n_dims, uint32_t n_frequencies, const T* dL_dy, uint32_t stride_k, uint32_t stride_i,
                            const float* in, uint32_t in_stride_i, uint32_t in_stride_j, float* dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_j);

// One nested encoding without parameters: it reads input dims [in_row, in_row + in_width) and writes rows [out_row, out_row + padded_width)
// of the encoded matrix, the rows behind its own outputs with its padding value 1.  param: n_bins (one-blob), n_frequencies (frequency,
// triangle wave); the identity's scale and offset ride in their own two words.
enum EncodingPartKind : uint32_t { PART_IDENTITY = 0, PART_ONEBLOB = 1, PART_FREQUENCY = 2, PART_TRIANGLE_WAVE = 3 };
constexpr uint32_t ENCODING_MAX_PARTS = 16;  // the table travels by value in the kernel arguments (16 x 32 B); more parts are refused
struct EncodingPart {
	uint32_t kind, in_row, in_width, out_row, padded_width, param;
	float scale, offset;
};
struct EncodingParts {
	uint32_t n_parts = 0, n_rows = 0;  // n_rows: the sum of the parts' padded widths
	EncodingPart part[ENCODING_MAX_PARTS] = {};
	void add(const EncodingPart& p);  // throws beyond ENCODING_MAX_PARTS
};
// all parts in one launch
template <typename T>
void encoding_parts_forward(hipStream_t stream, const EncodingParts& parts, uint32_t n, const float* in, uint32_t in_stride_i, uint32_t in_stride_d, T* out,
                            uint32_t stride_k, uint32_t stride_i);
// dL_dx of ALL n_input_dims dims in one launch: a dim some part reads gets that part's gradient, every other dim is written as zero
// (the caller lets nested encodings WITH parameters overwrite theirs afterwards)
template <typename T>
void encoding_parts_backward(hipStream_t stream, const EncodingParts& parts, uint32_t n, uint32_t n_input_dims, const T* dL_dy, uint32_t stride_k, uint32_t stride_i,
                             const float* in, uint32_t in_stride_i, uint32_t in_stride_d, float* dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_d);

// composite.h:47-133.  to_reduce / dL_dunreduced: n_to_reduce blocks of `width` rows, element (row r, sample i) at [r * stride_k + i * stride_i];
// reduced / dL_dreduced: `width` rows with their own strides.  fp32 accumulation in nested order, rounded to T at the store.
template <typename T>
void reduce_forward(hipStream_t stream, bool product, uint32_t n, uint32_t width, uint32_t n_to_reduce, const T* to_reduce, uint32_t stride_k, uint32_t stride_i,
                    T* reduced, uint32_t reduced_stride_k, uint32_t reduced_stride_i);
template <typename T>
void reduce_backward(hipStream_t stream, bool product, uint32_t n, uint32_t width, uint32_t n_to_reduce, const T* to_reduce, T* dL_dunreduced, uint32_t stride_k,
                     uint32_t stride_i, const T* dL_dreduced, uint32_t reduced_stride_k, uint32_t reduced_stride_i);

}  // namespace tcnn_hip

// grid_second_order.hip -- the input gradient dL_dx = sum_k dL_dy[k] * dy_dx[k] and the second-order passes through it (the parameter part
// of the second order is grid_backward() with io.ddx set: grid_backward_scatter.hip).
#include "grid_device.h"

namespace tcnn_hip {

template <typename GRAD_T>
__global__ void k_grid_backward_input(uint32_t n_dims, uint32_t n_features, GridIO io, const GRAD_T* __restrict__ dL_dy,
                                      const float* __restrict__ dy_dx, float* __restrict__ dL_dx, uint32_t dx_stride_i,
                                      uint32_t dx_stride_d) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= io.n) return;
	float result[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	for (uint32_t k = 0; k < n_features; ++k) {
		const float dl = (float)dL_dy[(size_t)k * io.stride_k + (size_t)i * io.stride_i];
		for (uint32_t d = 0; d < n_dims; ++d) {
			const float t = dl * dy_dx[((size_t)k * io.n + i) * n_dims + d];
			result[d] = result[d] + t;
		}
	}
	for (uint32_t d = 0; d < n_dims; ++d) dL_dx[(size_t)i * dx_stride_i + (size_t)d * dx_stride_d] = result[d];
}

// second order w.r.t. dL_dy: dL_ddLdy[k][i] = sum_d dy_dx[k][i][d] * ddx[i][d]  (grid.h:623-653)
__global__ void k_grid_backward_backward_dLdoutput(uint32_t n_dims, uint32_t n_features, uint32_t n_to_pad, GridIO io, const float* __restrict__ dy_dx,
                                                   half_t* __restrict__ dL_ddLdy) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= io.n) return;
	float dd[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	for (uint32_t d = 0; d < n_dims; ++d) dd[d] = io.ddx[(size_t)i * io.ddx_stride_i + (size_t)d * io.ddx_stride_d];
	for (uint32_t k = 0; k < n_features; ++k) {
		float result = 0.0f;
		for (uint32_t d = 0; d < n_dims; ++d) result += dy_dx[((size_t)k * io.n + i) * n_dims + d] * dd[d];
		dL_ddLdy[(size_t)k * io.stride_k + (size_t)i * io.stride_i] = to_half_rn(result);
	}
	for (uint32_t k = n_features; k < n_features + n_to_pad; ++k) dL_ddLdy[(size_t)k * io.stride_k + (size_t)i * io.stride_i] = (half_t)0.0f;
}

// the same for an fp32 encoding (T = float): the fp32 sum is stored as it is, padded columns are fp32 zeros
__global__ void k_grid_backward_backward_dLdoutput_f32(uint32_t n_dims, uint32_t n_features, uint32_t n_to_pad, GridIO io, const float* __restrict__ dy_dx,
                                                       float* __restrict__ dL_ddLdy) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= io.n) return;
	float dd[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	for (uint32_t d = 0; d < n_dims; ++d) dd[d] = io.ddx[(size_t)i * io.ddx_stride_i + (size_t)d * io.ddx_stride_d];
	for (uint32_t k = 0; k < n_features; ++k) {
		float result = 0.0f;
		for (uint32_t d = 0; d < n_dims; ++d) result += dy_dx[((size_t)k * io.n + i) * n_dims + d] * dd[d];
		dL_ddLdy[(size_t)k * io.stride_k + (size_t)i * io.stride_i] = result;
	}
	for (uint32_t k = n_features; k < n_features + n_to_pad; ++k) dL_ddLdy[(size_t)k * io.stride_k + (size_t)i * io.stride_i] = 0.0f;
}

// second order w.r.t. the positions (grid.h:457-620).  With v(corner) = sum_f grid[corner][f] * dL_dy[f] and s_d = +-1
// (right / left corner along d):
//   dL_dx[a] = scale^2 * ( ddx[a] * pos''(a) * sum_c s_a prod_{e != a} w_e v(c)                           (Smoothstep only)
//                        + sum_{b != a} ddx[b] * pos'(b) * pos'(a) * sum_c s_a s_b prod_{e != a, b} w_e v(c) )
// summed over the levels; one thread per sample walks the levels (no atomics, fixed order).  One body for both value types: T = half_t is
// the 16-bit encoding's kernel, T = float the fp32 encoding's (kernel_grid_backward_input_backward_input<float>: fp32 features, one 8-byte
// load per corner at F = 2, 16-byte loads from F = 4 on, and an fp32 dL_dy).  The fp32 form also takes the two differences that would
// subtract a rounded value in a form that does not (second_order_weights_f32, pos'' = 12 * (0.5 - t)): its results are held to bars
// relative to the plain magnitudes of their terms (tests/second_order_f32_cases.py).
template <uint32_t D, uint32_t F, typename T>
TCNN_DEVICE void backward_backward_input_sample(const GridMeta& meta, const GridIO& io, uint32_t i, const T* __restrict__ dL_dy, const T* __restrict__ params,
                                                float* __restrict__ dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_d) {
	constexpr uint32_t N_CORNERS = 1u << D;
	constexpr bool FP32 = std::is_same<T, float>::value;
	float x[D], dd[D], out[D];
	load_position<D>(io, i, x);
	load_ddx<D>(io, i, dd);
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) out[d] = 0.0f;
	const bool nearest = meta.interp == (uint32_t)InterpolationType::Nearest;
	const float max_level = io.max_level ? io.max_level[i] : meta.max_level;  // per sample where the array is set (it wins, grid.h:70-72)
	for (uint32_t level = 0; level < meta.n_levels && !nearest; ++level) {
		if (level_is_off<false>(meta, max_level, level, F)) break;
		const Level<D> lv = make_level<D>(meta, level);
		const T* __restrict__ grid = params + (size_t)meta.offset[level] * F;
		Cell<D> c = make_cell<D, false>(lv, x);
		if constexpr (FP32) second_order_weights_f32<D>(lv, x, c);
		float d2[D];  // pos''(d): 0 for Linear, smoothstep'' = 6 - 12 t otherwise (common_device.h:1012-1014)
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			float p = __builtin_fmaf(lv.scale, x[d], 0.5f);
			p -= __builtin_floorf(p);
			if constexpr (FP32) {
				d2[d] = lv.smooth ? 12.0f * (0.5f - p) : 0.0f;  // 0.5 - t is one rounding of the exact fraction; 6 - 12 t subtracts a rounded 12 t
			} else {
				d2[d] = lv.smooth ? 6.0f - 12.0f * p : 0.0f;
			}
		}
		float gy[F];
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) gy[f] = (float)dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
		float v[N_CORNERS];
#pragma unroll
		for (uint32_t idx = 0; idx < N_CORNERS; ++idx) {
			const T* __restrict__ entry = grid + (size_t)corner_index<D, false>(lv, c, idx) * F;
			float acc = 0.0f;
			if constexpr (FP32) {
				float val[F];
				load_features<F>(entry, val);
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) acc += val[f] * gy[f];
			} else {
				h2 val[(F + 1) / 2];
				load_features<F>(entry, val);
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) acc += (float)val[f / 2][f % 2] * gy[f];
			}
			v[idx] = acc;
		}
		const float s2 = lv.scale * lv.scale;
#pragma unroll
		for (uint32_t a = 0; a < D; ++a) {
			float grad_out = 0.0f;
#pragma unroll
			for (uint32_t idx = 0; idx < N_CORNERS; ++idx) {
				const float sa = ((idx >> a) & 1u) ? 1.0f : -1.0f;
				if (lv.smooth) {  // diagonal of the Hessian
					float wgt = s2 * dd[a] * d2[a] * sa;
#pragma unroll
					for (uint32_t e = 0; e < D; ++e) {
						if (e != a) wgt *= ((idx >> e) & 1u) ? c.w[e][1] : c.w[e][0];
					}
					grad_out += wgt * v[idx];
				}
#pragma unroll
				for (uint32_t b = 0; b < D; ++b) {  // mixed terms
					if (b == a) continue;
					float wgt = s2 * dd[b] * c.derivative[b] * c.derivative[a] * sa * (((idx >> b) & 1u) ? 1.0f : -1.0f);
#pragma unroll
					for (uint32_t e = 0; e < D; ++e) {
						if (e != a && e != b) wgt *= ((idx >> e) & 1u) ? c.w[e][1] : c.w[e][0];
					}
					grad_out += wgt * v[idx];
				}
			}
			out[a] += grad_out;
		}
	}
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) dL_dx[(size_t)i * dx_stride_i + (size_t)d * dx_stride_d] = out[d];
}

template <uint32_t D, uint32_t F>
__global__ void __launch_bounds__(128) k_grid_backward_backward_input(const GridMeta meta, const GridIO io, const half_t* __restrict__ dL_dy,
                                                                       const half_t* __restrict__ params, float* __restrict__ dL_dx,
                                                                       uint32_t dx_stride_i, uint32_t dx_stride_d) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= io.n) return;
	backward_backward_input_sample<D, F, half_t>(meta, io, i, dL_dy, params, dL_dx, dx_stride_i, dx_stride_d);
}

template <uint32_t D, uint32_t F>
__global__ void __launch_bounds__(128) k_grid_backward_backward_input_f32(const GridMeta meta, const GridIO io, const float* __restrict__ dL_dy,
                                                                           const float* __restrict__ params, float* __restrict__ dL_dx,
                                                                           uint32_t dx_stride_i, uint32_t dx_stride_d) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= io.n) return;
	backward_backward_input_sample<D, F, float>(meta, io, i, dL_dy, params, dL_dx, dx_stride_i, dx_stride_d);
}

void grid_backward_input(hipStream_t stream, uint32_t n_dims, uint32_t n_features, const GridIO& io, const half_t* dL_dy,
                         const float* dy_dx, float* dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_d) {
	if (io.n == 0) return;
	TCNN_LAUNCH(k_grid_backward_input<half_t>, dim3(div_round_up(io.n, 128u)), dim3(128), 0, stream, n_dims, n_features, io, dL_dy, dy_dx,
	            dL_dx, dx_stride_i, dx_stride_d);
}

void grid_backward_input(hipStream_t stream, uint32_t n_dims, uint32_t n_features, const GridIO& io, const float* dL_dy, const float* dy_dx, float* dL_dx,
                             uint32_t dx_stride_i, uint32_t dx_stride_d) {
	if (io.n == 0) return;
	TCNN_LAUNCH(k_grid_backward_input<float>, dim3(div_round_up(io.n, 128u)), dim3(128), 0, stream, n_dims, n_features, io, dL_dy, dy_dx, dL_dx, dx_stride_i,
	            dx_stride_d);
}

void grid_backward_backward_dLdoutput(hipStream_t stream, uint32_t n_dims, uint32_t n_features, uint32_t n_to_pad, const GridIO& io,
                                      const float* dy_dx, half_t* dL_ddLdy) {
	if (io.n == 0) return;
	if (!io.ddx || !dy_dx) throw std::runtime_error("grid second-order pass: dL_ddLdinput and the forward's dy_dx are required");
	TCNN_LAUNCH(k_grid_backward_backward_dLdoutput, dim3(div_round_up(io.n, 128u)), dim3(128), 0, stream, n_dims, n_features, n_to_pad, io, dy_dx, dL_ddLdy);
}

void grid_backward_backward_input(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* dL_dy, const half_t* params,
                                  float* dL_dx, uint32_t dx_stride_i, uint32_t dx_stride_d) {
	if (io.n == 0) return;
	if (!io.ddx) throw std::runtime_error("grid second-order pass: dL_ddLdinput is required");
	const uint32_t blocks = div_round_up(io.n, 128u);
	grid_dispatch(meta, [&](auto D, auto F) {
		TCNN_LAUNCH((k_grid_backward_backward_input<D, F>), dim3(blocks), dim3(128), 0, stream, meta, io, dL_dy, params, dL_dx, dx_stride_i, dx_stride_d);
	});
}

void grid_backward_backward_dLdoutput(hipStream_t stream, uint32_t n_dims, uint32_t n_features, uint32_t n_to_pad, const GridIO& io, const float* dy_dx,
                                      float* dL_ddLdy) {
	if (io.n == 0) return;
	if (!io.ddx || !dy_dx) throw std::runtime_error("grid second-order pass: dL_ddLdinput and the forward's dy_dx are required");
	TCNN_LAUNCH(k_grid_backward_backward_dLdoutput_f32, dim3(div_round_up(io.n, 128u)), dim3(128), 0, stream, n_dims, n_features, n_to_pad, io, dy_dx, dL_ddLdy);
}

void grid_backward_backward_input(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* dL_dy, const float* params, float* dL_dx,
                                      uint32_t dx_stride_i, uint32_t dx_stride_d) {
	if (io.n == 0) return;
	if (!io.ddx) throw std::runtime_error("grid second-order pass: dL_ddLdinput is required");
	const uint32_t blocks = div_round_up(io.n, 128u);
	grid_dispatch(meta, [&](auto D, auto F) {
		TCNN_LAUNCH((k_grid_backward_backward_input_f32<D, F>), dim3(blocks), dim3(128), 0, stream, meta, io, dL_dy, params, dL_dx, dx_stride_i, dx_stride_d);
	});
}

}  // namespace tcnn_hip

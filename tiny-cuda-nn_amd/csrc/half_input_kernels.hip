// half_input_kernels.hip -- see half_input_kernels.h.  Two HBM streams that transpose through LDS: the caller's matrix is sample-major
// [n][n_dims], the network kernels' input and input-gradient matrices are feature-major [padded][n].  A workgroup moves a tile of 256
// samples x up to 64 features (one 128-byte line per sample on the caller's side, one 512-byte run per feature on the network's):
// 16-byte global accesses wherever the pointers and widths allow them, all of a lane's global loads issued before its first LDS store,
// 2-byte accesses otherwise.  No arithmetic, no templates: the widths are run-time values and an element is 16 bits of either type.
#include "half_input_kernels.h"

#include <stdexcept>

namespace tcnn_hip {

typedef uint16_t w4 __attribute__((ext_vector_type(4)));
typedef uint16_t w8 __attribute__((ext_vector_type(8)));

constexpr uint32_t HI_THREADS = 256;
constexpr uint32_t HI_TILE = 256;                               // samples per workgroup
constexpr uint32_t HI_CHUNK = 64;                               // features per workgroup
constexpr uint32_t HI_LD = HI_TILE + 4;                         // row pitch of the LDS tile [feature][sample]: 8-byte aligned rows, 2 banks apart
constexpr uint32_t HI_VEC = 8;                                  // elements of a 16-byte access
constexpr uint32_t HI_LOADS = HI_TILE * HI_CHUNK / HI_VEC / HI_THREADS;  // 16-byte accesses per lane that cover a full tile: 8

TCNN_DEVICE bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0u; }
TCNN_DEVICE w8 join8(w4 a, w4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }

// The sample-major side of a tile: element (sample s, feature j) of the block at g[s * n_dims + j], s < rows, j < kr.
//   ROWS8: n_dims is a multiple of 8 and g is 16-byte aligned -- a lane moves 8 features of one sample;
//   RUN8:  the block covers whole rows (kr == n_dims), so its elements are ONE contiguous run, 16-byte aligned and a multiple of 8 long -- a
//          lane moves 8 consecutive elements of the run, which may cross from one sample to the next (n_dims = 3, 20, ...);
//   otherwise 2 bytes at a time.
enum : uint32_t { HI_SCALAR = 0, HI_ROWS8 = 1, HI_RUN8 = 2 };
TCNN_DEVICE uint32_t sample_major_mode(const void* g, uint32_t rows, uint32_t n_dims, uint32_t kr) {
	if (kr == 0u || !aligned16(g)) return HI_SCALAR;
	if (n_dims % HI_VEC == 0u) return HI_ROWS8;
	if (kr == n_dims && (rows * n_dims) % HI_VEC == 0u) return HI_RUN8;
	return HI_SCALAR;
}

__global__ void __launch_bounds__(HI_THREADS) k_half_input_pad(uint32_t n, uint32_t n_dims, uint32_t padded, const uint16_t* __restrict__ in,
                                                                uint16_t* __restrict__ out, uint16_t pad_bits) {
	__shared__ __attribute__((aligned(16))) uint16_t tile[HI_CHUNK * HI_LD];
	const uint32_t first = blockIdx.x * HI_TILE, rows = min(HI_TILE, n - first);
	const uint32_t k0 = blockIdx.y * HI_CHUNK, kw = min(HI_CHUNK, padded - k0);  // the rows of `out` this block writes ...
	const uint32_t kr = k0 < n_dims ? min(kw, n_dims - k0) : 0u;                  // ... and how many of them come from `in`
	const uint16_t* src = in + (size_t)first * n_dims + k0;
	const uint32_t mode = sample_major_mode(src, rows, n_dims, kr);
	if (mode == HI_SCALAR) {
		for (uint32_t e = threadIdx.x; e < rows * kr; e += HI_THREADS) {
			const uint32_t s = e / kr, j = e - s * kr;
			tile[j * HI_LD + s] = src[(size_t)s * n_dims + j];
		}
	} else {
		const uint32_t per_row = mode == HI_ROWS8 ? kr / HI_VEC : 1u, total = rows * kr / HI_VEC;  // <= HI_LOADS * HI_THREADS
		w8 v[HI_LOADS];
#pragma unroll
		for (uint32_t it = 0; it < HI_LOADS; ++it) {
			const uint32_t e8 = threadIdx.x + it * HI_THREADS;
			if (e8 < total) {
				const size_t offset = mode == HI_ROWS8 ? (size_t)(e8 / per_row) * n_dims + HI_VEC * (e8 % per_row) : (size_t)HI_VEC * e8;
				v[it] = *(const w8*)(src + offset);
			}
		}
#pragma unroll
		for (uint32_t it = 0; it < HI_LOADS; ++it) {
			const uint32_t e8 = threadIdx.x + it * HI_THREADS;
			if (e8 < total) {
				uint32_t s, j;  // of the lane's first element; RUN8: kr == n_dims
				if (mode == HI_ROWS8) {
					s = e8 / per_row;
					j = HI_VEC * (e8 % per_row);
				} else {
					s = HI_VEC * e8 / kr;
					j = HI_VEC * e8 - s * kr;
				}
#pragma unroll
				for (uint32_t q = 0; q < HI_VEC; ++q) {
					tile[j * HI_LD + s] = v[it][q];
					if (++j == kr) {  // (ROWS8: the 8 features end at the row's end at the latest, and nothing follows)
						j = 0;
						++s;
					}
				}
			}
		}
	}
	__syncthreads();
	uint16_t* dst = out + (size_t)k0 * n + first;  // (feature k, sample s) of the block at dst[k * n + s]
	if (rows == HI_TILE && n % HI_VEC == 0u && aligned16(out)) {  // eight samples of one feature per lane
		const w4 pad4 = w4{pad_bits, pad_bits, pad_bits, pad_bits};
		for (uint32_t e8 = threadIdx.x; e8 < kw * (HI_TILE / HI_VEC); e8 += HI_THREADS) {
			const uint32_t k = e8 / (HI_TILE / HI_VEC), s = HI_VEC * (e8 % (HI_TILE / HI_VEC));
			const uint16_t* t = tile + k * HI_LD + s;
			*(w8*)(dst + (size_t)k * n + s) = k < kr ? join8(*(const w4*)t, *(const w4*)(t + 4)) : join8(pad4, pad4);
		}
	} else {
		for (uint32_t e = threadIdx.x; e < kw * HI_TILE; e += HI_THREADS) {
			const uint32_t k = e / HI_TILE, s = e % HI_TILE;
			if (s < rows) dst[(size_t)k * n + s] = k < kr ? tile[k * HI_LD + s] : pad_bits;
		}
	}
}

__global__ void __launch_bounds__(HI_THREADS) k_half_input_unpad(uint32_t n, uint32_t n_dims, const uint16_t* __restrict__ dL_dy, uint16_t* __restrict__ dL_dx) {
	__shared__ __attribute__((aligned(16))) uint16_t tile[HI_CHUNK * HI_LD];
	const uint32_t first = blockIdx.x * HI_TILE, rows = min(HI_TILE, n - first);
	const uint32_t k0 = blockIdx.y * HI_CHUNK, kr = min(HI_CHUNK, n_dims - k0);  // the features this block moves (the grid covers n_dims, not the padding)
	const uint16_t* src = dL_dy + (size_t)k0 * n + first;  // (feature k, sample s) of the block at src[k * n + s]
	if (rows == HI_TILE && n % HI_VEC == 0u && aligned16(dL_dy)) {  // eight samples of one feature per lane
		const uint32_t total = kr * (HI_TILE / HI_VEC);  // <= HI_LOADS * HI_THREADS
		w8 v[HI_LOADS];
#pragma unroll
		for (uint32_t it = 0; it < HI_LOADS; ++it) {
			const uint32_t e8 = threadIdx.x + it * HI_THREADS;
			if (e8 < total) v[it] = *(const w8*)(src + (size_t)(e8 / (HI_TILE / HI_VEC)) * n + HI_VEC * (e8 % (HI_TILE / HI_VEC)));
		}
#pragma unroll
		for (uint32_t it = 0; it < HI_LOADS; ++it) {
			const uint32_t e8 = threadIdx.x + it * HI_THREADS;
			if (e8 < total) {
				uint16_t* t = tile + (e8 / (HI_TILE / HI_VEC)) * HI_LD + HI_VEC * (e8 % (HI_TILE / HI_VEC));
				*(w4*)t = __builtin_shufflevector(v[it], v[it], 0, 1, 2, 3);
				*(w4*)(t + 4) = __builtin_shufflevector(v[it], v[it], 4, 5, 6, 7);
			}
		}
	} else {
		for (uint32_t e = threadIdx.x; e < kr * HI_TILE; e += HI_THREADS) {
			const uint32_t k = e / HI_TILE, s = e % HI_TILE;
			if (s < rows) tile[k * HI_LD + s] = src[(size_t)k * n + s];
		}
	}
	__syncthreads();
	uint16_t* dst = dL_dx + (size_t)first * n_dims + k0;  // (sample s, feature j) of the block at dst[s * n_dims + j]
	const uint32_t mode = sample_major_mode(dst, rows, n_dims, kr);
	if (mode == HI_SCALAR) {
		for (uint32_t e = threadIdx.x; e < rows * kr; e += HI_THREADS) {
			const uint32_t s = e / kr, j = e - s * kr;
			dst[(size_t)s * n_dims + j] = tile[j * HI_LD + s];
		}
		return;
	}
	const uint32_t per_row = mode == HI_ROWS8 ? kr / HI_VEC : 1u, total = rows * kr / HI_VEC;
	for (uint32_t e8 = threadIdx.x; e8 < total; e8 += HI_THREADS) {
		uint32_t s, j;
		size_t offset;
		if (mode == HI_ROWS8) {
			s = e8 / per_row;
			j = HI_VEC * (e8 % per_row);
			offset = (size_t)s * n_dims + j;
		} else {
			s = HI_VEC * e8 / kr;
			j = HI_VEC * e8 - s * kr;
			offset = (size_t)HI_VEC * e8;
		}
		w8 v;
#pragma unroll
		for (uint32_t q = 0; q < HI_VEC; ++q) {
			v[q] = tile[j * HI_LD + s];
			if (++j == kr) {
				j = 0;
				++s;
			}
		}
		*(w8*)(dst + offset) = v;
	}
}

void half_input_pad(hipStream_t stream, uint32_t n, uint32_t n_dims, uint32_t padded, const uint16_t* in, uint16_t* out, uint16_t pad_bits) {
	if (n == 0) return;
	if (n_dims == 0 || padded < n_dims) throw std::runtime_error("half_input_pad: the padded width is smaller than the input width");
	TCNN_LAUNCH(k_half_input_pad, dim3(div_round_up(n, HI_TILE), div_round_up(padded, HI_CHUNK)), dim3(HI_THREADS), 0, stream, n, n_dims, padded, in, out, pad_bits);
}

void half_input_unpad(hipStream_t stream, uint32_t n, uint32_t n_dims, const uint16_t* dL_dy, uint16_t* dL_dx) {
	if (n == 0 || n_dims == 0) return;
	TCNN_LAUNCH(k_half_input_unpad, dim3(div_round_up(n, HI_TILE), div_round_up(n_dims, HI_CHUNK)), dim3(HI_THREADS), 0, stream, n, n_dims, dL_dy, dL_dx);
}

}  // namespace tcnn_hip

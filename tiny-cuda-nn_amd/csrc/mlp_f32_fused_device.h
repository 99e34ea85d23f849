// mlp_f32_fused_device.h -- what the fused fp32 network kernels share (mlp_f32_fused.hip: forward / inference; mlp_f32_fused_backward.hip: the
// backward chain): the split of a workgroup over its tile of samples and the weights' LDS layout, both described in mlp_f32_fused.hip.
#pragma once
#include "mlp_kernels.h"

namespace tcnn_hip {

constexpr uint32_t F32F_THREADS = 512;
constexpr uint32_t F32F_WAVE_SAMPLES = 32;                 // two 16-column sample tiles
constexpr uint32_t F32F_PAD = 8;                           // floats between the end of a weight row and the next row in LDS
constexpr uint32_t F32F_RESIDENT_LDS_BYTES = 128u << 10;   // of the CU's 160 KiB
constexpr uint32_t F32F_MAX_BLOCKS = 512;                  // two workgroups per CU where LDS and registers allow
static_assert(F32F_THREADS / WAVE * F32F_WAVE_SAMPLES == MLP_F32_FUSED_TILE, "a workgroup's waves cover its tile");

// one weight matrix [rows][K], global -> LDS rows of K + F32F_PAD floats, 16 bytes per thread and step
TCNN_DEVICE void f32f_copy_matrix(float* dst, const float* src, uint32_t rows, uint32_t K) {
	const uint32_t chunks_per_row = K / 4u, chunks = rows * chunks_per_row;
	for (uint32_t c = threadIdx.x; c < chunks; c += F32F_THREADS) {
		const uint32_t row = c / chunks_per_row, kc = c % chunks_per_row;
		*(f4*)(dst + row * (K + F32F_PAD) + 4u * kc) = *(const f4*)(src + (size_t)row * K + 4u * kc);
	}
}

}  // namespace tcnn_hip

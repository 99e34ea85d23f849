// mlp_f32_fused_device.h -- what the fused fp32 network kernels share (mlp_f32_fused.hip: forward / inference; mlp_f32_fused_backward.hip: the
// backward chain and the weight gradients; mlp_f32_fused_second_order.hip: the second-order pass): the split of a workgroup over its tile of
// samples and the weights' LDS layout, both described in mlp_f32_fused.hip, and the weight-gradient kernel of all matrices, described in
// mlp_f32_fused_backward.hip.
#pragma once
#include "mlp_kernels.h"

#include <algorithm>

namespace tcnn_hip {

constexpr uint32_t F32F_THREADS = 512;
constexpr uint32_t F32F_WAVE_SAMPLES = 32;                 // two 16-column sample tiles
constexpr uint32_t F32F_PAD = 8;                           // floats between the end of a weight row and the next row in LDS
constexpr uint32_t F32F_RESIDENT_LDS_BYTES = 128u << 10;   // of the CU's 160 KiB
#ifndef TCNN_F32F_MAX_BLOCKS
#define TCNN_F32F_MAX_BLOCKS 512                           // (the host emulator's build sets 2: uneven shares of the persistent tile loop)
#endif
constexpr uint32_t F32F_MAX_BLOCKS = TCNN_F32F_MAX_BLOCKS; // two workgroups per CU where LDS and registers allow
static_assert(F32F_THREADS / WAVE * F32F_WAVE_SAMPLES == MLP_F32_FUSED_TILE, "a workgroup's waves cover its tile");

// one weight matrix [rows][K], global -> LDS rows of K + F32F_PAD floats, 16 bytes per thread and step
TCNN_DEVICE void f32f_copy_matrix(float* dst, const float* src, uint32_t rows, uint32_t K) {
	const uint32_t chunks_per_row = K / 4u, chunks = rows * chunks_per_row;
	for (uint32_t c = threadIdx.x; c < chunks; c += F32F_THREADS) {
		const uint32_t row = c / chunks_per_row, kc = c % chunks_per_row;
		*(f4*)(dst + row * (K + F32F_PAD) + 4u * kc) = *(const f4*)(src + (size_t)row * K + 4u * kc);
	}
}

// floats of LDS with every matrix resident / of the staging buffer (the largest matrix): the forward matrices (params) ...
inline uint32_t f32f_resident_floats(const MlpMeta& m) {
	return m.width * (m.in_width + F32F_PAD) + (m.n_hidden_matmuls * m.width + m.padded_out) * (m.width + F32F_PAD);
}
inline uint32_t f32f_staged_floats(const MlpMeta& m) {
	return std::max(m.width * (m.in_width + F32F_PAD), std::max(m.width, m.padded_out) * (m.width + F32F_PAD));
}
// ... and the transposed ones (params_t), the input matrix only where dL_dinput is computed
inline uint32_t f32b_resident_floats(const MlpMeta& m, bool want_dx) {
	return m.width * (m.padded_out + F32F_PAD) + (m.n_hidden_matmuls * m.width + (want_dx ? m.in_width : 0u)) * (m.width + F32F_PAD);
}
inline uint32_t f32b_staged_floats(const MlpMeta& m, bool want_dx) {
	return std::max(m.width * (m.padded_out + F32F_PAD), std::max(m.width, want_dx ? m.in_width : 0u) * (m.width + F32F_PAD));
}

// the chain kernel of mlp_f32_fused_backward alone: dL_doutput -> D_j (to dact [n_hidden][n][W], or null) -> dL_dinput (or null), the hidden
// activation's derivative taken at `at` [n_hidden][n][W]
void mlp_f32_fused_backward_chain(hipStream_t stream, const MlpMeta& m, uint32_t n, const float* params_t, const float* at, const float* dL_doutput, float* dL_dinput,
                                  float* dact);

// ---- weight gradients (mlp_f32_fused_backward.hip, 2.) ---------------------------------------------------------------------------------
constexpr uint32_t F32G_THREADS = 512;
constexpr uint32_t F32G_BS = 32;                  // samples per LDS stage
constexpr uint32_t F32G_LDF = F32G_BS + 4;        // row stride of the feature-major stage [feature][sample]
constexpr uint32_t F32G_TARGET_BLOCKS = 1024;     // (matrices x slices) to aim for: four workgroups per CU
static_assert(MLP_F32_FUSED_TILE % F32G_BS == 0, "a sample tile is a whole number of stages");

// row stride of a sample-major stage [sample][width]: the four rows of a "samples in k" read 16 banks apart, and room for the second tile of
// a wave's 2 x 2 block where the matrix has an odd number of tiles
TCNN_HOST_DEVICE uint32_t f32g_ld(uint32_t width) { return next_multiple(width, 32u) + 16u; }

struct F32WgradArgs {
	static constexpr bool DUAL = false;
	MlpMeta m;
	uint32_t n, n_slices;
	uint32_t stage_floats;    // of one LDS stage: the largest matrix's operand pair
	const float* dact;        // [n_hidden][n][W] D_j
	const float* dL_doutput;  // [n][padded_out]
	const float* hidden;      // [n_hidden][n][W] post-activations
	const float* input;       // feature-major [in_width][n]
	float* partials;          // [n_slices][n_params]
};
// the second-order pass (mlp_f32_fused_second_order.hip, 3.): every matrix sums TWO products over its slice, d (x) a of the four operands
// above (there: d_j, g, u_j, v) and then, per stage, the second pair below (c_j, c_out, a_j, x).  dact2 == nullptr: no second pair at all
// (stage_floats is then one pair's); dL_doutput2 == nullptr: none for the output matrix.
struct F32WgradDualArgs : F32WgradArgs {
	static constexpr bool DUAL = true;
	const float* dact2;
	const float* dL_doutput2;
	const float* hidden2;
	const float* input2;
};

template <typename ARGS>
__global__ void __launch_bounds__(F32G_THREADS) k_mlp_f32_wgrad_all(const ARGS p) {
	constexpr uint32_t BS = F32G_BS, LDF = F32G_LDF, CS = BS / 4u;
	constexpr bool DUAL = ARGS::DUAL;
	constexpr uint32_t NP = DUAL ? 2u : 1u;
	TCNN_DYN_LDS(lds_raw);
	float* lds = (float*)lds_raw;

	const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63u, lr = lane & 15u, g = lane >> 4;
	const uint32_t W = p.m.width, IN = p.m.in_width, HM = p.m.n_hidden_matmuls, OUTP = p.m.padded_out;
	const uint32_t n_matrices = HM + 2u, mi = blockIdx.x % n_matrices, slice = blockIdx.x / n_matrices;
	const size_t n = p.n, layer_elems = n * W;
	// this item's matrix [WO][WI] (uniform)
	const bool fm = mi == 0u, out = mi == HM + 1u;
	const uint32_t WO = out ? OUTP : W, WI = fm ? IN : W;
	const float* d[NP];       // sample-major [n][WO]
	const float* av_src[NP];  // feature-major [IN][n], or sample-major [n][W]
	d[0] = out ? p.dL_doutput : p.dact + mi * layer_elems;
	av_src[0] = fm ? p.input : p.hidden + (mi - 1u) * layer_elems;
	bool second = false;  // (uniform)
	if constexpr (DUAL) {
		second = p.dact2 != nullptr && (!out || p.dL_doutput2 != nullptr);
		d[1] = out ? p.dL_doutput2 : p.dact2 + mi * layer_elems;
		av_src[1] = fm ? p.input2 : p.hidden2 + (mi - 1u) * layer_elems;
	}
	const size_t offset = fm ? 0u : (size_t)W * IN + (size_t)(mi - 1u) * W * W;
	const uint32_t ldd = f32g_ld(WO), lda = f32g_ld(WI);
	const uint32_t ckd = WO / 4u, d_chunks = BS * ckd;                    // 16-byte chunks of a stage: <= 512
	const uint32_t cka = WI / 4u, a_chunks = fm ? WI * CS : BS * cka;      // <= 1024 (feature-major), <= 512
	const uint32_t pair_floats = BS * ldd + (fm ? next_multiple(WI, 32u) * LDF : BS * lda);  // (the second pair lies behind the first)

	// this wave's 2 x 2 block of 16 x 16 tiles
	const uint32_t nbi = div_round_up(WI, 32u), wo = w / nbi, wi = w % nbi;
	const bool active = 32u * wo < WO;  // (uniform per wave)
	// the tiles of slice s: [s T / S, (s + 1) T / S), in stages of BS samples
	const uint32_t n_tiles = p.n / MLP_F32_FUSED_TILE, per_tile = MLP_F32_FUSED_TILE / BS;
	const uint32_t t_begin = (uint32_t)((uint64_t)slice * n_tiles / p.n_slices) * per_tile, t_end = (uint32_t)((uint64_t)(slice + 1u) * n_tiles / p.n_slices) * per_tile;

	f4 dreg[NP], areg[NP][2];
	auto load = [&](uint32_t t) {
		const size_t s = (size_t)t * BS;
#pragma unroll
		for (uint32_t k = 0; k < NP; ++k) {
			if (k == 1u && !second) break;
			if (tid < d_chunks) dreg[k] = *(const f4*)(d[k] + (s + tid / ckd) * WO + 4u * (tid % ckd));
#pragma unroll
			for (uint32_t q = 0; q < 2; ++q) {
				const uint32_t c = tid + q * F32G_THREADS;
				if (c < a_chunks) {
					areg[k][q] = fm ? *(const f4*)(av_src[k] + (size_t)(c / CS) * n + s + 4u * (c % CS)) : *(const f4*)(av_src[k] + (s + c / cka) * W + 4u * (c % cka));
				}
			}
		}
	};
	auto store = [&](float* stage) {
#pragma unroll
		for (uint32_t k = 0; k < NP; ++k) {
			if (k == 1u && !second) break;
			float* dT = stage + k * pair_floats;
			float* aT = dT + BS * ldd;
			if (tid < d_chunks) *(f4*)(dT + (tid / ckd) * ldd + 4u * (tid % ckd)) = dreg[k];
#pragma unroll
			for (uint32_t q = 0; q < 2; ++q) {
				const uint32_t c = tid + q * F32G_THREADS;
				if (c < a_chunks) *(f4*)(aT + (fm ? (c / CS) * LDF + 4u * (c % CS) : (c / cka) * lda + 4u * (c % cka))) = areg[k][q];
			}
		}
	};
	// "samples in k": step q of a stage is samples 4 q + g.  d: row 4 q + g, column = this lane's row of the tile; a: the same (sample-major)
	// or row = this lane's feature, column 4 q + g (feature-major).  Tiles past the matrix read staged or unwritten LDS inside the stage and
	// are not stored.
	const uint32_t d_at = g * ldd + 32u * wo + lr, d_step = 4u * ldd;
	const uint32_t a_at = fm ? (32u * wi + lr) * LDF + g : g * lda + 32u * wi + lr, a_step = fm ? 4u : 4u * lda, a_tile = fm ? 16u * LDF : 16u;

	f4 acc[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
	load(t_begin);
	store(lds);
	__syncthreads();
	for (uint32_t t = t_begin; t < t_end; ++t) {
		const float* stage = lds + ((t - t_begin) & 1u) * p.stage_floats;
		const bool more = t + 1u < t_end;
		if (more) load(t + 1u);
		if (active) {
#pragma unroll
			for (uint32_t k = 0; k < NP; ++k) {
				if (k == 1u && !second) break;
				const float* dT = stage + k * pair_floats;
				const float* aT = dT + BS * ldd;
#pragma unroll
				for (uint32_t q = 0; q < BS / 4u; ++q) {
					float av[2], bv[2];
#pragma unroll
					for (uint32_t b = 0; b < 2; ++b) {
						av[b] = dT[d_at + q * d_step + 16u * b];
						bv[b] = aT[a_at + q * a_step + b * a_tile];
					}
#pragma unroll
					for (uint32_t oi = 0; oi < 2; ++oi)
#pragma unroll
						for (uint32_t ii = 0; ii < 2; ++ii) acc[oi][ii] = mfma_16x16x4_f32(av[oi], bv[ii], acc[oi][ii]);
				}
			}
		}
		if (more) store(lds + ((t + 1u - t_begin) & 1u) * p.stage_floats);
		__syncthreads();
	}

	// this slice's slab, parameter order; accumulator element r <-> (out = 4 g + r, in = lr) of its 16 x 16 tile
	float* P = p.partials + (size_t)slice * p.m.n_params() + offset;
#pragma unroll
	for (uint32_t oi = 0; oi < 2; ++oi) {
#pragma unroll
		for (uint32_t ii = 0; ii < 2; ++ii) {
			const uint32_t ob = 32u * wo + 16u * oi, ib = 32u * wi + 16u * ii;
			f4 v = acc[oi][ii];
			mfma_settle(v);  // read on the far side of the branch below
			if (active && ob < WO && ib < WI) {
#pragma unroll
				for (uint32_t r = 0; r < 4; ++r) P[(size_t)(ob + 4u * g + r) * WI + ib + lr] = v[r];
			}
		}
	}
}

// one LDS stage of the largest matrix's operand pair: d [BS][ld] and a [BS][ld], or a feature-major [features in whole 2 x 2 blocks][LDF]
inline uint32_t f32g_stage_floats(const MlpMeta& m) {
	const uint32_t input = F32G_BS * f32g_ld(m.width) + std::max(F32G_BS * f32g_ld(m.in_width), next_multiple(m.in_width, 32u) * F32G_LDF);
	const uint32_t others = F32G_BS * f32g_ld(std::max(m.width, m.padded_out)) + F32G_BS * f32g_ld(m.width);
	return std::max(input, others);
}

}  // namespace tcnn_hip

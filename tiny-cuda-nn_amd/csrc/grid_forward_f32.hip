// grid_forward_f32.hip -- the tiled forward gather of an fp32 grid encoding, with and without dy_dx: what every eikonal step (the input
// requires a gradient) and every fp32 inference runs.  The design is the 16-bit gather's (grid_forward.hip says what bounds it: the L2's
// line rate, which an fp32 table -- twice the bytes per entry -- feels more):
//   * work split: grid_forward_plan.h's ForwardPlan with the table bytes of float entries -- (level, tile) items level-major, cut into eight
//     runs of equal cost, block b serves run b & 7, so an XCD keeps its one to three tables hot in its private L2; a workgroup finds its item
//     in one round of scalar loads (forward_plan_item);
//   * loads: a thread owns SPT samples of ONE level, computes their cells and issues every corner load -- 2^D * SPT accesses of 4 / 8 / 16
//     bytes, two of 16 at F = 8 -- before the first use.  SPT is 2 while a thread then holds at most 64 corner floats, 1 beyond (DESIGN.md
//     lists registers and occupancy per instance; none uses scratch);
//   * arithmetic: k_grid_forward_f32's, statement for statement (corner_weight, the corner order, result = fmaf(weight, value, result),
//     accumulate_dy_dx) -- the same bits as that kernel and the oracle's fp32 restatement;
//   * stores: features through io.stride_k / io.stride_i (either layout); a lane's D floats of dy_dx[((level * F + f) * n + i) * D + d] as ONE
//     8 / 12 / 16-byte store per feature, contiguous across the wave.  No LDS;
//   * a level the scalar max_level switches off loads nothing from the table and stores zeros (features and dy_dx rows).
// Not taken, and left to k_grid_forward_f32 by the fp32 grid_forward(): a per-sample max_level, Nearest, a null `out`, parameters off a
// 16-byte boundary.  Not part of the host emulator's build, which runs that kernel at every form.
#include "grid_forward_plan.h"
#include "switches.h"

namespace tcnn_hip {

// samples per thread: two while their corner values fit 64 registers (D = 4, F = 8 alone holds 128 per sample)
constexpr uint32_t f32_forward_spt(uint32_t D, uint32_t F) { return (F << D) <= 32u ? 2u : 1u; }

// the D floats of sample i in one row of dy_dx (`row` = dy_dx + k * n * D, wave-uniform), as one store
template <uint32_t D>
TCNN_DEVICE void store_dy_dx(float* __restrict__ row, uint32_t n, uint32_t i, const float (&g)[D]) {
	if constexpr (D == 2) {
		*(f2*)(row + (size_t)i * 2u) = f2{g[0], g[1]};
	} else if constexpr (D == 4) {
		*(f4*)(row + (size_t)i * 4u) = f4{g[0], g[1], g[2], g[3]};
	} else {
		// 12 bytes on a 4-byte boundary: a buffer store, because the compiler splits the global form in two (load_position has the load's twin).
		// The row is the buffer -- n * 12 bytes, as for the positions --, so the range check drops what a lane past the batch would store.
		static_assert(D == 3, "GridEncoding: number of input dims must be 2, 3 or 4.");
		typedef uint32_t u3 __attribute__((ext_vector_type(3)));
		const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)row, 0, (int)(n * 12u), 0x00020000);
		const u3 bits = {__builtin_bit_cast(uint32_t, g[0]), __builtin_bit_cast(uint32_t, g[1]), __builtin_bit_cast(uint32_t, g[2])};
		__builtin_amdgcn_raw_buffer_store_b96(bits, rsrc, (int)(i * 12u), 0, 0);
	}
}

template <uint32_t D, uint32_t F, uint32_t SPT, bool DYDX, bool FAST>
TCNN_DEVICE void grid_forward_f32_tile(const Level<D>& lv, const GridIO& io, const float* __restrict__ grid, uint32_t level, uint32_t first, const float (&x)[SPT][D],
                                       float* __restrict__ out, float* __restrict__ dy_dx) {
	constexpr uint32_t NC = 1u << D;
	Cell<D> c[SPT];
	float val[SPT][NC][F];
	// every gather of the thread first (independent loads in flight) ...
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		c[s] = make_cell<D, FAST>(lv, x[s]);
#pragma unroll
		for (uint32_t idx = 0; idx < NC; ++idx) load_features<F>(grid + (size_t)corner_index<D, FAST>(lv, c[s], idx) * F, val[s][idx]);
	}
	// ... then the N-linear interpolation, corner order and fp32 fma chain of grid.h:144-163
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		float result[F];
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) result[f] = 0.0f;
#pragma unroll
		for (uint32_t idx = 0; idx < NC; ++idx) {
			const float weight = corner_weight<D>(c[s], idx);
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) result[f] = __builtin_fmaf(weight, val[s][idx][f], result[f]);
		}
		const uint32_t i = first + s * GRID_THREADS + threadIdx.x;
		const bool live = i < io.n;  // (a lane past the batch gathered sample n - 1's corners and stores nothing)
		if (live) {
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) out[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i] = result[f];
		}
		if constexpr (DYDX) {
			float grads[F][D];
#pragma unroll
			for (uint32_t f = 0; f < F; ++f)
#pragma unroll
				for (uint32_t d = 0; d < D; ++d) grads[f][d] = 0.0f;
			accumulate_dy_dx<D, F>(lv, c[s], [&](uint32_t corner, uint32_t f) { return val[s][corner][f]; }, grads);
			if (live) {
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) store_dy_dx<D>(dy_dx + (size_t)(level * F + f) * io.n * D, io.n, i, grads[f]);
			}
		}
	}
}

template <uint32_t D, uint32_t F, uint32_t SPT, bool DYDX>
__global__ void __launch_bounds__(GRID_THREADS) k_grid_forward_f32_tiles(const GridMeta meta, const GridIO io, const ForwardPlan plan, const float* __restrict__ params,
                                                                          float* __restrict__ out, float* __restrict__ dy_dx) {
	constexpr uint32_t TILE = GRID_THREADS * SPT;
	ForwardPlan::Segment mine;
	uint32_t tile;
	if (!forward_plan_item(meta, io, plan, mine, tile)) return;
	const uint32_t level = mine.level, first = tile * TILE;
	if (level_is_off<true>(meta, level, F)) {  // switched off by the scalar max_level: nothing is loaded, zeros are stored
		const float zeros[D] = {};
#pragma unroll
		for (uint32_t s = 0; s < SPT; ++s) {
			const uint32_t i = first + s * GRID_THREADS + threadIdx.x;
			if (i >= io.n) continue;
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) {
				out[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i] = 0.0f;
				if constexpr (DYDX) store_dy_dx<D>(dy_dx + (size_t)(level * F + f) * io.n * D, io.n, i, zeros);
			}
		}
		return;
	}
	float x[SPT][D];
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) load_position<D, true>(io, min(first + s * GRID_THREADS + threadIdx.x, io.n - 1u), x[s]);
	const Level<D> lv = level_of_segment<D>(meta, mine);
	const float* __restrict__ grid = params + (size_t)mine.offset * F;
	if (lv.fast) {  // wave-uniform: one lean code path per level kind
		grid_forward_f32_tile<D, F, SPT, DYDX, true>(lv, io, grid, level, first, x, out, dy_dx);
	} else {
		grid_forward_f32_tile<D, F, SPT, DYDX, false>(lv, io, grid, level, first, x, out, dy_dx);
	}
}

bool grid_forward_f32_is_tiled(const GridMeta& meta, bool per_sample_max_level) {
	return g_fp32_grid_forward.load() != 0 && !per_sample_max_level && meta.interp != (uint32_t)InterpolationType::Nearest;
}

void launch_forward_f32_tiles(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* params, float* out, float* dy_dx) {
	grid_dispatch(meta, [&](auto D, auto F) {
		constexpr uint32_t SPT = f32_forward_spt(D, F);
		const ForwardPlan plan = make_forward_plan(meta, io.n, GRID_THREADS * SPT, sizeof(float));
		const dim3 blocks(forward_plan_blocks(plan));
		if (dy_dx) {
			TCNN_LAUNCH((k_grid_forward_f32_tiles<D, F, SPT, true>), blocks, dim3(GRID_THREADS), 0, stream, meta, io, plan, params, out, dy_dx);
		} else {
			TCNN_LAUNCH((k_grid_forward_f32_tiles<D, F, SPT, false>), blocks, dim3(GRID_THREADS), 0, stream, meta, io, plan, params, out, (float*)nullptr);
		}
	});
}

}  // namespace tcnn_hip

// grid_forward.hip -- the gathers: the tiled forward that training and inference run, the reference-form forward with dy_dx, the fp32
// encoding's reference-form forward and the index helper, and the launchers.  grid_forward_plan.h: the tiled gather's work plan.
#include "grid_forward_plan.h"

namespace tcnn_hip {

// =============================================================================================
// forward (grid.h:49-212)
// =============================================================================================
template <uint32_t D, uint32_t F, bool DYDX, bool FAST>
TCNN_DEVICE void grid_forward_sample(const Level<D>& lv, const GridIO& io, const half_t* __restrict__ grid, uint32_t level, uint32_t i,
                                     bool level_off, half_t* __restrict__ out, float* __restrict__ dy_dx) {
	constexpr uint32_t NP = (F + 1) / 2;
	h2 result[NP];
#pragma unroll
	for (uint32_t p = 0; p < NP; ++p) result[p] = h2{(half_t)0.0f, (half_t)0.0f};
	float grads[DYDX ? F : 1][D];
#pragma unroll
	for (uint32_t f = 0; f < (DYDX ? F : 1); ++f)
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) grads[f][d] = 0.0f;

	if (!level_off) {
		const Cell<D> c = make_cell<D, FAST>(lv, io, i);
		if (lv.nearest) {
			load_features<F>(grid + (size_t)corner_index<D, FAST>(lv, c, 0) * F, result);
		} else {
			// gather all corners first (independent loads in flight) ...
			h2 val[1u << D][NP];
#pragma unroll
			for (uint32_t idx = 0; idx < (1u << D); ++idx) load_features<F>(grid + (size_t)corner_index<D, FAST>(lv, c, idx) * F, val[idx]);
			// ... then the N-linear interpolation, corner order and fp16 fma chain of grid.h:144-163
#pragma unroll
			for (uint32_t idx = 0; idx < (1u << D); ++idx) {
				const half_t wh = to_half_rn(corner_weight<D>(c, idx));
				const h2 w2 = h2{wh, wh};
#pragma unroll
				for (uint32_t p = 0; p < NP; ++p) result[p] = fma_h2(w2, val[idx][p], result[p]);
			}
			if constexpr (DYDX) accumulate_dy_dx<D, F>(lv, c, [&](uint32_t corner, uint32_t f) { return (float)val[corner][f / 2][f % 2]; }, grads);
		}
	}
#pragma unroll
	for (uint32_t f = 0; f < F; ++f) {
		const uint32_t k = level * F + f;
		if (out) out[(size_t)k * io.stride_k + (size_t)i * io.stride_i] = result[f / 2][f % 2];
		if constexpr (DYDX) {
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) dy_dx[((size_t)k * io.n + i) * D + d] = grads[f][d];
		}
	}
}

template <uint32_t D, uint32_t F, bool DYDX>
__global__ void __launch_bounds__(GRID_THREADS) k_grid_forward(const GridMeta meta, const GridIO io, const half_t* __restrict__ params,
                                                                half_t* __restrict__ out, float* __restrict__ dy_dx) {
	uint32_t level, tile;
	if (!grid_work_item(meta.n_levels, div_round_up(io.n, GRID_TILE), level, tile)) return;
	const Level<D> lv = make_level<D>(meta, level);
	const half_t* __restrict__ grid = params + (size_t)meta.offset[level] * F;
	const bool level_off = level_is_off<true>(meta, level, F);
	if (lv.fast) {  // wave-uniform: one lean code path per level kind
#pragma unroll
		for (uint32_t s = 0; s < GRID_SPT; ++s) {
			const uint32_t i = tile * GRID_TILE + s * GRID_THREADS + threadIdx.x;
			if (i < io.n) grid_forward_sample<D, F, DYDX, true>(lv, io, grid, level, i, io.max_level ? level_is_off<true>(meta, io, i, level, F) : level_off, out, dy_dx);
		}
	} else {
		for (uint32_t s = 0; s < GRID_SPT; ++s) {
			const uint32_t i = tile * GRID_TILE + s * GRID_THREADS + threadIdx.x;
			if (i < io.n) grid_forward_sample<D, F, DYDX, false>(lv, io, grid, level, i, io.max_level ? level_is_off<true>(meta, io, i, level, F) : level_off, out, dy_dx);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// forward, the form training and inference run (no dy_dx).
//
// What bounds it (scripts/microbench_l1.hip, profiles/r02_microbench_l1.txt): a gather instruction whose 64 lanes miss
// the CU's L1 costs ~150 clk per CU however wide the access is and whatever cache-policy bits it carries -- the XCD's
// L2 hands out one 128-byte line per channel and clock (~263 G lines/s chip-wide), and each x-neighbour corner pair of
// a sample is one line with 8 useful bytes in it.  The same instruction costs ~37 clk when it hits L1, ~20 clk for the
// 12-byte-strided position loads, ~16 clk from LDS.  So the levers are (1) as few instructions per (sample, level) as
// possible besides the 2^(D-1) line fetches, (2) an even load per XCD:
//   * a thread owns SPT samples of ONE level and issues all their 2^D * SPT gathers before the first use (walking
//     several levels per block with the positions loaded once measured slower: two tables then compete for the L2);
//   * the (level, tile) items are laid end to end, each with a cost weight (tables that fit the CU's L1 are cheap),
//     and cut into 8 runs of equal cost, one per XCD (block b runs on XCD b % 8 -- observed, only speed depends on
//     it): every XCD sees its 1-3 tables, 2 MiB each at the headline size, hot in its private 4 MiB L2.
// ---------------------------------------------------------------------------------------------
template <uint32_t D, uint32_t F, uint32_t SPT, bool FAST>
TCNN_DEVICE void grid_forward_tile(const Level<D>& lv, const GridIO& io, const half_t* __restrict__ grid, uint32_t level, uint32_t first,
                                   const float (&x)[SPT][D], half_t* __restrict__ out) {
	constexpr uint32_t NP = (F + 1) / 2, NC = 1u << D;
	Cell<D> c[SPT];
	h2 val[SPT][NC][NP];
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		c[s] = make_cell<D, FAST>(lv, x[s]);
#pragma unroll
		for (uint32_t idx = 0; idx < NC; ++idx) load_features<F>(grid + (size_t)corner_index<D, FAST>(lv, c[s], idx) * F, val[s][idx]);
	}
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		h2 result[NP];
#pragma unroll
		for (uint32_t p = 0; p < NP; ++p) result[p] = h2{(half_t)0.0f, (half_t)0.0f};
#pragma unroll
		for (uint32_t idx = 0; idx < NC; ++idx) {  // corner order and fp16 fma chain of grid.h:144-163
			const half_t wh = to_half_rn(corner_weight<D>(c[s], idx));
			const h2 w2 = h2{wh, wh};
#pragma unroll
			for (uint32_t p = 0; p < NP; ++p) result[p] = fma_h2(w2, val[s][idx][p], result[p]);
		}
		const uint32_t i = first + s * GRID_THREADS + threadIdx.x;
		if (i < io.n) {
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) out[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i] = result[f / 2][f % 2];
		}
	}
}

template <uint32_t D, uint32_t F, uint32_t SPT>
__global__ void __launch_bounds__(GRID_THREADS) k_grid_forward_tiles(const GridMeta meta, const GridIO io, const ForwardPlan plan,
                                                                      const half_t* __restrict__ params, half_t* __restrict__ out) {
	constexpr uint32_t TILE = GRID_THREADS * SPT;
	// block -> (segment of its XCD's run, tile): level-major, so an XCD walks one table at a time.  (forward_plan_item is this search as a
	// function, for the fp32 gather; called from here it changed this kernel's instruction schedule, so the text stays.)
	const uint32_t xcd = blockIdx.x & 7u;
	uint32_t slot = blockIdx.x >> 3, tile = 0;
	bool found = false;
	ForwardPlan::Segment mine = {};
	{
		ForwardPlan::Segment head[FWD_SEGMENTS_AT_ONCE];  // (rows are zero-padded: an unused segment holds no tiles and never matches)
#pragma unroll
		for (uint32_t k = 0; k < FWD_SEGMENTS_AT_ONCE; ++k) head[k] = plan.segments[xcd][k];
#if !defined(TCNN_HOST_EMU)
		{  // (all of it now, in ONE round -- the four segments and what the position loads need of the other kernel arguments)
			uint64_t positions = (uint64_t)(uintptr_t)io.positions, per_sample = (uint64_t)(uintptr_t)io.max_level;
			uint32_t a = io.pos_stride_i, b = io.pos_stride_d, c = io.n, d = meta.grid_type, e = meta.interp;
			asm volatile("" : "+s"(positions), "+s"(per_sample), "+s"(a), "+s"(b), "+s"(c), "+s"(d), "+s"(e), "+s"(head[0].level), "+s"(head[0].tile_begin), "+s"(head[0].tile_end),
			             "+s"(head[0].hashmap_size), "+s"(head[0].resolution), "+s"(head[0].scale_bits), "+s"(head[0].offset), "+s"(head[0].fast));
#pragma unroll
			for (uint32_t k = 1; k < FWD_SEGMENTS_AT_ONCE; ++k) {
				asm volatile("" : "+s"(head[k].level), "+s"(head[k].tile_begin), "+s"(head[k].tile_end), "+s"(head[k].hashmap_size), "+s"(head[k].resolution),
				             "+s"(head[k].scale_bits), "+s"(head[k].offset), "+s"(head[k].fast));
			}
		}
#endif
		// branch-free (selects): written with branches the compiler sinks each segment's loads into "the segments before it did not match"
		// and the one round of loads becomes up to four
#pragma unroll
		for (uint32_t k = 0; k < FWD_SEGMENTS_AT_ONCE; ++k) {
			const uint32_t n = head[k].tile_end - head[k].tile_begin;
			const bool here = !found && slot < n;
			mine.level = here ? head[k].level : mine.level;
			mine.hashmap_size = here ? head[k].hashmap_size : mine.hashmap_size;
			mine.resolution = here ? head[k].resolution : mine.resolution;
			mine.scale_bits = here ? head[k].scale_bits : mine.scale_bits;
			mine.offset = here ? head[k].offset : mine.offset;
			mine.fast = here ? head[k].fast : mine.fast;
			tile = here ? head[k].tile_begin + slot : tile;
			slot -= (found || here) ? 0u : n;
			found = found || here;
		}
	}
	if (!found) {  // (more than 32 levels: the rest of the run, one segment at a time)
		for (uint32_t k = FWD_SEGMENTS_AT_ONCE; k < plan.n_segments[xcd]; ++k) {
			const ForwardPlan::Segment seg = plan.segments[xcd][k];
			const uint32_t n = seg.tile_end - seg.tile_begin;
			if (slot < n) {
				mine = seg;
				tile = seg.tile_begin + slot;
				found = true;
				break;
			}
			slot -= n;
		}
	}
	const uint32_t level = mine.level;
	if (!found) return;
	const uint32_t first = tile * TILE;
	float x[SPT][D];
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) load_position<D, true>(io, min(first + s * GRID_THREADS + threadIdx.x, io.n - 1u), x[s]);
	const Level<D> lv = level_of_segment<D>(meta, mine);
	const half_t* __restrict__ grid = params + (size_t)mine.offset * F;
	const bool level_off = level_is_off<true>(meta, level, F);
	if (level_off || lv.nearest || io.max_level) {  // rare forms: one sample at a time
		// (a per-sample max_level: the lane's value is read ahead of its table loads; an off lane issues none, a wave of off lanes
		// branches over the gather and only stores its zeros)
		for (uint32_t s = 0; s < SPT; ++s) {
			const uint32_t i = first + s * GRID_THREADS + threadIdx.x;
			if (i < io.n) grid_forward_sample<D, F, false, false>(lv, io, grid, level, i, io.max_level ? level_is_off<true>(meta, io, i, level, F) : level_off, out, nullptr);
		}
	} else if (lv.fast) {  // wave-uniform: one lean code path per level kind
		grid_forward_tile<D, F, SPT, true>(lv, io, grid, level, first, x, out);
	} else {
		grid_forward_tile<D, F, SPT, false>(lv, io, grid, level, first, x, out);
	}
}

// =============================================================================================
// fp32 encodings: GridEncodingTemplated<float> (what cpp_api.cu:165-168 instantiates for create_encoding(..., Precision::Fp32),
// tcnn.Encoding(dtype=torch.float32)).  Parameters, encoded features and gradients are fp32; the interpolation is the reference's
// kernel_grid<float> -- fp32 weights, result = fma(weight, value, result) in fp32 (grid.h:144-163) --, the backward pass its
// kernel_grid_backward<float, float>: one fp32 global atomic per corner and feature (grid.h:252-255; gradients of any magnitude survive,
// nothing is scaled).  One thread per (sample, level), the reference's formulation; same index / weight code as the 16-bit kernels above.
// The forward of every eikonal step (with dy_dx) and of every fp32 inference runs the tiled gather of grid_forward_f32.hip instead
// (k_grid_forward_f32_tiles, the same arithmetic and bits); this kernel keeps the forms that one does not take -- a per-sample max_level,
// Nearest, a null `out`, parameters off a 16-byte boundary, tcnn_set_fp32_grid_forward(0) -- and is what the host emulator runs.
// =============================================================================================
template <uint32_t D, uint32_t F, bool DYDX>
__global__ void __launch_bounds__(GRID_THREADS) k_grid_forward_f32(const GridMeta meta, const GridIO io, const float* __restrict__ params, float* __restrict__ out,
                                                                    float* __restrict__ dy_dx) {
	uint32_t level, tile;
	if (!grid_work_item(meta.n_levels, div_round_up(io.n, GRID_TILE), level, tile)) return;
	const Level<D> lv = make_level<D>(meta, level);
	const float* __restrict__ grid = params + (size_t)meta.offset[level] * F;
	const bool level_off = level_is_off<true>(meta, level, F);
	for (uint32_t s = 0; s < GRID_SPT; ++s) {
		const uint32_t i = tile * GRID_TILE + s * GRID_THREADS + threadIdx.x;
		if (i >= io.n) continue;
		const bool off = io.max_level ? level_is_off<true>(meta, io, i, level, F) : level_off;
		float result[F], grads[DYDX ? F : 1][D];
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) result[f] = 0.0f;
#pragma unroll
		for (uint32_t f = 0; f < (DYDX ? F : 1); ++f)
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) grads[f][d] = 0.0f;
		if (!off) {
			const Cell<D> c = make_cell<D, false>(lv, io, i);
			if (lv.nearest) {
				const float* v = grid + (size_t)corner_index<D, false>(lv, c, 0) * F;
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) result[f] = v[f];
			} else {
				float val[1u << D][F];
#pragma unroll
				for (uint32_t idx = 0; idx < (1u << D); ++idx) {
					const float* v = grid + (size_t)corner_index<D, false>(lv, c, idx) * F;
#pragma unroll
					for (uint32_t f = 0; f < F; ++f) val[idx][f] = v[f];
				}
#pragma unroll
				for (uint32_t idx = 0; idx < (1u << D); ++idx) {
					const float weight = corner_weight<D>(c, idx);
#pragma unroll
					for (uint32_t f = 0; f < F; ++f) result[f] = __builtin_fmaf(weight, val[idx][f], result[f]);
				}
				if constexpr (DYDX) accumulate_dy_dx<D, F>(lv, c, [&](uint32_t corner, uint32_t f) { return val[corner][f]; }, grads);
			}
		}
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) {
			const uint32_t k = level * F + f;
			if (out) out[(size_t)k * io.stride_k + (size_t)i * io.stride_i] = result[f];
			if constexpr (DYDX) {
#pragma unroll
				for (uint32_t d = 0; d < D; ++d) dy_dx[((size_t)k * io.n + i) * D + d] = grads[f][d];
			}
		}
	}
}

template <uint32_t D>
__global__ void k_grid_indices(const GridMeta meta, const GridIO io, uint32_t* __restrict__ indices) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= io.n) return;
	for (uint32_t level = 0; level < meta.n_levels; ++level) {
		const Level<D> lv = make_level<D>(meta, level);
		for (uint32_t idx = 0; idx < (1u << D); ++idx) {
			uint32_t index;
			if (lv.fast) {
				index = corner_index<D, true>(lv, make_cell<D, true>(lv, io, i), idx);
			} else {
				index = corner_index<D, false>(lv, make_cell<D, false>(lv, io, i), idx);
			}
			indices[((size_t)i * meta.n_levels + level) * (1u << D) + idx] = index;
		}
	}
}

template <uint32_t D, uint32_t F, uint32_t SPT>
static void launch_forward_tiles(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* params, half_t* out) {
	// (Gathering the levels whose table fits a CU's LDS out of LDS -- one launch per level, the table copied in by every workgroup -- was
	// built in round 3 and measured slower in every arrangement: scripts/exp_grid_forward_lds.patch, profiles/r03_exp_notes.txt.)
	const ForwardPlan plan = make_forward_plan(meta, io.n, GRID_THREADS * SPT);
	TCNN_LAUNCH((k_grid_forward_tiles<D, F, SPT>), dim3(forward_plan_blocks(plan)), dim3(GRID_THREADS), 0, stream, meta, io, plan, params, out);
}

void grid_forward(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* params, half_t* out, float* dy_dx) {
	if (io.n == 0) return;
	if (!dy_dx && out) {
#ifndef TCNN_FWD_SPT
#define TCNN_FWD_SPT 2  // samples per thread of the tiled gather (a workgroup: 256 x SPT samples of one level)
#endif
		grid_dispatch(meta, [&](auto D, auto F) { launch_forward_tiles<D, F, TCNN_FWD_SPT>(stream, meta, io, params, out); });
		return;
	}
	const uint32_t blocks = grid_n_blocks(meta.n_levels, io.n);
	grid_dispatch(meta, [&](auto D, auto F) {
		if (dy_dx) {
			TCNN_LAUNCH((k_grid_forward<D, F, true>), dim3(blocks), dim3(GRID_THREADS), 0, stream, meta, io, params, out, dy_dx);
		} else {
			TCNN_LAUNCH((k_grid_forward<D, F, false>), dim3(blocks), dim3(GRID_THREADS), 0, stream, meta, io, params, out, (float*)nullptr);
		}
	});
}

// ---- fp32 encodings (GridEncodingTemplated<float>) ----
void grid_forward(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* params, float* out, float* dy_dx) {
	if (io.n == 0) return;
#if !defined(TCNN_HOST_EMU)  // (the host emulator does not build the tiled fp32 gather: it runs the kernel below at every form)
	// the tiled gather (grid_forward_f32.hip) takes the common forms; it loads a corner's features as 16-byte accesses, hence the alignment
	if (out && ((uintptr_t)params & 15u) == 0u && grid_forward_f32_is_tiled(meta, io.max_level != nullptr)) {
		launch_forward_f32_tiles(stream, meta, io, params, out, dy_dx);
		return;
	}
#endif
	const uint32_t blocks = grid_n_blocks(meta.n_levels, io.n);
	grid_dispatch(meta, [&](auto D, auto F) {
		if (dy_dx) {
			TCNN_LAUNCH((k_grid_forward_f32<D, F, true>), dim3(blocks), dim3(GRID_THREADS), 0, stream, meta, io, params, out, dy_dx);
		} else {
			TCNN_LAUNCH((k_grid_forward_f32<D, F, false>), dim3(blocks), dim3(GRID_THREADS), 0, stream, meta, io, params, out, (float*)nullptr);
		}
	});
}

void grid_indices(hipStream_t stream, const GridMeta& meta, const GridIO& io, uint32_t* indices) {
	if (io.n == 0) return;
	const uint32_t blocks = div_round_up(io.n, 128u);
	switch (meta.n_dims) {
		case 2: TCNN_LAUNCH((k_grid_indices<2>), dim3(blocks), dim3(128), 0, stream, meta, io, indices); break;
		case 3: TCNN_LAUNCH((k_grid_indices<3>), dim3(blocks), dim3(128), 0, stream, meta, io, indices); break;
		case 4: TCNN_LAUNCH((k_grid_indices<4>), dim3(blocks), dim3(128), 0, stream, meta, io, indices); break;
		default: throw std::runtime_error("GridEncoding: number of input dims must be 2, 3 or 4.");
	}
}

}  // namespace tcnn_hip

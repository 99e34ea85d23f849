// grid_forward.hip -- the gathers: the tiled forward that training and inference run, the reference-form forward with dy_dx, the fp32
// encoding's forward and the index helper; the tiled gather's work plan and the launchers.
#include "grid_device.h"

#include <algorithm>
#include <cmath>

namespace tcnn_hip {

// =============================================================================================
// forward (grid.h:49-212)
// =============================================================================================
// d(feature)/d(position) of one sample (grid.h:172-211): along every dimension the differences of the corner pairs, weighted by the
// other dimensions' interpolation weights.  value(corner, f): feature f of corner `corner` as float.
template <uint32_t D, uint32_t F, typename VALUE>
TCNN_DEVICE void accumulate_dy_dx(const Level<D>& lv, const Cell<D>& c, VALUE&& value, float (&grads)[F][D]) {
#pragma unroll
	for (uint32_t gd = 0; gd < D; ++gd) {
#pragma unroll
		for (uint32_t idx = 0; idx < (1u << (D - 1)); ++idx) {
			float weight = lv.scale;
			uint32_t corner = 0;  // corner with the gradient dimension at its low side
#pragma unroll
			for (uint32_t ngd = 0; ngd < D - 1; ++ngd) {
				const uint32_t dim = ngd >= gd ? (ngd + 1) : ngd;
				const uint32_t bit = (idx >> ngd) & 1u;
				weight *= bit ? c.w[dim][1] : c.w[dim][0];
				corner |= bit << dim;
			}
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) {
				const float diff = value(corner | (1u << gd), f) - value(corner, f);
				float t = weight * diff;
				t = t * c.derivative[gd];
				grads[f][gd] = grads[f][gd] + t;
			}
		}
	}
}

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
constexpr uint32_t FWD_MAX_SEGMENTS = 20;  // per XCD: ceil(MAX_N_LEVELS / 8) + the two cut levels at the ends of a run
struct ForwardPlan {
	uint32_t tiles;  // sample tiles per level
	uint32_t n_segments[8];
	// a run of one level's tiles with what the workgroup needs of that level (make_level's inputs): the workgroup's whole "what am I?" is ONE
	// round of scalar loads -- the XCD's first four segments at once, searched in registers -- instead of a loop of dependent loads over the
	// segments followed by a round for the level's table geometry (a workgroup lives a few microseconds: every round trip ahead of its first
	// gather is occupancy the L2's line rate does not get)
	struct Segment {
		uint32_t level, tile_begin, tile_end, hashmap_size, resolution, scale_bits, offset, fast;
	} segments[8][FWD_MAX_SEGMENTS];
};
constexpr uint32_t FWD_SEGMENTS_AT_ONCE = 4;
template <uint32_t D>
TCNN_DEVICE Level<D> level_of_segment(const GridMeta& meta, const ForwardPlan::Segment& seg) {
	Level<D> lv;
	lv.hashmap_size = seg.hashmap_size;
	lv.resolution = seg.resolution;
	lv.mask = seg.hashmap_size - 1u;
	lv.scale = __builtin_bit_cast(float, seg.scale_bits);
	lv.is_hash = meta.grid_type == (uint32_t)GridType::Hash;
	lv.smooth = meta.interp == (uint32_t)InterpolationType::Smoothstep;
	lv.nearest = meta.interp == (uint32_t)InterpolationType::Nearest;
	lv.fast = (seg.fast & 1u) != 0u;  // (the plan stores 0 or 1)
	return lv;
}

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
	// block -> (segment of its XCD's run, tile): level-major, so an XCD walks one table at a time
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
// nothing is scaled).  Not a hot path of the step (the trainer's encoding is 16-bit): one thread per (sample, level), the reference's
// formulation; same index / weight code as the 16-bit kernels above.
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

// Cuts the (level, tile) items, level-major, into 8 runs of equal cost.  Cost of an item (measured per kind of level,
// profiles/r02_exp_forward.txt): 4 for a level whose table fits a CU's 32 KiB L1 next to the streaming traffic
// (<= 24 KiB), 8 for a hashed level (one L2 line per corner pair), 11 for a larger densely indexed level, each times
// (1 + 1.5 x the share of fetches that miss the L2) for tables beyond the L2 (T = 2^22: 16 MiB per level, 2.4x the
// time of a 2 MiB level).  Falls back to uniform costs if a run would need more than FWD_MAX_SEGMENTS segments.
static ForwardPlan make_forward_plan(const GridMeta& meta, uint32_t n, uint32_t tile_samples) {
	for (int uniform = 0; uniform < 2; ++uniform) {
		ForwardPlan plan = {};
		plan.tiles = div_round_up(n, tile_samples);
		uint64_t total = 0;
		uint32_t cost[MAX_N_LEVELS];
		for (uint32_t l = 0; l < meta.n_levels; ++l) {
			const size_t table_bytes = (size_t)level_geometry(meta, l).entries * meta.n_feat * sizeof(half_t);
			// What a (level, 512-sample tile) item costs, from per-workgroup clock stamps of this kernel on the headline and the T = 2^22 stress shape
			// (scripts/exp_forward_stamps.*, profiles/r04_exp_notes.txt sections 18 and 20; microseconds of workgroup life, halved):
			//   tables that fit the L1 (<= 24 KiB)                                   4
			//   hashed levels: no locality at all                                    8 while the table fits the L2, x (1 + 2.5 miss) beyond it (16 MiB: 24)
			//   dense levels: grid_index's stride arithmetic, but the corners of a   4.6 + 1.15 log2(table bytes / 24 KiB), the table capped at the L2's
			//   cell are neighbours in y and z too                                   3 MiB, x (1 + 0.8 miss) beyond it  (55 KiB: 6, 1 MiB: 11, 7 MiB: 21)
			// miss = share of the line fetches that miss the XCD's 4 MiB L2 (about 3 MiB of it hold the table while outputs stream through).
			// Round 2's weights (dense 11 whatever the size, told from hashed by "no power-of-two size"; miss x 1.5 for both kinds) had the XCDs that
			// hold the dense levels finish 8 us late on the headline (its dense levels ARE powers of two) and 40-87 us EARLY on the stress shape.
			const bool hashed = level_geometry(meta, l).hashed;
			const double miss = std::max(0.0, 1.0 - 3.0 * 1048576.0 / (double)table_bytes);
			const double in_l2 = std::min((double)table_bytes, 3.0 * 1048576.0);
			const double base = table_bytes <= 24u * 1024u ? 4.0
			                    : hashed ? 8.0 * (1.0 + 2.5 * miss)
			                             : (4.6 + 1.15 * std::log2(in_l2 / (24.0 * 1024.0))) * (1.0 + 0.8 * miss);
			cost[l] = uniform ? 16u : (uint32_t)(4.0 * base + 0.5);  // (quarter-microsecond units: the cuts fall on whole tiles)
			// A level the scalar max_level switches off gathers nothing: its items load positions and store zeros.  Weighed like the others they
			// left the levels that are still on -- the coarse ones, all in the first XCDs' runs -- where they were, and the forward pass took as
			// long as with every level on (measured: 0.082 ms at max_level 1.0, 0.5 and 0.25 alike).  A quarter of the cheapest kind.
			if (!uniform && level_is_off<true>(meta, l, meta.n_feat)) cost[l] = 4u;
			total += (uint64_t)cost[l] * plan.tiles;
		}
		bool ok = true;
		uint64_t done = 0;  // cost of the items already assigned
		uint32_t xcd = 0;
		for (uint32_t l = 0; l < meta.n_levels && ok; ++l) {
			const LevelGeometry geo = level_geometry(meta, l);
			uint32_t t = 0;
			while (t < plan.tiles) {
				// XCD `xcd` takes items while the cost assigned so far stays below its cumulative share
				const uint64_t limit = (total * (xcd + 1) + 7) / 8;
				uint32_t take = (uint32_t)std::min<uint64_t>(plan.tiles - t, (limit - done + cost[l] - 1) / cost[l]);
				if (xcd == 7) take = plan.tiles - t;
				if (take > 0) {
					uint32_t& ns = plan.n_segments[xcd];
					if (ns == FWD_MAX_SEGMENTS) {
						ok = false;
						break;
					}
					plan.segments[xcd][ns++] = {l, t, t + take, geo.entries, meta.resolution[l], __builtin_bit_cast(uint32_t, meta.scale[l]), meta.offset[l], geo.fast ? 1u : 0u};
					t += take;
					done += (uint64_t)take * cost[l];
				}
				if (done >= limit && xcd < 7) ++xcd;
			}
		}
		if (ok) return plan;
	}
	throw std::runtime_error("grid_forward: could not build the work plan");
}

template <uint32_t D, uint32_t F, uint32_t SPT>
static void launch_forward_tiles(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* params, half_t* out) {
	// (Gathering the levels whose table fits a CU's LDS out of LDS -- one launch per level, the table copied in by every workgroup -- was
	// built in round 3 and measured slower in every arrangement: scripts/exp_grid_forward_lds.patch, profiles/r03_exp_notes.txt.)
	const ForwardPlan plan = make_forward_plan(meta, io.n, GRID_THREADS * SPT);
	uint32_t slots = 0;
	for (uint32_t x = 0; x < 8; ++x) {
		uint32_t n = 0;
		for (uint32_t k = 0; k < plan.n_segments[x]; ++k) n += plan.segments[x][k].tile_end - plan.segments[x][k].tile_begin;
		slots = std::max(slots, n);
	}
	TCNN_LAUNCH((k_grid_forward_tiles<D, F, SPT>), dim3(8u * slots), dim3(GRID_THREADS), 0, stream, meta, io, plan, params, out);
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

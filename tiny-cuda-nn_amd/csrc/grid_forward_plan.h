// grid_forward_plan.h -- what the tiled forward gathers agree on (grid_forward.hip: the 16-bit tables; grid_forward_f32.hip: the fp32 ones):
// the work plan the host cuts, the workgroup's search for its item in it, and the d(feature)/d(position) sum both precisions share.
#pragma once
#include "grid_device.h"

#include <algorithm>
#include <cmath>

namespace tcnn_hip {

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

// The (level, tile) items laid level-major and cut into 8 runs of equal cost, one per XCD: block b serves run b & 7 (grid_forward.hip says
// what bounds the gather and why the runs follow the tables).
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

// block -> (segment of its XCD's run, tile): level-major, so an XCD walks one table at a time.  False: the block lies past its run's end.
// (The fp32 gather's form of the search; k_grid_forward_tiles keeps the same statements in its own body: called from there, this function
// changed that kernel's instruction schedule -- profiles/f32_grid_forward_tiles16_disassembly_diff.txt.)
TCNN_DEVICE bool forward_plan_item(const GridMeta& meta, const GridIO& io, const ForwardPlan& plan, ForwardPlan::Segment& mine, uint32_t& tile) {
	const uint32_t xcd = blockIdx.x & 7u;
	uint32_t slot = blockIdx.x >> 3;
	tile = 0;
	bool found = false;
	mine = {};
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
	return found;
}

// Cuts the (level, tile) items, level-major, into 8 runs of equal cost.  Cost of an item (measured per kind of level,
// profiles/r02_exp_forward.txt): 4 for a level whose table fits a CU's 32 KiB L1 next to the streaming traffic
// (<= 24 KiB), 8 for a hashed level (one L2 line per corner pair), 11 for a larger densely indexed level, each times
// (1 + 1.5 x the share of fetches that miss the L2) for tables beyond the L2 (T = 2^22: 16 MiB per level, 2.4x the
// time of a 2 MiB level).  Falls back to uniform costs if a run would need more than FWD_MAX_SEGMENTS segments.
// element_bytes: sizeof of a table value -- the cost is a function of the table's BYTES (an fp32 table leaves the L1 and the L2 at half
// the entries of a 16-bit one); the 16-bit gather's callers leave it out.
inline ForwardPlan make_forward_plan(const GridMeta& meta, uint32_t n, uint32_t tile_samples, size_t element_bytes = sizeof(half_t)) {
	for (int uniform = 0; uniform < 2; ++uniform) {
		ForwardPlan plan = {};
		plan.tiles = div_round_up(n, tile_samples);
		uint64_t total = 0;
		uint32_t cost[MAX_N_LEVELS];
		for (uint32_t l = 0; l < meta.n_levels; ++l) {
			const size_t table_bytes = (size_t)level_geometry(meta, l).entries * meta.n_feat * element_bytes;
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

// workgroups of a launch over `plan`: 8 x the longest run
inline uint32_t forward_plan_blocks(const ForwardPlan& plan) {
	uint32_t slots = 0;
	for (uint32_t x = 0; x < 8; ++x) {
		uint32_t n = 0;
		for (uint32_t k = 0; k < plan.n_segments[x]; ++k) n += plan.segments[x][k].tile_end - plan.segments[x][k].tile_begin;
		slots = std::max(slots, n);
	}
	return 8u * slots;
}

// the tiled gather of fp32 tables (grid_forward_f32.hip), for the fp32 grid_forward() once it has decided the route: `out` set, `params` on
// a 16-byte boundary, no per-sample max_level, not Nearest
void launch_forward_f32_tiles(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* params, float* out, float* dy_dx);

}  // namespace tcnn_hip

// grid_backward.hip -- the backward's entry point and launch sequence; the sliced owner-computes kernel (small levels of the bucketed mode, the
// sliced A/B modes) and the reference-form atomic kernels (stochastic interpolation, fp32 encodings, fallback).
#include "grid_backward_owner.h"
#include "elementwise_kernels.h"  // Pcg32 (stochastic interpolation)

namespace tcnn_hip {

// Stochastic interpolation (grid.h:284-299): the sample's whole gradient goes to ONE corner, picked per dimension with probability equal to
// its weight from random_val(1337, i + level * n) (common_device.h:469-473); the cell is moved there, its corner 0 is the pick.
template <uint32_t D>
TCNN_DEVICE void pick_stochastic_corner(Cell<D>& c, uint32_t i, uint32_t level, uint32_t n) {
	Pcg32 rng(1337u);
	rng.advance((int64_t)(uint32_t)(i + level * n));
	const float sample = rng.next_float();
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) {
		if (!(sample >= c.w[d][1])) c.grid[d] += 1u;
	}
}

// =============================================================================================
// backward, the reference's formulation (grid.h:215-320): one packed-half global atomic per corner.
// Kept for A/B measurements only (F >= 2): scattered global atomics top out at ~21 G updates/s on
// MI355X whatever their flavour (profiles/r01_microbench_atomics.txt) -- 1.6 ms for one headline step.
// =============================================================================================
template <uint32_t D, uint32_t F>
__global__ void __launch_bounds__(GRID_THREADS) k_grid_backward_atomic(const GridMeta meta, const GridIO io, const half_t* __restrict__ dL_dy,
                                                                        half_t* __restrict__ grid_gradient) {
	uint32_t level, tile;
	if (!grid_work_item(meta.n_levels, div_round_up(io.n, GRID_TILE), level, tile)) return;
	if (!io.max_level && level_is_off<false>(meta, level, F)) return;
	const Level<D> lv = make_level<D>(meta, level);
	half_t* __restrict__ grad = grid_gradient + (size_t)meta.offset[level] * F;
	const bool second_order = io.ddx != nullptr;  // kernel_grid_backward_input_backward_grid (grid.h:427-455): another corner weight

	for (uint32_t s = 0; s < GRID_SPT; ++s) {
		const uint32_t i = tile * GRID_TILE + s * GRID_THREADS + threadIdx.x;
		if (i >= io.n) continue;
		if (io.max_level && level_is_off<false>(meta, io, i, level, F)) continue;
		Cell<D> c = make_cell<D, false>(lv, io, i);
		half_t g[F];
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) g[f] = dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
		float dd[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) dd[d] = 0.0f;
		if (second_order) load_ddx<D>(io, i, dd);
		const bool one_corner = !second_order && (lv.nearest || meta.stochastic != 0u);
		if (!second_order && meta.stochastic != 0u && !lv.nearest) pick_stochastic_corner<D>(c, i, level, io.n);
		const uint32_t n_corners = one_corner ? 1u : (1u << D);
		for (uint32_t idx = 0; idx < n_corners; ++idx) {
			const float weight = second_order ? corner_weight_second_order<D>(lv, c, idx, dd) : corner_weight<D>(c, idx);
			const uint32_t index = corner_index<D, false>(lv, c, idx);
			if constexpr (F == 1) {
				// fp32 product rounded once, as the bucketed form does for F == 1; a packed atomic on the aligned pair, the partner gets +0
				const half_t v = one_corner ? g[0] : to_half_rn(weight * (float)g[0]);
				atomic_add_h2(grad + (index & ~1u), (index & 1u) ? h2{(half_t)0.0f, v} : h2{v, (half_t)0.0f});
			} else {
				const half_t wh = one_corner ? (half_t)1.0f : to_half_rn(weight);
				const h2 w2 = h2{wh, wh};
#pragma unroll
				for (uint32_t p = 0; p < F / 2; ++p) atomic_add_h2(grad + (size_t)index * F + 2 * p, w2 * h2{g[2 * p], g[2 * p + 1]});  // (GRAD_T)weight * grad, grid.h:254
			}
		}
	}
}

template <uint32_t D, uint32_t F>
__global__ void __launch_bounds__(GRID_THREADS) k_grid_backward_atomic_f32(const GridMeta meta, const GridIO io, const float* __restrict__ dL_dy,
                                                                            float* __restrict__ grid_gradient) {
	uint32_t level, tile;
	if (!grid_work_item(meta.n_levels, div_round_up(io.n, GRID_TILE), level, tile)) return;
	if (!io.max_level && level_is_off<false>(meta, level, F)) return;
	const Level<D> lv = make_level<D>(meta, level);
	float* __restrict__ grad = grid_gradient + (size_t)meta.offset[level] * F;
	const bool second_order = io.ddx != nullptr;  // kernel_grid_backward_input_backward_grid<float, float> (grid.h:427-455): another corner weight
	for (uint32_t s = 0; s < GRID_SPT; ++s) {
		const uint32_t i = tile * GRID_TILE + s * GRID_THREADS + threadIdx.x;
		if (i >= io.n) continue;
		if (io.max_level && level_is_off<false>(meta, io, i, level, F)) continue;
		float x[D];
		load_position<D>(io, i, x);
		Cell<D> c = make_cell<D, false>(lv, x);
		float g[F];
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) g[f] = dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
		float dd[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) dd[d] = 0.0f;
		if (second_order) {
			load_ddx<D>(io, i, dd);
			second_order_weights_f32<D>(lv, x, c);
		}
		const bool one_corner = !second_order && (lv.nearest || meta.stochastic != 0u);
		if (!second_order && meta.stochastic != 0u && !lv.nearest) pick_stochastic_corner<D>(c, i, level, io.n);
		const uint32_t n_corners = one_corner ? 1u : (1u << D);
		for (uint32_t idx = 0; idx < n_corners; ++idx) {
			const float weight = one_corner ? 1.0f : (second_order ? corner_weight_second_order<D>(lv, c, idx, dd) : corner_weight<D>(c, idx));
			const uint32_t index = corner_index<D, false>(lv, c, idx);
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) atomic_add_f32(grad + (size_t)index * F + f, weight * g[f]);  // (T)weight * grad, T = float (grid.h:254)
		}
	}
}

// =============================================================================================
// backward, owner-computes form (the default).  No global atomics on the hot path: a workgroup OWNS a
// contiguous slice of one level's table, keeps it in LDS, walks the samples, recomputes the corner
// indices (integer ALU is cheap) and accumulates only the corners that fall into its slice; the slice
// is then written back with plain coalesced stores -- which also makes the reference's per-step
// gradient memset (grid.h:865-867) unnecessary.
//
// Measured LDS atomic rates that shape this (profiles/r01_microbench_lds_atomics.txt): a dense
// ds_add_f32 / ds_pk_add_f16 wave instruction costs ~170 clk (floating-point LDS atomics are serialised
// per lane, ~2.6 clk each), a dense ds_add_u32 / ds_add_u64 7 / 11 clk; with <= 2-3 active lanes all of
// them cost ~7 clk.  Hence two accumulator kinds, chosen per level on the host:
//   * small tables (coarse levels, nearly every corner of every sample hits the slice -> dense
//     atomics): 64-bit fixed point (2^-24 resolution, exact and order-independent, cannot overflow for
//     any fp16 input), the SAMPLES are additionally split over several workgroups, each flushing its
//     partial table with a few packed-half global atomics;
//   * large tables (fine / hashed levels, a slice sees ~1/16 of the corners -> sparse atomics):
//     packed fp16 (the reference's own accumulation type, vec.h:328-351) or fp32 slices.
// =============================================================================================
enum class Acc { F32, PK16, FIX64 };

template <uint32_t D, uint32_t F, Acc ACC, bool FAST>
TCNN_DEVICE void sliced_accumulate(const GridMeta& meta, const Level<D>& lv, const GridIO& io, const half_t* __restrict__ dL_dy, uint32_t level, uint32_t begin,
                                   uint32_t end, uint32_t slice_begin, uint32_t slice_count, unsigned char* lds_raw) {
	constexpr uint32_t N_CORNERS = 1u << D;
	float* tab_f = (float*)lds_raw;                            // [entries][F]
	h2* tab_h = (h2*)lds_raw;                                  // [entries][F/2]
	unsigned long long* tab_q = (unsigned long long*)lds_raw;  // [entries][F]
	// U samples per lane and iteration: all their position / gradient loads are issued before the first
	// use (each workgroup streams the whole batch; with one sample in flight the loop is latency-bound).
	constexpr uint32_t U = 4;
	for (uint32_t base = begin + threadIdx.x; base < end; base += SLICED_THREADS * U) {
		float x[U][D];
		half_t g[U][F];
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) {
			const uint32_t i = min(base + u * SLICED_THREADS, end - 1);  // clamped: out-of-range lanes are masked below
			load_position<D>(io, i, x[u]);
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) g[u][f] = dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
		}
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) {
			const Cell<D> c = make_cell<D, FAST>(lv, x[u]);
			// which of this sample's corners live in my slice?  (branch-free bit mask)
			uint32_t match = 0;
#pragma unroll
			for (uint32_t idx = 0; idx < N_CORNERS; ++idx) {
				const uint32_t rel = corner_index<D, FAST>(lv, c, idx) - slice_begin;
				match |= (rel < slice_count ? 1u : 0u) << idx;
			}
			if (lv.nearest) match &= 1u;
			if (base + u * SLICED_THREADS >= end) match = 0;
			if (io.max_level && level_is_off<false>(meta, io, min(base + u * SLICED_THREADS, end - 1), level, F)) match = 0;  // per-sample max_level

			while (match) {
				const uint32_t idx = (uint32_t)__builtin_ctz(match);
				match &= match - 1;
				const uint32_t rel = corner_index<D, FAST>(lv, c, idx) - slice_begin;
				const float weight = lv.nearest ? 1.0f : corner_weight<D>(c, idx);
				const half_t wh = to_half_rn(weight);  // (GRAD_T)weight, grid.h:254
				if constexpr (ACC == Acc::PK16) {
					const h2 w2 = h2{wh, wh};
#pragma unroll
					for (uint32_t p = 0; p < F / 2; ++p) lds_atomic_add_h2(&tab_h[rel * (F / 2) + p], w2 * h2{g[u][2 * p], g[u][2 * p + 1]});
				} else {
					const float wq = F == 1 ? weight : (float)wh;  // F == 1: grad_t is float in the reference (grid.h:665)
#pragma unroll
					for (uint32_t f = 0; f < F; ++f) {
						const float prod = wq * (float)g[u][f];
						if constexpr (ACC == Acc::FIX64) {
							lds_atomic_add_u64(&tab_q[rel * F + f], (unsigned long long)to_fixed(prod));
						} else {
							lds_atomic_add_f32(&tab_f[rel * F + f], prod);
						}
					}
				}
			}
		}
	}
}

template <uint32_t D, uint32_t F, Acc ACC>
TCNN_DEVICE void sliced_level(const GridMeta& meta, const GridIO& io, const Level<D>& lv, uint32_t level, uint32_t slice, uint32_t chunk,
                              uint32_t n_chunks, uint32_t entries_per_slice, const half_t* __restrict__ dL_dy, half_t* __restrict__ grid_gradient,
                              bool accumulate, bool level_off, unsigned char* lds_raw) {
	const uint32_t slice_begin = slice * entries_per_slice;
	const uint32_t slice_count = slice_extent(slice_begin, entries_per_slice, lv.hashmap_size);
	half_t* __restrict__ grad = grid_gradient + ((size_t)meta.offset[level] + slice_begin) * F;

	constexpr uint32_t WORDS_PER_VALUE_X2 = ACC == Acc::FIX64 ? 4 : (ACC == Acc::F32 ? 2 : 1);  // 32-bit words per value, times two
	const uint32_t lds_words = slice_count * F * WORDS_PER_VALUE_X2 / 2;
	for (uint32_t e = threadIdx.x; e < lds_words; e += SLICED_THREADS) ((uint32_t*)lds_raw)[e] = 0u;  // +0.0f / (0, 0) / 0
	__syncthreads();

	if (!level_off) {
		const uint32_t per_chunk = div_round_up(io.n, n_chunks);
		const uint32_t begin = chunk * per_chunk;
		const uint32_t end = min(begin + per_chunk, io.n);
		if (lv.fast) {
			sliced_accumulate<D, F, ACC, true>(meta, lv, io, dL_dy, level, begin, end, slice_begin, slice_count, lds_raw);
		} else {
			sliced_accumulate<D, F, ACC, false>(meta, lv, io, dL_dy, level, begin, end, slice_begin, slice_count, lds_raw);
		}
	}
	__syncthreads();

	// ---- write the slice back: this workgroup is its only writer when n_chunks == 1
	const uint32_t n_halves = slice_count * F;  // even: level sizes are multiples of 8
	for (uint32_t e2 = threadIdx.x; e2 < n_halves / 2; e2 += SLICED_THREADS) {
		h2 v;
		if constexpr (ACC == Acc::PK16) {
			v = ((const h2*)lds_raw)[e2];
		} else if constexpr (ACC == Acc::F32) {
			v = h2{(half_t)((const float*)lds_raw)[2 * e2], (half_t)((const float*)lds_raw)[2 * e2 + 1]};
		} else {
			const long long q0 = ((const long long*)lds_raw)[2 * e2], q1 = ((const long long*)lds_raw)[2 * e2 + 1];
			v = h2{(half_t)(float)((double)q0 * (1.0 / FIXED_SCALE)), (half_t)(float)((double)q1 * (1.0 / FIXED_SCALE))};
		}
		store_pair(grad, e2, v, n_chunks, accumulate);
	}
}

template <uint32_t D, uint32_t F, bool PACKED>
__global__ void __launch_bounds__(SLICED_THREADS) k_grid_backward_sliced(const GridMeta meta, const GridIO io, const SlicePlan plan,
                                                                           const half_t* __restrict__ dL_dy, half_t* __restrict__ grid_gradient,
                                                                           const int accumulate, const BucketPlan bplan,
                                                                           uint32_t* __restrict__ counters, const uint32_t* __restrict__ queues,
                                                                           const uint32_t* __restrict__ overflow) {
	TCNN_DYN_LDS(lds_raw);
	uint32_t item = 0, local_block;
	if (plan.blocks_per_item) {
		// near-uniform plan (the bucketed backward): work item = blockIdx / stride, no search; an item with fewer workgroups
		// than the stride leaves the rest idle (each idle workgroup still claims a CU's LDS for an instant, so the host only
		// picks this when almost nothing is padded)
		item = blockIdx.x / plan.blocks_per_item;
		local_block = blockIdx.x % plan.blocks_per_item;
		if (local_block >= plan.block_begin[item + 1] - plan.block_begin[item]) return;
	} else {
		while (item + 1 < plan.n_items && blockIdx.x >= plan.block_begin[item + 1]) ++item;
		local_block = blockIdx.x - plan.block_begin[item];
	}
	const uint32_t level = plan.level[item], kind = plan.kind[item];
	const uint32_t n_slices = plan.n_slices[item];
	const uint32_t n_chunks = (plan.block_begin[item + 1] - plan.block_begin[item]) / n_slices;
	const uint32_t slice = local_block % n_slices, chunk = local_block / n_slices;

	const bool level_off = !io.max_level && level_is_off<false>(meta, level, F);  // (a per-sample max_level is tested sample by sample)
	const Level<D> lv = make_level<D>(meta, level);

	if (kind == SLICE_BUCKET) {
		if (bplan.packed_owner) return;  // k_grid_bucket_owner runs them
		const uint32_t j = plan.slot[item];
		const OwnerSlice own = {bplan.capacity[j], bplan.n_chunks[j], bplan.n_buckets[j], bplan.counter_base[j], bplan.queue_base[j], meta.offset[level], j,
		                        bplan.shift, bplan.overflow_counter, bplan.overflow_capacity, bplan.n_owner_blocks, bplan.level_sum_base, bplan.n_levels};
		bucket_level<D, F>(meta, lv, level, slice, chunk, own, counters, queues, overflow, grid_gradient, accumulate != 0, lds_raw);
		return;
	}
	if (kind == SLICE_GLOBAL_ATOMIC) {
		// Dense-indexed level too large for the fixed-point path: its corners are memory-adjacent, so a float
		// slice would see all-or-nothing samples (8 serial iterations at 1/16 lane occupancy).  The memory-side
		// atomic units are otherwise idle during this launch: send this level's updates there (tile = slice).
		if (level_off) return;
		half_t* __restrict__ grad = grid_gradient + (size_t)meta.offset[level] * F;
		const uint32_t per_tile = div_round_up(io.n, n_slices);
		const uint32_t begin = slice * per_tile, end = min(begin + per_tile, io.n);
		for (uint32_t i = begin + threadIdx.x; i < end; i += SLICED_THREADS) {
			if (io.max_level && level_is_off<false>(meta, io, i, level, F)) continue;
			const Cell<D> c = make_cell<D, false>(lv, io, i);
			half_t g[F];
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) g[f] = dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
			const uint32_t n_corners = lv.nearest ? 1u : (1u << D);
			for (uint32_t idx = 0; idx < n_corners; ++idx) {
				const half_t wh = lv.nearest ? (half_t)1.0f : to_half_rn(corner_weight<D>(c, idx));
				const uint32_t index = corner_index<D, false>(lv, c, idx);
				if constexpr (F == 1) {
					// a packed atomic on the aligned pair; the partner half gets +0
					const h2 v = (index & 1u) ? h2{(half_t)0.0f, wh * g[0]} : h2{wh * g[0], (half_t)0.0f};
					atomic_add_h2(grad + (index & ~1u), v);
				} else {
					const h2 w2 = h2{wh, wh};
#pragma unroll
					for (uint32_t p = 0; p < F / 2; ++p) atomic_add_h2(grad + (size_t)index * F + 2 * p, w2 * h2{g[2 * p], g[2 * p + 1]});
				}
			}
		}
		return;
	}

	// equal slices of this level's table (level sizes are multiples of 8; the host sized n_slices to fit LDS)
	const uint32_t entries_per_slice = next_multiple(div_round_up(lv.hashmap_size, n_slices), 8u);
	if (kind == SLICE_FIXED64) {
		sliced_level<D, F, Acc::FIX64>(meta, io, lv, level, slice, chunk, n_chunks, entries_per_slice, dL_dy, grid_gradient, accumulate != 0,
		                               level_off, lds_raw);
	} else {
		sliced_level<D, F, PACKED ? Acc::PK16 : Acc::F32>(meta, io, lv, level, slice, chunk, n_chunks, entries_per_slice, dL_dy, grid_gradient,
		                                                   accumulate != 0, level_off, lds_raw);
	}
}

static void grid_backward_atomic(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* dL_dy, half_t* grid_gradient,
                                 bool accumulate) {
	const size_t n_params = (size_t)meta.offset[meta.n_levels] * meta.n_feat;
	if (!accumulate) {  // grid.h:865-867
		if (hipMemsetAsync(grid_gradient, 0, n_params * sizeof(half_t), stream) != hipSuccess) throw std::runtime_error("grid_backward: memset failed");
	}
	const uint32_t blocks = grid_n_blocks(meta.n_levels, io.n);
	grid_dispatch(meta, [&](auto D, auto F) { TCNN_LAUNCH((k_grid_backward_atomic<D, F>), dim3(blocks), dim3(GRID_THREADS), 0, stream, meta, io, dL_dy, grid_gradient); });
}

GridBackwardWorkspace grid_backward_workspace_size(const GridMeta& meta, uint32_t n, GridBackwardMode mode, uint32_t lds_slice_bytes) {
	GridBackwardWorkspace ws;
	if (mode != GridBackwardMode::Bucketed || n == 0) return ws;
	const BackwardPlan bp = make_backward_plan(meta, n, true, true, false, lds_slice_bytes);
	ws.scratch_bytes = bp.workspace_bytes;
	ws.n_counters = bp.n_counters;
	return ws;
}

static void grid_backward_sliced_launches(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* dL_dy, half_t* grid_gradient,
                                          bool accumulate, bool packed, bool bucketed, uint32_t lds_slice_bytes, const GridBackwardWorkspace& ws);

// The queue counters are handed back zeroed by the kernels themselves; if the launch sequence is cut short by an error
// they are cleared here, so that the contract ("zero on entry") survives for the next call.
static void grid_backward_sliced(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* dL_dy, half_t* grid_gradient,
                                 bool accumulate, bool packed, bool bucketed, uint32_t lds_slice_bytes, const GridBackwardWorkspace& ws) {
	try {
		grid_backward_sliced_launches(stream, meta, io, dL_dy, grid_gradient, accumulate, packed, bucketed, lds_slice_bytes, ws);
	} catch (...) {
		if (bucketed && ws.counters) (void)hipMemsetAsync(ws.counters, 0, ws.n_counters * sizeof(uint32_t), stream);
		throw;
	}
}

static void grid_backward_sliced_launches(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* dL_dy, half_t* grid_gradient,
                                          bool accumulate, bool packed, bool bucketed, uint32_t lds_slice_bytes, const GridBackwardWorkspace& ws) {
	const uint32_t F = meta.n_feat;
	packed = packed && (F % 2 == 0);
	const BackwardPlan bp = make_backward_plan(meta, io.n, packed, bucketed, accumulate, lds_slice_bytes);
	lds_slice_bytes = bp.lds_slice_bytes;
	const SlicePlan& plan = bp.slices;
	const BucketPlan& bk = bp.buckets;
	const uint32_t blocks = bp.blocks;
	if (io.ddx) {
		for (uint32_t p = 0; p < plan.n_items; ++p) {
			if (plan.kind[p] != SLICE_BUCKET) throw std::runtime_error("grid_backward: second-order scatter needs every level in the bucketed path (grid_backward() checks this)");
		}
	}
	uint32_t* counters = nullptr;
	uint32_t* queues = nullptr;
	uint32_t* overflow = nullptr;
	if (bk.n_levels) {
		if (!ws.scratch || ws.scratch_bytes < bp.workspace_bytes || !ws.counters || ws.n_counters < bp.n_counters) {
			throw std::runtime_error("grid_backward: workspace too small for the bucketed backward");
		}
		counters = ws.counters;  // zero on entry (contract); the kernels below leave them zeroed again
		queues = (uint32_t*)ws.scratch;
		overflow = (uint32_t*)((unsigned char*)ws.scratch + bp.overflow_offset);
	}
	if (bk.n_levels) {
		if (ws.phase_hook) ws.phase_hook(ws.hook_user, 0, 1);
		// pass A: derive every corner once, bin by owner (+ zero the gradients of chunked levels)
		launch_bucket_scatter(stream, meta, io, bk, dL_dy, counters, queues, overflow, grid_gradient, accumulate);
		if (ws.phase_hook) ws.phase_hook(ws.hook_user, 0, 0);
	}
	if (ws.phase_hook) ws.phase_hook(ws.hook_user, 1, 1);
	for (uint32_t p = 0; p < plan.n_items; ++p) {
		struct { uint32_t level, kind, n_chunks; } it = {plan.level[p], plan.kind[p], bp.n_chunks[p]};
		if (it.kind != SLICE_BUCKET && (it.n_chunks > 1 || it.kind == SLICE_GLOBAL_ATOMIC) && !accumulate) {  // atomically updated levels start from zero
			const uint32_t entries = meta.offset[it.level + 1] - meta.offset[it.level];
			if (hipMemsetAsync(grid_gradient + (size_t)meta.offset[it.level] * F, 0, (size_t)entries * F * sizeof(half_t), stream) != hipSuccess) {
				throw std::runtime_error("grid_backward: memset failed");
			}
		}
	}
	const int acc = accumulate ? 1 : 0;
	// bucket items: the packed owner kernel (even F) unless grid_owner_mode() asks for the 64-bit-per-value form; mode "wide" runs the
	// packed kernel's own 64-bit redo on every slice (tests)
	const int owner_mode = grid_owner_mode();
	BucketPlan bk_launch = bk;
	bk_launch.packed_owner = (bk.n_levels && F % 2 == 0 && owner_mode != 1) ? 1u : 0u;
	bool other_items = false;
	for (uint32_t p = 0; p < plan.n_items; ++p) other_items = other_items || plan.kind[p] != SLICE_BUCKET;
	if (bk_launch.packed_owner) launch_bucket_owners(stream, meta, bp, accumulate, owner_mode == 2, counters, queues, overflow, grid_gradient);
	if (!bk_launch.packed_owner || other_items) {
		grid_dispatch(meta, [&](auto D, auto F) {
			if (!packed) {
				TCNN_SET_MAX_DYN_LDS((k_grid_backward_sliced<D, F, false>), lds_slice_bytes);
				TCNN_LAUNCH((k_grid_backward_sliced<D, F, false>), dim3(blocks), dim3(SLICED_THREADS), lds_slice_bytes, stream, meta, io, plan, dL_dy, grid_gradient, acc,
				            bk_launch, counters, (const uint32_t*)queues, (const uint32_t*)overflow);
			} else if constexpr (F % 2 == 0) {  // (packed implies an even F: no packed-half instances for odd F)
				TCNN_SET_MAX_DYN_LDS((k_grid_backward_sliced<D, F, true>), lds_slice_bytes);
				TCNN_LAUNCH((k_grid_backward_sliced<D, F, true>), dim3(blocks), dim3(SLICED_THREADS), lds_slice_bytes, stream, meta, io, plan, dL_dy, grid_gradient, acc,
				            bk_launch, counters, (const uint32_t*)queues, (const uint32_t*)overflow);
			}
		});
	}
	if (ws.phase_hook) ws.phase_hook(ws.hook_user, 1, 0);
}

void grid_backward(hipStream_t stream, const GridMeta& meta, const GridIO& io, const half_t* dL_dy, half_t* grid_gradient, bool accumulate,
                   GridBackwardMode mode, uint32_t lds_slice_bytes, const GridBackwardWorkspace& ws) {
	if (io.n == 0) return;
	if (!grid_gradient) throw std::runtime_error("grid_backward: missing gradient buffer");
	if (io.ddx) {  // second-order scatter
		if (meta.interp == (uint32_t)InterpolationType::Nearest) {  // d(dy_dx)/d(grid) == 0 without interpolation (grid.h:422-425)
			const size_t bytes = (size_t)meta.offset[meta.n_levels] * meta.n_feat * sizeof(half_t);
			if (!accumulate && hipMemsetAsync(grid_gradient, 0, bytes, stream) != hipSuccess) throw std::runtime_error("grid_backward: memset failed");
			return;
		}
		if (mode != GridBackwardMode::Bucketed) throw std::runtime_error("grid_backward: the second-order scatter runs in the bucketed mode only");
		// more than 32 levels, or a level beyond 4096 buckets of the chosen slice size: the second-order weight through the
		// reference's formulation (global atomics) instead
		const BackwardPlan bp = make_backward_plan(meta, io.n, meta.n_feat % 2 == 0, true, accumulate, lds_slice_bytes);
		for (uint32_t p = 0; p < bp.slices.n_items; ++p) {
			if (bp.slices.kind[p] != SLICE_BUCKET) mode = GridBackwardMode::Atomic;
		}
	}
	// stochastic interpolation (one unweighted update per sample and level): the reference's atomic form; the owner-computes
	// passes are built around all 2^D weighted corners
	if (meta.stochastic != 0u && !io.ddx) mode = GridBackwardMode::Atomic;
	switch (mode) {
		case GridBackwardMode::SlicedF32: grid_backward_sliced(stream, meta, io, dL_dy, grid_gradient, accumulate, false, false, lds_slice_bytes, ws); break;
		case GridBackwardMode::SlicedF16: grid_backward_sliced(stream, meta, io, dL_dy, grid_gradient, accumulate, true, false, lds_slice_bytes, ws); break;
		case GridBackwardMode::Atomic:
			if (ws.phase_hook) ws.phase_hook(ws.hook_user, 1, 1);
			grid_backward_atomic(stream, meta, io, dL_dy, grid_gradient, accumulate);
			if (ws.phase_hook) ws.phase_hook(ws.hook_user, 1, 0);
			break;
		case GridBackwardMode::Bucketed:
			grid_backward_sliced(stream, meta, io, dL_dy, grid_gradient, accumulate, true, true, lds_slice_bytes, ws);
			break;
	}
}

// ---- fp32 encodings (GridEncodingTemplated<float>) ----
void grid_backward(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* dL_dy, float* grid_gradient, bool accumulate) {
	if (io.n == 0) return;
	if (!grid_gradient) throw std::runtime_error("grid_backward: missing gradient buffer");
	const size_t n_params = (size_t)meta.offset[meta.n_levels] * meta.n_feat;
	if (!accumulate) {  // grid.h:865-867
		if (hipMemsetAsync(grid_gradient, 0, n_params * sizeof(float), stream) != hipSuccess) throw std::runtime_error("grid_backward: memset failed");
	}
	// second-order scatter (io.ddx set): d(dy_dx)/d(grid) == 0 without interpolation (grid.h:422-425)
	if (io.ddx && meta.interp == (uint32_t)InterpolationType::Nearest) return;
	const uint32_t blocks = grid_n_blocks(meta.n_levels, io.n);
	grid_dispatch(meta, [&](auto D, auto F) { TCNN_LAUNCH((k_grid_backward_atomic_f32<D, F>), dim3(blocks), dim3(GRID_THREADS), 0, stream, meta, io, dL_dy, grid_gradient); });
}

}  // namespace tcnn_hip

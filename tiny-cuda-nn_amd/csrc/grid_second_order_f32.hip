// grid_second_order_f32.hip -- the second-order pass of an fp32 grid encoding without floating-point atomics and without a sample-major walk
// (tcnn_set_fp32_grid_second_order; grid_second_order.hip states the formulas and keeps the kernels these replace):
//   A. the parameter gradient through the owner pass of grid_backward_f32.hip.  Its launch sequence stays -- clear, count, scan, scatter,
//      owners -- and only the scatter is another kernel: k_f32_second_order_records forms the record of kernel_grid_backward_input_backward_grid,
//      corner weight scale * sum_d ddx[d] * pos'(d) * (+-1) * prod_{e != d} w_e, with the statements of k_grid_backward_atomic_f32, so a term
//      has that kernel's bits.  A record's slice depends on its entry index alone: the counting launch is the first-order one, and this body
//      derives index and liveness as that one does, so each run is exactly as long as what is written into it.  The owners take every value's
//      quantum from the largest term that reaches it (grid_backward_plan.h): weights above one change nothing.
//   B. the input gradient level-major and tiled: one workgroup per (level, sample tile) item of grid_forward_plan.h's ForwardPlan with the
//      table bytes of float entries -- the tile size and the eight runs of grid_forward_f32.hip, so an XCD walks one table at a time.  A lane
//      holds its samples' x, ddx and the level's F values of dL_dy, issues every corner load (8 bytes at F = 2, 16 from F = 4) before the first
//      use, forms v(c) = sum_f grid[c][f] * dL_dy[f] and the level's D sums with the statements of k_grid_backward_backward_input_f32, and
//      stores them coalesced to partial[level][d][i].  k_f32_sum_levels then adds the levels in ascending order per (i, d) and overwrites
//      dL_dinput: the additions of the sample-major kernel in its order -- the same bits --, no atomics, nothing that depends on a schedule.
//      A level the scalar max_level switches off (the backward passes' '>' rule) has no items and no row in `partial`.
// Not part of the host emulator's build.
#include "grid_backward_plan.h"
#include "grid_forward_plan.h"
#include "switches.h"

namespace tcnn_hip {

// ---- A: the scatter of the second-order records ------------------------------------------------------------------------------------------
// entry index and second-order weight of each corner of one sample on one level
template <uint32_t D, bool FAST>
TCNN_DEVICE void f32_second_order_corners(const Level<D>& lv, const float (&x)[D], const float (&dd)[D], uint32_t (&index)[1u << D], float (&weight)[1u << D]) {
	Cell<D> c = make_cell<D, FAST>(lv, x);
	second_order_weights_f32<D>(lv, x, c);
#pragma unroll
	for (uint32_t idx = 0; idx < (1u << D); ++idx) {
		index[idx] = corner_index<D, FAST>(lv, c, idx);
		weight[idx] = corner_weight_second_order<D>(lv, c, idx, dd);
	}
}

template <uint32_t D, uint32_t F>
__global__ void __launch_bounds__(F32_SCATTER_THREADS) k_f32_second_order_records(const GridMeta meta, const GridIO io, const F32OwnerPlan plan, const float* __restrict__ dL_dy,
                                                                                  uint32_t* __restrict__ control, uint32_t* __restrict__ queues) {
	constexpr uint32_t N_CORNERS = 1u << D, SPT = F32_RECORDS_PER_LANE >> D, TILE = SPT * F32_SCATTER_THREADS, W = f32_record_words(F);
	TCNN_DYN_LDS(lds_raw);
	const uint32_t j = blockIdx.x / plan.tiles, tile = blockIdx.x % plan.tiles;
	const uint32_t level = plan.level[j], nb = plan.n_slices[j], shift = plan.shift[j];
	if (!io.max_level && level_is_off<false>(meta, level, F)) return;  // no records: the owners store zeros
	const Level<D> lv = make_level<D>(meta, level);
	uint32_t* cnt = (uint32_t*)lds_raw;  // [nb] records of this tile per slice
	uint32_t* run = cnt + nb;            // [nb] where the tile's records of a slice begin in the queue
	for (uint32_t b = threadIdx.x; b < nb; b += F32_SCATTER_THREADS) cnt[b] = 0u;

	float x[SPT][D], dd[SPT][D], g[SPT][F];
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		const uint32_t i = min(tile * TILE + s * F32_SCATTER_THREADS + threadIdx.x, io.n - 1u);  // clamped: lanes past the batch are masked below
		load_position<D>(io, i, x[s]);
		load_ddx<D>(io, i, dd[s]);
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) g[s][f] = dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
	}
	__syncthreads();

	uint32_t index[SPT][N_CORNERS], rank[SPT][N_CORNERS];
	float weight[SPT][N_CORNERS];
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		const uint32_t i = tile * TILE + s * F32_SCATTER_THREADS + threadIdx.x;
		bool live = i < io.n;
		if (live && io.max_level && level_is_off<false>(meta, io, i, level, F)) live = false;  // per-sample max_level: no records
		if (lv.fast) f32_second_order_corners<D, true>(lv, x[s], dd[s], index[s], weight[s]);
		else f32_second_order_corners<D, false>(lv, x[s], dd[s], index[s], weight[s]);
#pragma unroll
		for (uint32_t idx = 0; idx < N_CORNERS; ++idx) {
			if (!live) {
				index[s][idx] = BUCKET_INVALID_INDEX;
			} else {
				rank[s][idx] = atomic_add_u32(&cnt[index[s][idx] >> shift], 1u);
			}
		}
	}
	__syncthreads();

	uint32_t* __restrict__ cursors = control + plan.cursor_base + plan.slice_base[j];
	for (uint32_t b = threadIdx.x; b < nb; b += F32_SCATTER_THREADS) {
		const uint32_t c = cnt[b];
		run[b] = c ? atomic_add_u32(&cursors[b], c) : 0u;
	}
	__syncthreads();
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
#pragma unroll
		for (uint32_t idx = 0; idx < N_CORNERS; ++idx) {
			if (index[s][idx] == BUCKET_INVALID_INDEX) continue;
			const uint32_t pos = run[index[s][idx] >> shift] + rank[s][idx];
			if (pos >= plan.n_queue_records) continue;  // (cannot happen: the counts are of these very records)
			uint32_t* __restrict__ dst = queues + (size_t)pos * W;
			queue_store(dst, index[s][idx] & ((1u << shift) - 1u));
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) queue_store(dst + 1 + f, __builtin_bit_cast(uint32_t, weight[s][idx] * g[s][f]));  // (T)weight * grad, T = float (grid.h:449)
		}
	}
}

void launch_f32_second_order_scatter(hipStream_t stream, const GridMeta& meta, const GridIO& io, const F32OwnerPlan& plan, const float* dL_dy, uint32_t* control, uint32_t* queues,
                                     uint32_t record_blocks, uint32_t record_lds) {
	grid_dispatch(meta, [&](auto D, auto F) {
		TCNN_LAUNCH((k_f32_second_order_records<D, F>), dim3(record_blocks), dim3(F32_SCATTER_THREADS), record_lds, stream, meta, io, plan, dL_dy, control, queues);
	});
}

// ---- B: the input gradient, level-major and tiled ----------------------------------------------------------------------------------------
// samples per thread: the tiled forward's rule (two while their corner values fit 64 registers), but one at D = 4, where the 16 corners' weight
// products of one sample alone take the register file (two samples: 240 VGPRs and up)
constexpr uint32_t f32_second_order_spt(uint32_t D, uint32_t F) { return D < 4u && (F << D) <= 32u ? 2u : 1u; }

// levels the scalar max_level leaves on for the backward passes: a prefix, level_is_off is monotonic in the level
static uint32_t levels_on(const GridMeta& meta) {
	uint32_t n = 0;
	while (n < meta.n_levels && !level_is_off<false>(meta, n, meta.n_feat)) ++n;
	return n;
}

template <uint32_t D, uint32_t F, uint32_t SPT, bool FAST>
TCNN_DEVICE void second_order_input_tile(const Level<D>& lv, const GridIO& io, const float* __restrict__ grid, const float* __restrict__ dL_dy, uint32_t level, uint32_t first,
                                         float* __restrict__ partial) {
	constexpr uint32_t NC = 1u << D;
	float x[SPT][D], dd[SPT][D], gy[SPT][F], val[SPT][NC][F];
	Cell<D> c[SPT];
	// every load of the thread first: positions, ddx and dL_dy, then the gathers (independent loads in flight) ...
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		const uint32_t i = min(first + s * GRID_THREADS + threadIdx.x, io.n - 1u);  // (a lane past the batch works on sample n - 1 and stores nothing)
		load_position<D, true>(io, i, x[s]);
		load_ddx<D>(io, i, dd[s]);
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) gy[s][f] = dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
	}
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		c[s] = make_cell<D, FAST>(lv, x[s]);
#pragma unroll
		for (uint32_t idx = 0; idx < NC; ++idx) load_features<F>(grid + (size_t)corner_index<D, FAST>(lv, c[s], idx) * F, val[s][idx]);
	}
	// ... then backward_backward_input_sample's arithmetic for this level, statement for statement
	const float s2 = lv.scale * lv.scale;
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		second_order_weights_f32<D>(lv, x[s], c[s]);
		float d2[D];  // pos''(d): 0 for Linear, 12 * (0.5 - t) for Smoothstep
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			float p = __builtin_fmaf(lv.scale, x[s][d], 0.5f);
			p -= __builtin_floorf(p);
			d2[d] = lv.smooth ? 12.0f * (0.5f - p) : 0.0f;
		}
		float v[NC];
#pragma unroll
		for (uint32_t idx = 0; idx < NC; ++idx) {
			float acc = 0.0f;
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) acc += val[s][idx][f] * gy[s][f];
			v[idx] = acc;
		}
		const uint32_t i = first + s * GRID_THREADS + threadIdx.x;
#pragma unroll
		for (uint32_t a = 0; a < D; ++a) {
			float grad_out = 0.0f;
#pragma unroll
			for (uint32_t idx = 0; idx < NC; ++idx) {
				const float sa = ((idx >> a) & 1u) ? 1.0f : -1.0f;
				if (lv.smooth) {  // diagonal of the Hessian
					float wgt = s2 * dd[s][a] * d2[a] * sa;
#pragma unroll
					for (uint32_t e = 0; e < D; ++e) {
						if (e != a) wgt *= ((idx >> e) & 1u) ? c[s].w[e][1] : c[s].w[e][0];
					}
					grad_out += wgt * v[idx];
				}
#pragma unroll
				for (uint32_t b = 0; b < D; ++b) {  // mixed terms
					if (b == a) continue;
					float wgt = s2 * dd[s][b] * c[s].derivative[b] * c[s].derivative[a] * sa * (((idx >> b) & 1u) ? 1.0f : -1.0f);
#pragma unroll
					for (uint32_t e = 0; e < D; ++e) {
						if (e != a && e != b) wgt *= ((idx >> e) & 1u) ? c[s].w[e][1] : c[s].w[e][0];
					}
					grad_out += wgt * v[idx];
				}
			}
			if (i < io.n) partial[((size_t)level * D + a) * io.n + i] = grad_out;
		}
	}
}

template <uint32_t D, uint32_t F, uint32_t SPT>
__global__ void __launch_bounds__(GRID_THREADS) k_grid_backward_backward_input_f32_tiles(const GridMeta meta, const GridIO io, const ForwardPlan plan, const float* __restrict__ dL_dy,
                                                                                          const float* __restrict__ params, float* __restrict__ partial) {
	ForwardPlan::Segment mine;
	uint32_t tile;
	if (!forward_plan_item(meta, io, plan, mine, tile)) return;
	const Level<D> lv = level_of_segment<D>(meta, mine);
	const float* __restrict__ grid = params + (size_t)mine.offset * F;
	if (lv.fast) {  // wave-uniform: one lean code path per level kind
		second_order_input_tile<D, F, SPT, true>(lv, io, grid, dL_dy, mine.level, tile * GRID_THREADS * SPT, partial);
	} else {
		second_order_input_tile<D, F, SPT, false>(lv, io, grid, dL_dy, mine.level, tile * GRID_THREADS * SPT, partial);
	}
}

// dL_dx[i][d] = ((0 + partial[0][d][i]) + partial[1][d][i]) + ...: one thread per (d, i), the rows read coalesced
__global__ void __launch_bounds__(256) k_f32_sum_levels(const uint32_t n, const uint32_t n_dims, const uint32_t n_levels_on, const float* __restrict__ partial, float* __restrict__ dL_dx,
                                                        const uint32_t dx_stride_i, const uint32_t dx_stride_d) {
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	if (e >= n * n_dims) return;
	const uint32_t d = e / n, i = e - d * n;
	float out = 0.0f;
	for (uint32_t level = 0; level < n_levels_on; ++level) out += partial[(size_t)level * n_dims * n + e];
	dL_dx[(size_t)i * dx_stride_i + (size_t)d * dx_stride_d] = out;
}

bool grid_backward_backward_input_f32_is_tiled(const GridMeta& meta, bool per_sample_max_level) {
	return (g_fp32_grid_second_order.load() & 2) != 0 && !per_sample_max_level && meta.interp != (uint32_t)InterpolationType::Nearest;
}

size_t grid_backward_backward_input_f32_partial_bytes(const GridMeta& meta, uint32_t n) { return (size_t)levels_on(meta) * meta.n_dims * n * sizeof(float); }

void grid_backward_backward_input_f32_tiled(hipStream_t stream, const GridMeta& meta, const GridIO& io, const float* dL_dy, const float* params, float* dL_dx, uint32_t dx_stride_i,
                                            uint32_t dx_stride_d, float* partial) {
	if (io.n == 0) return;
	if (!io.ddx) throw std::runtime_error("grid second-order pass: dL_ddLdinput is required");
	if (io.max_level || meta.interp == (uint32_t)InterpolationType::Nearest || ((uintptr_t)params & 15u) != 0) {
		throw std::runtime_error("grid second-order pass: the tiled input gradient does not take this form (grid_backward_backward_input does)");
	}
	if ((uint64_t)io.n * meta.n_dims > 0xFFFFFFFFull) throw std::runtime_error("grid second-order pass: batch too large");
	const uint32_t n_on = levels_on(meta);
	if (n_on && !partial) throw std::runtime_error("grid second-order pass: the tiled input gradient needs its scratch array");
	if (n_on) {
		GridMeta on = meta;  // the plan's items: the levels that are on
		on.n_levels = n_on;
		on.max_level = 1.0f;
		grid_dispatch(meta, [&](auto D, auto F) {
			constexpr uint32_t SPT = f32_second_order_spt(D, F);
			const ForwardPlan plan = make_forward_plan(on, io.n, GRID_THREADS * SPT, sizeof(float));
			TCNN_LAUNCH((k_grid_backward_backward_input_f32_tiles<D, F, SPT>), dim3(forward_plan_blocks(plan)), dim3(GRID_THREADS), 0, stream, meta, io, plan, dL_dy, params, partial);
		});
	}
	TCNN_LAUNCH(k_f32_sum_levels, dim3(div_round_up(io.n * meta.n_dims, 256u)), dim3(256), 0, stream, io.n, meta.n_dims, n_on, (const float*)partial, dL_dx, dx_stride_i, dx_stride_d);
}

}  // namespace tcnn_hip

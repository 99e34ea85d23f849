// grid_backward_f32.hip -- the owner-computed backward of an fp32 grid encoding: parameters, dL_dy and the gradient stay float, the sums are
// exact.  No floating-point atomics on global memory, no memset of the table, a result that does not depend on the order of the samples.
// grid_backward_plan.h (F32OwnerPlan) states the plan, the record and the quantum rule; the launches, in order:
//   k_f32_clear    zeroes the control block at the head of the workspace (slice counts, run starts, cursors): a kernel, not a memset node, and
//                  no state survives a call;
//   k_f32_records  <COUNT> one (level, sample tile) per workgroup: streams the tile's positions and dL_dy (every load of a lane issued before
//                  its first use), counts the tile's records per table slice in LDS and adds the non-zero counts to the slices' global counts;
//   k_f32_scan     one workgroup: exclusive prefix of all slice counts -- slice s owns records [start[s], start[s] + count[s]) of the queue;
//   k_f32_records  <scatter> the same tiles again: derives each corner ONCE more with its fp32 term, ranks it within its slice by an integer
//                  LDS atomic, reserves the tile's part of every slice's run with one global integer atomic per non-empty slice, and writes
//                  the records {entry within the slice, F terms} there (the second-order scatter, io.ddx set: k_f32_second_order_records of
//                  grid_second_order_f32.hip in this place -- the same entries, so the same counts and runs, with the second-order term);
//   k_f32_owner    a workgroup per slice: streams its run twice -- first the largest |term| of every value (integer LDS maxima), which fixes
//                  the value's quantum, then every term rounded once on that quantum into a 64-bit LDS sum (ds_add_u64: dense integer LDS
//                  atomics cost 11 clk per wave instruction, floating-point ones ~170; the second pass finds the run in L2) -- converts each
//                  sum to fp32 once and stores it, or adds it to the stored value, once per entry, under GradientMode::Accumulate.
#include "grid_backward_plan.h"

namespace tcnn_hip {

__global__ void __launch_bounds__(256) k_f32_clear(uint32_t* __restrict__ control, const uint32_t n_words) {  // n_words: a multiple of 4
	for (uint32_t w = (blockIdx.x * 256u + threadIdx.x) * 4u; w < n_words; w += gridDim.x * 1024u) *(u4*)(control + w) = u4{0u, 0u, 0u, 0u};
}

// the records of one sample on one level: entry index and weight of each corner, as k_grid_backward_atomic_f32 derives them
template <uint32_t D, bool FAST>
TCNN_DEVICE void f32_corners(const Level<D>& lv, const float (&x)[D], uint32_t (&index)[1u << D], float (&weight)[1u << D]) {
	const Cell<D> c = make_cell<D, FAST>(lv, x);
#pragma unroll
	for (uint32_t idx = 0; idx < (1u << D); ++idx) {
		index[idx] = corner_index<D, FAST>(lv, c, idx);
		weight[idx] = lv.nearest ? 1.0f : corner_weight<D>(c, idx);
	}
}

// COUNT: the counting launch; else the scatter (the records themselves).  One body, so that both derive the same records from the same
// arithmetic: the runs the scan lays out are exactly as long as what the scatter writes.
template <uint32_t D, uint32_t F, bool COUNT>
__global__ void __launch_bounds__(F32_SCATTER_THREADS) k_f32_records(const GridMeta meta, const GridIO io, const F32OwnerPlan plan, const float* __restrict__ dL_dy,
                                                                     uint32_t* __restrict__ control, uint32_t* __restrict__ queues) {
	constexpr uint32_t N_CORNERS = 1u << D, SPT = F32_RECORDS_PER_LANE >> D, TILE = SPT * F32_SCATTER_THREADS, W = f32_record_words(F);
	TCNN_DYN_LDS(lds_raw);
	const uint32_t j = blockIdx.x / plan.tiles, tile = blockIdx.x % plan.tiles;
	const uint32_t level = plan.level[j], nb = plan.n_slices[j], shift = plan.shift[j];
	if (!io.max_level && level_is_off<false>(meta, level, F)) return;  // no records: the owners store zeros
	const Level<D> lv = make_level<D>(meta, level);
	uint32_t* cnt = (uint32_t*)lds_raw;  // [nb] records of this tile per slice
	uint32_t* run = cnt + nb;            // [nb] scatter: where the tile's records of a slice begin in the queue
	for (uint32_t b = threadIdx.x; b < nb; b += F32_SCATTER_THREADS) cnt[b] = 0u;

	float x[SPT][D], g[SPT][F];
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		const uint32_t i = min(tile * TILE + s * F32_SCATTER_THREADS + threadIdx.x, io.n - 1u);  // clamped: lanes past the batch are masked below
		load_position<D>(io, i, x[s]);
		if constexpr (!COUNT) {
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) g[s][f] = dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
		}
	}
	__syncthreads();

	const uint32_t n_corners = lv.nearest ? 1u : N_CORNERS;
	uint32_t index[SPT][N_CORNERS], rank[SPT][N_CORNERS];
	float weight[SPT][N_CORNERS];
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
		const uint32_t i = tile * TILE + s * F32_SCATTER_THREADS + threadIdx.x;
		bool live = i < io.n;
		if (live && io.max_level && level_is_off<false>(meta, io, i, level, F)) live = false;  // per-sample max_level: no records
		if (lv.fast) f32_corners<D, true>(lv, x[s], index[s], weight[s]);
		else f32_corners<D, false>(lv, x[s], index[s], weight[s]);
#pragma unroll
		for (uint32_t idx = 0; idx < N_CORNERS; ++idx) {
			if (!live || idx >= n_corners) {
				index[s][idx] = BUCKET_INVALID_INDEX;
			} else {
				rank[s][idx] = atomic_add_u32(&cnt[index[s][idx] >> shift], 1u);
			}
		}
	}
	__syncthreads();

	uint32_t* __restrict__ slice_words = control + (COUNT ? plan.count_base : plan.cursor_base) + plan.slice_base[j];
	for (uint32_t b = threadIdx.x; b < nb; b += F32_SCATTER_THREADS) {
		const uint32_t c = cnt[b];
		if constexpr (COUNT) {
			if (c) atomic_add_u32(&slice_words[b], c);
		} else {
			run[b] = c ? atomic_add_u32(&slice_words[b], c) : 0u;
		}
	}
	if constexpr (!COUNT) {
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
				for (uint32_t f = 0; f < F; ++f) queue_store(dst + 1 + f, __builtin_bit_cast(uint32_t, weight[s][idx] * g[s][f]));  // (T)weight * grad, T = float (grid.h:254)
			}
		}
	}
}

// exclusive prefix over all slices' counts: one workgroup, a contiguous share per thread, a Hillis-Steele scan of the shares in LDS
__global__ void __launch_bounds__(SLICED_THREADS) k_f32_scan(const F32OwnerPlan plan, uint32_t* __restrict__ control) {
	__shared__ uint32_t share[SLICED_THREADS];
	const uint32_t S = plan.n_slices_total, per = div_round_up(S, SLICED_THREADS);
	const uint32_t b0 = min(threadIdx.x * per, S), b1 = min(b0 + per, S);
	uint32_t sum = 0;
	for (uint32_t b = b0; b < b1; ++b) sum += control[plan.count_base + b];
	share[threadIdx.x] = sum;
	__syncthreads();
	for (uint32_t d = 1; d < SLICED_THREADS; d <<= 1) {
		const uint32_t below = threadIdx.x >= d ? share[threadIdx.x - d] : 0u;
		__syncthreads();
		share[threadIdx.x] += below;
		__syncthreads();
	}
	uint32_t running = share[threadIdx.x] - sum;
	for (uint32_t b = b0; b < b1; ++b) {
		control[plan.start_base + b] = running;
		control[plan.cursor_base + b] = running;
		running += control[plan.count_base + b];
	}
}

// the quantum's exponent of a value whose largest finite |term| has the bits `max_bits` (0: no term, or zeros only): that term is below
// 2^e with e = (biased exponent, at least 1) - 126
TCNN_DEVICE int f32_quantum_exponent(uint32_t max_bits, uint32_t log2_terms) {
	const int biased = (int)(max_bits >> 23);
	return (biased < 1 ? 1 : biased) - 126 + (int)log2_terms - 62;
}

template <uint32_t F>
__global__ void __launch_bounds__(SLICED_THREADS) k_f32_owner(const GridLevelTable table, const F32OwnerPlan plan, const uint32_t* __restrict__ control,
                                                              const uint32_t* __restrict__ queues, float* __restrict__ grid_gradient, const int accumulate) {
	constexpr uint32_t W = f32_record_words(F), V = F32_OWNER_VALUES;
	TCNN_DYN_LDS(lds_raw);
	unsigned long long* tab = (unsigned long long*)lds_raw;  // [entries][F] sums of quanta
	uint32_t* largest = (uint32_t*)(tab + V);                // [entries][F] bits of the largest finite |term|
	uint32_t* flags = largest + V;                           // 4 bits per value
	uint32_t j = 0;
	while (j + 1 < plan.n_levels && blockIdx.x >= plan.slice_base[j + 1]) ++j;
	const uint32_t slice = blockIdx.x - plan.slice_base[j];
	const uint32_t level = plan.level[j], entries = table.offset[level + 1] - table.offset[level];
	const uint32_t entries_per_slice = 1u << plan.shift[j], slice_begin = slice * entries_per_slice;
	const uint32_t n_values = min(entries_per_slice, entries - slice_begin) * F;  // (slice < ceil(entries / entries_per_slice))
	const uint32_t start = min(control[plan.start_base + blockIdx.x], plan.n_queue_records);
	const uint32_t count = min(control[plan.count_base + blockIdx.x], plan.n_queue_records - start);  // (the runs lie inside the queue by construction)

	for (uint32_t w = threadIdx.x; w < F32_OWNER_LDS_BYTES / 16u; w += SLICED_THREADS) ((u4*)lds_raw)[w] = u4{0u, 0u, 0u, 0u};
	__syncthreads();

	// U records in flight per lane: the run is streamed at memory speed, not at one round trip per record
	constexpr uint32_t U = F <= 2 ? 4 : 2;
	const uint32_t* __restrict__ q = queues + (size_t)start * W;
	auto stream = [&](auto&& term) {
		for (uint32_t base = threadIdx.x; base < count; base += SLICED_THREADS * U) {
			uint32_t rec[U][W];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) {
				const uint32_t r = min(base + u * SLICED_THREADS, count - 1u);
#pragma unroll
				for (uint32_t w = 0; w < W; ++w) rec[u][w] = q[(size_t)r * W + w];
			}
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) {
				if (base + u * SLICED_THREADS >= count) continue;
				const uint32_t v0 = (rec[u][0] & (entries_per_slice - 1u)) * F;
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) term(v0 + f, rec[u][1 + f]);
			}
		}
	};
	stream([&](uint32_t v, uint32_t bits) {
		const uint32_t magnitude = bits & 0x7FFFFFFFu;
		if (magnitude < 0x7F800000u) {
			if (magnitude) atomicMax(&largest[v], magnitude);  // (the bits of non-negative floats order as the floats do)
		} else {  // not finite: a flag instead of a term (see the plan)
			const uint32_t flag = magnitude > 0x7F800000u ? F32_FLAG_NAN : ((bits >> 31) ? F32_FLAG_NEG_INF : F32_FLAG_POS_INF);
			atomicOr(&flags[v >> 3], flag << (4u * (v & 7u)));
		}
	});
	__syncthreads();
	stream([&](uint32_t v, uint32_t bits) {
		const uint32_t magnitude = bits & 0x7FFFFFFFu;
		if (magnitude == 0u || magnitude >= 0x7F800000u) return;
		const int q_exp = f32_quantum_exponent(largest[v], plan.log2_terms);
		const long long quanta = (long long)__builtin_rint(__builtin_ldexp((double)__builtin_bit_cast(float, bits), -q_exp));  // exact scaling, one rounding to nearest (even)
		if (quanta != 0) lds_atomic_add_u64(&tab[v], (unsigned long long)quanta);
	});
	__syncthreads();

	float* __restrict__ grad = grid_gradient + ((size_t)table.offset[level] + slice_begin) * F;
	for (uint32_t v = threadIdx.x; v < n_values; v += SLICED_THREADS) {
		// ONE conversion of the sum, then an exact scaling by the quantum; a flagged value as a floating-point sum would have ended
		float value = __builtin_ldexpf((float)(long long)tab[v], f32_quantum_exponent(largest[v], plan.log2_terms));
		const uint32_t flag = (flags[v >> 3] >> (4u * (v & 7u))) & 15u;
		if (flag) {
			const bool nan = (flag & F32_FLAG_NAN) || (flag & (F32_FLAG_POS_INF | F32_FLAG_NEG_INF)) == (F32_FLAG_POS_INF | F32_FLAG_NEG_INF);
			value = nan ? __builtin_nanf("") : ((flag & F32_FLAG_POS_INF) ? __builtin_inff() : -__builtin_inff());
		}
		grad[v] = accumulate ? grad[v] + value : value;  // Accumulate: added to the stored value, once per entry
	}
}

void launch_f32_owner_backward(hipStream_t stream, const GridMeta& meta, const GridIO& io, const F32BackwardPlan& bp, const float* dL_dy, void* workspace,
                               float* grid_gradient, bool accumulate) {
	const F32OwnerPlan& plan = bp.owners;
	uint32_t* control = (uint32_t*)workspace;
	uint32_t* queues = (uint32_t*)((unsigned char*)workspace + bp.queue_offset);
	TCNN_LAUNCH(k_f32_clear, dim3(std::min(div_round_up(plan.control_words, 1024u), 2048u)), dim3(256), 0, stream, control, plan.control_words);
	uint32_t max_slices = 0;
	for (uint32_t j = 0; j < plan.n_levels; ++j) max_slices = std::max(max_slices, plan.n_slices[j]);
	const uint32_t record_lds = 2u * max_slices * (uint32_t)sizeof(uint32_t);
	const uint32_t record_blocks = plan.n_levels * plan.tiles;
	GridLevelTable table;
	for (uint32_t l = 0; l <= MAX_N_LEVELS; ++l) table.offset[l] = l <= meta.n_levels ? meta.offset[l] : 0u;
	grid_dispatch(meta, [&](auto D, auto F) {
		TCNN_LAUNCH((k_f32_records<D, F, true>), dim3(record_blocks), dim3(F32_SCATTER_THREADS), record_lds, stream, meta, io, plan, dL_dy, control, queues);
		TCNN_LAUNCH(k_f32_scan, dim3(1), dim3(SLICED_THREADS), 0, stream, plan, control);
		if (io.ddx) {  // the second-order records: the same runs, another term (grid_second_order_f32.hip)
			launch_f32_second_order_scatter(stream, meta, io, plan, dL_dy, control, queues, record_blocks, record_lds);
		} else {
			TCNN_LAUNCH((k_f32_records<D, F, false>), dim3(record_blocks), dim3(F32_SCATTER_THREADS), record_lds, stream, meta, io, plan, dL_dy, control, queues);
		}
		TCNN_SET_MAX_DYN_LDS((k_f32_owner<F>), F32_OWNER_LDS_BYTES);
		TCNN_LAUNCH((k_f32_owner<F>), dim3(plan.n_slices_total), dim3(SLICED_THREADS), F32_OWNER_LDS_BYTES, stream, table, plan, (const uint32_t*)control, (const uint32_t*)queues,
		            grid_gradient, accumulate ? 1 : 0);
	});
}

}  // namespace tcnn_hip

// grid_backward_scatter.hip -- pass A of the bucketed backward: every corner record derived once and appended to its owner's queue.
#include "grid_backward_plan.h"
#include "exp_diag.h"  // experiment switches: compile-time zeros in the product build

namespace tcnn_hip {

// =============================================================================================
// backward, bucket-once form for the large levels.  The slice passes above re-derive every corner of every
// sample once PER SLICE (16 x 13 passes over the batch at the headline config: VALU-bound).  Here each corner
// is derived ONCE:
//   pass A (k_grid_bucket_scatter): a workgroup takes one (level, sample tile), computes the corner records
//     {entry index, (GRAD_T)weight * grad} (grid.h:254), ranks them by table slice ("bucket") with integer LDS
//     atomics, reorders them by bucket in LDS and appends each bucket's run to that bucket's queue in HBM with
//     coalesced stores (one global integer atomic per (workgroup, bucket) reserves the run);
//   pass B (kind SLICE_BUCKET of k_grid_backward_sliced): the workgroup that owns a slice streams its queue and
//     accumulates in 64-bit fixed point in LDS (dense ds_add_u64: 11 clk per wave instruction vs ~170 for the
//     floating-point LDS atomics), then stores the slice -- exact, order-independent, no memset, no float atomics;
//   overflow: records that did not fit their queue (capacity = 2x the uniform expectation) or whose x-neighbour lives in
//     another bucket travel through one list; each owner picks its slice's records out of it before it stores (exact);
//     beyond OVERFLOW_INLINE_MAX records (strongly clustered inputs) the last owner to finish applies the list with the
//     reference's global atomics instead.
// HBM traffic: 2 x 8 B per corner (F = 2) -- 0.44 GB per headline step, a fraction of the chip's bandwidth.
// =============================================================================================
// SECOND_ORDER: scatter d(dL_dx)/d(grid) instead of dy/d(grid) (backward_backward_input's parameter part) -- a compile-time switch: as a
// run-time select the corner weight of the second-order form (three products per dimension and corner) sits next to the first-order one in
// every training step's instruction stream and register budget
template <uint32_t D, uint32_t F, bool SECOND_ORDER>
__global__ void __launch_bounds__(BUCKET_THREADS) k_grid_bucket_scatter(const GridMeta meta, const GridIO io, const BucketPlan plan,
                                                                         const half_t* __restrict__ dL_dy, uint32_t* __restrict__ counters,
                                                                         uint32_t* __restrict__ queues, uint32_t* __restrict__ overflow,
                                                                         half_t* __restrict__ grid_gradient, const int accumulate) {
	constexpr uint32_t N_CORNERS = 1u << D, PW = BucketRecord<F>::PAYLOAD_WORDS, W = BucketRecord<F>::WORDS, PWP = BucketRecord<F>::PAIR_WORDS;
	constexpr uint32_t N_PAIRS_PER_SAMPLE = N_CORNERS / 2;
	constexpr uint32_t SPT = bucket_spt(D, F), TILE = SPT * BUCKET_THREADS, N_PAIR = TILE * N_PAIRS_PER_SAMPLE;
	TCNN_DYN_LDS(lds_raw);
	constexpr uint32_t diag_scatter = EXP_DIAG_SCATTER;  // 0 in the product build (exp_diag.h)
	constexpr uint32_t PAYLOAD_MAGNITUDE = F == 1 ? 0x7FFFFFFFu : 0x7FFF7FFFu;  // a payload word without its sign bit(s): one fp32, or two 16-bit values
	if (blockIdx.x >= plan.scatter_blocks) {
		// gradients of chunked levels are accumulated with atomics by several owners in pass B: zero them here
		const uint32_t z = blockIdx.x - plan.scatter_blocks;
		uint32_t zj = 0;
		while (zj + 1 < plan.n_levels && z >= plan.zero_block_begin[zj + 1]) ++zj;
		const uint32_t zl = plan.level[zj];
		const uint32_t n_halves = (meta.offset[zl + 1] - meta.offset[zl]) * F;  // a multiple of 8
		const uint32_t h = (z - plan.zero_block_begin[zj]) * ZERO_BLOCK_HALVES + threadIdx.x * 8u;
		if (h < n_halves) *(u4*)(grid_gradient + (size_t)meta.offset[zl] * F + h) = u4{0u, 0u, 0u, 0u};
		return;
	}
	// persistent workgroup: `wgs_per_level` of them share the sample tiles of one level
	const uint32_t j = blockIdx.x / plan.wgs_per_level, first_tile = blockIdx.x % plan.wgs_per_level;
	const uint32_t level = plan.level[j], nb = plan.n_buckets[j], shift = plan.shift;
	const bool per_sample = io.max_level != nullptr;
	if (!per_sample && level_is_off<false>(meta, level, F)) return;  // no records, the owners store zeros
	const Level<D> lv = make_level<D>(meta, level);
	const bool linear = !lv.smooth && !lv.nearest;
	// Zero records.  Under the loss scale the products (GRAD_T)weight * dL/dy underflow to +-0 in 16 bits for much of a converged fit.  The owners
	// sum in exact fixed point and store +0 for an entry nothing was added to, so a record of zeros changes no bit of the gradient: a pair whose
	// two payloads are all +-0 is not ranked, staged or queued, and a zero record that would travel through the overflow list is not pushed.
	// The one place that could tell: a chunked level in GradientMode::Accumulate.  Its slices are neither cleared nor stored, only added to where
	// an owner's sum is non-zero, so an entry may still hold the caller's -0 when the last owner drains a long overflow list with global
	// atomics, and -0 + +0 is +0.  Such a level keeps every record (everywhere else the slice has been stored by then and holds no -0).
#if defined(TCNN_TEST_KEEP_ZERO_RECORDS)  // tests/emu: the kernel as it was before zero records were dropped, for the bit-for-bit comparison
#if !defined(TCNN_HOST_EMU)
#error "TCNN_TEST_KEEP_ZERO_RECORDS is a switch of the host emulator's test builds (tests/emu/emu_zero_records.py)"
#endif
	const bool keep_zero = true;
#else
	const bool keep_zero = accumulate != 0 && plan.n_chunks[j] > 1u;
#endif

	// Queue unit: a PAIR of records -- the two corners that differ in dimension 0 only.  Their table entries are
	// neighbours (dense index +1; hashed: prime[0] == 1, so the indices differ in the low bits only) and therefore
	// share a bucket except once in ~2^shift pairs: the second record of such a pair is routed through the overflow
	// list instead.  Halves the ranking / reordering work per corner; a pair is 16 bytes for F == 2.
	uint32_t* stage = (uint32_t*)lds_raw;   // [N_PAIR][PWP]
	uint32_t* cnt = stage + N_PAIR * PWP;   // [nb] pairs of this tile per bucket
	uint32_t* delta = cnt + nb;             // [nb] exclusive prefix of cnt, later (queue position - staging position)
	uint32_t* part = delta + nb;            // [64] scan scratch of wave 0
	uint32_t* total_p = part + 64;          // [1]
	for (uint32_t b = threadIdx.x; b < nb; b += BUCKET_THREADS) cnt[b] = 0u;

	auto push_overflow = [&](uint32_t index, const uint32_t* payload) {
		const uint32_t o = atomic_add_u32(&counters[plan.overflow_counter], 1u);
		if (o < plan.overflow_capacity) {
			uint32_t* dst = overflow + (size_t)o * (W + 1);
			dst[0] = level;
			dst[1] = index;
#pragma unroll
			for (uint32_t p = 0; p < PW; ++p) dst[2 + p] = payload[p];
		}
	};
	auto load_tile = [&](uint32_t tile, float (&x)[SPT][D], half_t (&g)[SPT][F]) {
#pragma unroll
		for (uint32_t s = 0; s < SPT; ++s) {
			const uint32_t i = min(tile * TILE + s * BUCKET_THREADS + threadIdx.x, io.n - 1u);
			load_position<D>(io, i, x[s]);
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) g[s][f] = dL_dy[(size_t)(level * F + f) * io.stride_k + (size_t)i * io.stride_i];
		}
	};

	float x[SPT][D], x_next[SPT][D];
	half_t g[SPT][F], g_next[SPT][F];
	constexpr bool second_order = SECOND_ORDER;
	if (first_tile < plan.tiles) load_tile(first_tile, x, g);
#if !defined(TCNN_HOST_EMU)
	// The first tile's inputs are waited for HERE, not at the loop's top.  gfx9 counts loads and stores in one counter (vmcnt); the waits
	// the compiler places in the loop header serve the first iteration (inputs still on their way) and every later one (inputs long there:
	// the wait for the reservation atomics covered them) alike, and on the later ones "s_waitcnt vmcnt(0)" sits out the round trip of the
	// queue stores the previous tile's append loop has just issued -- once per tile and workgroup.
#pragma unroll
	for (uint32_t s = 0; s < SPT; ++s) {
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) asm volatile("" : "+v"(x[s][d]));
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) asm volatile("" : "+v"(g[s][f]));
	}
#endif
	__syncthreads();

	float level_abs_sum = 0.0f;  // (bfloat16 build)
	for (uint32_t tile = first_tile; tile < plan.tiles; tile += plan.wgs_per_level) {
		const uint32_t chunk = tile / plan.tiles_per_chunk[j];
		uint32_t* __restrict__ my_counters = counters + plan.counter_base[j] + chunk * nb;

		// (bfloat16 build) a sample's share of the level's sum that picks the owners' exponent (OwnerScale) starts from max_f |dL/dy|
		auto max_abs_dy = [&](uint32_t s) {
			float m = 0.0f;
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) m = __builtin_fmaxf(m, __builtin_fabsf((float)g[s][f]));
			return m;
		};
		// a per-sample max_level: bit s = sample s of this lane is off for the level -- it emits no record (and adds nothing to the level's sum)
		uint32_t off_mask = 0u;
		if (!SECOND_ORDER && per_sample) {  // (the second-order instance tests inside derive(), next to its ddx loads: no mask to keep alive)
#pragma unroll
			for (uint32_t s = 0; s < SPT; ++s) {
				if (level_is_off<false>(meta, io, min(tile * TILE + s * BUCKET_THREADS + threadIdx.x, io.n - 1u), level, F)) off_mask |= 1u << s;
			}
		}
		// first order: the corner weights of a sample add up to one, so the sum of |dL/dy| over the workgroup's tiles is the sum of what is
		// emitted.  (The second-order pass gathers its sum inside derive() below, where the weights are known.)
		if constexpr (HALF_IS_BF16 && !second_order) {
#pragma unroll
			for (uint32_t s = 0; s < SPT; ++s) {
				if (tile * TILE + s * BUCKET_THREADS + threadIdx.x < io.n && !((off_mask >> s) & 1u)) level_abs_sum += __builtin_fminf(max_abs_dy(s), LEVEL_SUM_CLAMP);  // (NaN -> the other operand: the bound test sees it)
			}
		}
		// ---- derive the records of my samples; rank each pair within its bucket
		uint32_t ridx[SPT][N_CORNERS], rank[SPT][N_PAIRS_PER_SAMPLE], pay[SPT][N_CORNERS][PW];
		// FAST, LINEAR: the table's kind and the interpolation are properties of the level, decided once ahead of the records (below).  As
		// run-time values the interpolation costs every sample the Smoothstep polynomial of each dimension and a select per weight.
		auto derive = [&](auto fast_arg, auto linear_arg) {
			constexpr bool FAST = decltype(fast_arg)::value, LINEAR = decltype(linear_arg)::value;
			const bool nearest = LINEAR ? false : lv.nearest;
#pragma unroll
			for (uint32_t s = 0; s < SPT; ++s) {
				bool valid = tile * TILE + s * BUCKET_THREADS + threadIdx.x < io.n && !((off_mask >> s) & 1u);
				if constexpr (second_order) {
					if (per_sample && level_is_off<false>(meta, io, min(tile * TILE + s * BUCKET_THREADS + threadIdx.x, io.n - 1u), level, F)) valid = false;
				}
				const Cell<D> c = make_cell<D, FAST, LINEAR>(lv, x[s]);
				float dd[D];
#pragma unroll
				for (uint32_t d = 0; d < D; ++d) dd[d] = 0.0f;
				if constexpr (second_order) load_ddx<D>(io, min(tile * TILE + s * BUCKET_THREADS + threadIdx.x, io.n - 1u), dd);
				float weight_abs_sum = 0.0f;  // (second order, bfloat16 build)
#pragma unroll
				for (uint32_t idx = 0; idx < N_CORNERS; ++idx) {
					float weight;
					if constexpr (second_order) weight = corner_weight_second_order<D>(lv, c, idx, dd);
					else weight = nearest ? 1.0f : corner_weight<D>(c, idx);
					if constexpr (second_order && HALF_IS_BF16) weight_abs_sum += __builtin_fabsf(weight);
					if constexpr (F == 1) {
						pay[s][idx][0] = __builtin_bit_cast(uint32_t, weight * (float)g[s][0]);
					} else {
						const half_t wh = to_half_rn(weight);  // (GRAD_T)weight, grid.h:254
						const h2 w2 = h2{wh, wh};
#pragma unroll
						for (uint32_t p = 0; p < PW; ++p) pay[s][idx][p] = h2_bits(w2 * h2{g[s][2 * p], g[s][2 * p + 1]});
					}
					ridx[s][idx] = corner_index<D, FAST>(lv, c, idx);
				}
				if constexpr (second_order && HALF_IS_BF16) {
					// the second-order records are dy * weight with weights of the size of ddx * scale, not of one: the level's sum (OwnerScale) is
					// taken from what is emitted -- from |dL/dy| alone small ddx left every record below 2^-k and large ones sent every slice wide
					if (valid) level_abs_sum += __builtin_fminf(max_abs_dy(s) * weight_abs_sum, LEVEL_SUM_CLAMP);
				}
				// Hashed levels (prime[0] == 1): the two entries of EVERY pair of a sample differ by the same low bits, x ^ (x + 1) under the table's
				// mask -- whether a pair's second record can ride with the first (same bucket; derivable from word 0 by construction) and the
				// flip count t are properties of the sample, not of the pair
				uint32_t fast_tag = 0;
				bool fast_together = true;
				if constexpr (FAST) {
					const uint32_t flips = c.hlo[0] ^ c.hhi[0];
					fast_together = ((flips & lv.mask) >> shift) == 0u;
					fast_tag = fast_together ? ((((uint32_t)__builtin_popcount(flips) - 1u) << PAIR_INDEX_BITS) | PAIR_HAS_SECOND) : 0u;
				}
#pragma unroll
				for (uint32_t pr = 0; pr < N_PAIRS_PER_SAMPLE; ++pr) {
					// a record whose payload is +-0 in every word adds nothing to the owners' exact sums: it is not created (see keep_zero above)
					uint32_t mag0 = 0u, mag1 = 0u;
#pragma unroll
					for (uint32_t p = 0; p < PW; ++p) {
						mag0 |= pay[s][2 * pr][p];
						mag1 |= pay[s][2 * pr + 1][p];
					}
					const bool nz0 = keep_zero || (mag0 & PAYLOAD_MAGNITUDE) != 0u, nz1 = keep_zero || (mag1 & PAYLOAD_MAGNITUDE) != 0u;
					if constexpr (EXP_COUNT_ZERO_PAIRS) {  // (false in the product build, exp_diag.h: the pairs of the level, and the all-zero ones among them)
						if (valid && (pr == 0u || !nearest)) exp_count_pair(level, ((mag0 | (nearest ? 0u : mag1)) & PAYLOAD_MAGNITUDE) == 0u);
					}
					const bool live = valid && (pr == 0u || !nearest) && (nz0 || (nz1 && !nearest));
					const uint32_t bucket = ridx[s][2 * pr] >> shift;
					if (!live) {
						ridx[s][2 * pr] = BUCKET_INVALID_INDEX;
						ridx[s][2 * pr + 1] = BUCKET_INVALID_INDEX;
					} else if (nearest) {
						ridx[s][2 * pr + 1] = BUCKET_INVALID_INDEX;
					} else if constexpr (FAST) {
						if (!fast_together) {
							if (nz1) push_overflow(ridx[s][2 * pr + 1], pay[s][2 * pr + 1]);
							ridx[s][2 * pr + 1] = BUCKET_INVALID_INDEX;
						}
						ridx[s][2 * pr] |= fast_tag;
					} else {
						// word 0 of the pair (t = 0: a dense index has its neighbour at index + 1); the second entry must be derivable from it
						// AND live in the same bucket, otherwise (about one pair in 2^shift) it travels through the overflow list
						const uint32_t word0 = ridx[s][2 * pr] | PAIR_HAS_SECOND;
						const uint32_t i1 = ridx[s][2 * pr + 1];
						if ((i1 >> shift) != bucket || pair_second_index<D>(lv, word0) != i1) {
							if (nz1) push_overflow(i1, pay[s][2 * pr + 1]);
							ridx[s][2 * pr + 1] = BUCKET_INVALID_INDEX;
						} else {
							ridx[s][2 * pr] = word0;
						}
					}
					rank[s][pr] = live && !(diag_scatter & 8u) ? atomic_add_u32(&cnt[bucket], 1u) : 0u;
				}
			}
		};
		if (lv.fast) {
			if (linear) derive(std::true_type{}, std::true_type{}); else derive(std::true_type{}, std::false_type{});
		} else {
			if (linear) derive(std::false_type{}, std::true_type{}); else derive(std::false_type{}, std::false_type{});
		}
		// the next tile's inputs travel while this one is ranked, reordered and written
		const uint32_t next_tile = tile + plan.wgs_per_level;
		if (next_tile < plan.tiles) load_tile(next_tile, x_next, g_next);
		__syncthreads();

		// ---- reserve this tile's run in every bucket queue (one returning global atomic per non-empty bucket; the
		// common case has one bucket per thread and hides the round trip behind the scan and the reordering) ...
		uint32_t reserved = 0;
		if (nb <= BUCKET_THREADS && threadIdx.x < nb) {
			const uint32_t c = cnt[threadIdx.x];
			if (c && !(diag_scatter & 2u)) reserved = atomic_add_u32(&my_counters[threadIdx.x], c);
		}
		// ... while wave 0 turns the counts into staging offsets (exclusive scan, wave-synchronous)
		if (threadIdx.x < WAVE) {
			const uint32_t per_lane = div_round_up(nb, WAVE);
			const uint32_t b_begin = min(threadIdx.x * per_lane, nb), b_end = min(b_begin + per_lane, nb);
			uint32_t sum = 0;
			for (uint32_t b = b_begin; b < b_end; ++b) sum += cnt[b];
			// exclusive prefix over the wave's lanes in registers: sibling blocks of 1, 2, 4, ... lanes merge, a lane in the upper sibling adds
			// the lower sibling's total (six cross-lane moves; the LDS ladder this replaces cost eighteen LDS round trips while three waves wait)
			uint32_t block_total = sum, running = 0;
#pragma unroll
			for (uint32_t d = 1; d < WAVE; d <<= 1) {
				const uint32_t sibling = (uint32_t)__shfl_xor((int)block_total, (int)d, 64);
				if (threadIdx.x & d) running += sibling;
				block_total += sibling;
			}
			for (uint32_t b = b_begin; b < b_end; ++b) {
				delta[b] = running;
				running += cnt[b];
			}
			if (threadIdx.x == WAVE - 1) total_p[0] = block_total;
		}
		__syncthreads();
		const uint32_t total = total_p[0];

		// ---- reorder by bucket in LDS
#pragma unroll
		for (uint32_t s = 0; s < SPT; ++s) {
#pragma unroll
			for (uint32_t pr = 0; pr < N_PAIRS_PER_SAMPLE; ++pr) {
				const uint32_t word0 = ridx[s][2 * pr];  // index | t | has_second (BUCKET_INVALID_INDEX: no pair)
				if (word0 == BUCKET_INVALID_INDEX) continue;
				const uint32_t pos = delta[(word0 & PAIR_INDEX_MASK) >> shift] + rank[s][pr];
				if (diag_scatter & 4u) continue;
#if defined(TCNN_HOST_EMU)
				uint32_t* dst = stage + pos * PWP;
#else
				uint32_t* dst = stage + __umul24(pos, PWP);  // pos < N_PAIR: one 24-bit multiply (as 32-bit index arithmetic it became a 64-bit multiply-add)
#endif
				dst[0] = word0;
#pragma unroll
				for (uint32_t p = 0; p < PW; ++p) {
					dst[1 + p] = pay[s][2 * pr][p];
					dst[1 + PW + p] = pay[s][2 * pr + 1][p];
				}
			}
		}
		__syncthreads();
#if !defined(TCNN_HOST_EMU)
		// (the next tile's inputs, requested before the ranking barrier, are waited for here -- ahead of this tile's queue stores, see the
		// note at the first tile's loads: nothing of this lane's is in flight when the stores go out, and nothing waits behind them)
#pragma unroll
		for (uint32_t s = 0; s < SPT; ++s) {
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) asm volatile("" : "+v"(x_next[s][d]));
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) asm volatile("" : "+v"(g_next[s][f]));
		}
#endif
		// delta[b] := (position of the run in bucket b's queue) - (position of the run in the staging area);
		// the counts are dead from here on: clear them for the next tile
		if (nb <= BUCKET_THREADS) {
			if (threadIdx.x < nb) {
				delta[threadIdx.x] = reserved - delta[threadIdx.x];
				cnt[threadIdx.x] = 0u;
			}
		} else {
			for (uint32_t b = threadIdx.x; b < nb; b += BUCKET_THREADS) {
				const uint32_t c = cnt[b];
				delta[b] = (c ? atomic_add_u32(&my_counters[b], c) : 0u) - delta[b];
				cnt[b] = 0u;
			}
		}
		__syncthreads();

		// ---- append the runs to the bucket queues: consecutive threads -> consecutive pairs
		const uint32_t cap = plan.capacity[j];
		uint32_t* __restrict__ q = queues + (plan.queue_base[j] + (size_t)chunk * nb * cap) * PWP;
		for (uint32_t t = threadIdx.x; t < total; t += BUCKET_THREADS) {
			uint32_t rec[PWP];
#pragma unroll
			for (uint32_t w = 0; w < PWP; ++w) rec[w] = stage[t * PWP + w];
			const uint32_t b = (rec[0] & PAIR_INDEX_MASK) >> shift;
			const uint32_t pos = t + delta[b];  // wraps like the subtraction above
			if (pos < cap) {
				uint32_t* dst = q + ((size_t)b * cap + pos) * PWP;
				if (diag_scatter & 1u) continue;
#pragma unroll
				for (uint32_t w = 0; w < PWP; ++w) queue_store(dst + w, rec[w]);
			} else {
				// (a pair is queued when either record is non-zero: the zero half of a spilled pair stays out of the list like any zero record)
				uint32_t mag0 = 0u, mag1 = 0u;
#pragma unroll
				for (uint32_t p = 0; p < PW; ++p) {
					mag0 |= rec[1 + p];
					mag1 |= rec[1 + PW + p];
				}
				if (keep_zero || (mag0 & PAYLOAD_MAGNITUDE)) push_overflow(rec[0] & PAIR_INDEX_MASK, &rec[1]);
				if ((rec[0] & PAIR_HAS_SECOND) && (keep_zero || (mag1 & PAYLOAD_MAGNITUDE))) push_overflow(pair_second_index<D>(lv, rec[0]), &rec[1 + PW]);
			}
		}
		__syncthreads();  // the staging area and the offsets are reused by the next tile
#pragma unroll
		for (uint32_t s = 0; s < SPT; ++s) {
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) x[s][d] = x_next[s][d];
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) g[s][f] = g_next[s][f];
		}
	}
	// ONE 64-bit integer atomic per workgroup, into one of the level's LEVEL_SUM_PARTS words (per wave and tile -- 2048 same-address atomics
	// per level -- the atomics serialised in their L2 channel and the pass took five times as long)
	if constexpr (HALF_IS_BF16) {
		const float wave_total = wave_sum_f32(level_abs_sum);
		if (lane_id() == 0) part[threadIdx.x / WAVE] = __builtin_bit_cast(uint32_t, wave_total);
		__syncthreads();
		if (threadIdx.x == 0) {
			float total = 0.0f;
			for (uint32_t w = 0; w < BUCKET_THREADS / WAVE; ++w) total += __builtin_bit_cast(float, part[w]);
			level_sum_add((unsigned long long*)(counters + plan.level_sum_base + 2u * (j * LEVEL_SUM_PARTS + (blockIdx.x % LEVEL_SUM_PARTS))), level_sum_units(total));
		}
	}
}

void launch_bucket_scatter(hipStream_t stream, const GridMeta& meta, const GridIO& io, const BucketPlan& plan, const half_t* dL_dy, uint32_t* counters,
                           uint32_t* queues, uint32_t* overflow, half_t* grid_gradient, bool accumulate) {
	// the scatter's workgroups, then the blocks that zero the gradients of chunked levels
	const uint32_t blocks = plan.scatter_blocks + plan.zero_block_begin[plan.n_levels];
	uint32_t max_buckets = 0;
	for (uint32_t j = 0; j < plan.n_levels; ++j) max_buckets = std::max(max_buckets, plan.n_buckets[j]);
	grid_dispatch(meta, [&](auto D, auto F) {
		const uint32_t lds = bucket_spt(D, F) * BUCKET_THREADS * ((1u << D) / 2u) * pair_words(F) * 4u + (2u * max_buckets + WAVE + 4u) * 4u;
		if (io.ddx) {
			TCNN_SET_MAX_DYN_LDS((k_grid_bucket_scatter<D, F, true>), lds);
			TCNN_LAUNCH((k_grid_bucket_scatter<D, F, true>), dim3(blocks), dim3(BUCKET_THREADS), lds, stream, meta, io, plan, dL_dy, counters, queues, overflow,
			            grid_gradient, accumulate ? 1 : 0);
		} else {
			TCNN_SET_MAX_DYN_LDS((k_grid_bucket_scatter<D, F, false>), lds);
			TCNN_LAUNCH((k_grid_bucket_scatter<D, F, false>), dim3(blocks), dim3(BUCKET_THREADS), lds, stream, meta, io, plan, dL_dy, counters, queues, overflow,
			            grid_gradient, accumulate ? 1 : 0);
		}
	});
}

}  // namespace tcnn_hip

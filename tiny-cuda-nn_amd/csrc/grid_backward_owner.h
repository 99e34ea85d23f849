// grid_backward_owner.h -- pass B of the bucketed backward, the part both owner kernels share: what an owner workgroup knows (OwnerSlice), the
// pieces every accumulator form is made of, the epilogue, and the 64-bit-per-value owner that k_grid_backward_sliced runs (F = 1, owner mode 1).
#pragma once
#include "grid_backward_plan.h"

namespace tcnn_hip {

// What an owner workgroup knows: the queues of its slot, its level's place in the gradient and the call's bookkeeping.  k_grid_bucket_owner
// fills it from its item descriptor and scalar kernel arguments, k_grid_backward_sliced from slot j of the BucketPlan.
struct OwnerSlice {
	uint32_t capacity, n_chunks, n_buckets, counter_base;  // the slot: pairs per queue, sample chunks, table slices, first counter
	uint64_t queue_base;                                   // first pair of the slot's queues
	uint32_t table_offset, sum_slot;                       // the level: first entry of its table, slot of its |dL/dy| sums (OwnerScale)
	uint32_t shift, overflow_counter, overflow_capacity, n_owner_blocks, level_sum_base, n_levels;  // the call (BucketPlan)
};

// round(v * 2^24) as a 64-bit integer using fp32 / int32 ops only (no fp64 conversions in the hot loop).
// v is a product of two halves: |v| <= 2^32 and at most 22 significant bits, so v * 2^8 splits exactly into an
// integer part (|hi| <= 2^40 would overflow -> clamp to the fp16 range first: |v| <= 65504 < 2^16 -> |hi| < 2^24)
// and a fraction |r| < 1 that is rounded to 16 bits.
TCNN_DEVICE long long to_fixed(float v) {
	v = __builtin_fminf(__builtin_fmaxf(v, -65504.0f), 65504.0f);
	const float s = v * 256.0f;
	const float hi = __builtin_truncf(s);
	const int lo = (int)__builtin_rintf((s - hi) * 65536.0f);
	return (long long)(int)hi * 65536ll + (long long)lo;
}

TCNN_DEVICE OwnerScale owner_scale(const OwnerSlice& own, const uint32_t* counters) {
	if constexpr (!HALF_IS_BF16) return OwnerScale{24};
	unsigned long long sum = 0;
#pragma unroll
	for (uint32_t p = 0; p < LEVEL_SUM_PARTS; ++p) {
		sum = saturating_add_u64(sum, *(const unsigned long long*)(counters + own.level_sum_base + 2u * (own.sum_slot * LEVEL_SUM_PARTS + p)));
	}
	if (sum == 0ull) return OwnerScale{40};
	const float share = (float)sum * (8.0f / 4294967296.0f) / (float)(own.n_buckets * own.n_chunks);
	int e;
	(void)__builtin_frexpf(share, &e);  // share < 2^e
	const int k = 30 - e;
	return OwnerScale{k < 20 ? 20 : (k > 40 ? 40 : k)};
}

// the 64-bit-per-value forms: IEEE half through to_fixed() (fp32 / int32 operations only); bfloat16 at the slice's exponent
TCNN_DEVICE long long to_fixed64(float v, const OwnerScale& sc) {
	if constexpr (!HALF_IS_BF16) return to_fixed(v);
	const double s = (double)v * sc.up64();
	if (!(__builtin_fabs(s) < 9.0e18)) return 0;  // beyond 64 bits, infinite or NaN: gradients no sum can represent (the reference's atomics would carry NaN / Inf on)
	return (long long)__builtin_rint(s);
}
TCNN_DEVICE half_t from_fixed64(long long q, const OwnerScale& sc) { return (half_t)(float)((double)q * sc.down64()); }

// ---- the pieces both owner forms are made of ----
// entries [begin, begin + extent) of a table of `hashmap_size` entries cut into slices of `entries_per_slice`
TCNN_DEVICE uint32_t slice_extent(uint32_t begin, uint32_t entries_per_slice, uint32_t hashmap_size) {
	return begin < hashmap_size ? min(entries_per_slice, hashmap_size - begin) : 0u;
}
// queue of (chunk, bucket) within the slot, and its records (`capacity` PAIRS of memory whatever its count)
TCNN_DEVICE uint32_t owner_queue(const OwnerSlice& own, uint32_t bucket, uint32_t chunk) { return chunk * own.n_buckets + bucket; }
template <uint32_t F>
TCNN_DEVICE const uint32_t* owner_queue_records(const OwnerSlice& own, const uint32_t* queues, uint32_t queue) {
	return queues + (own.queue_base + (size_t)queue * own.capacity) * BucketRecord<F>::PAIR_WORDS;
}
// Records that did not fit their queue (or whose x-neighbour lives in another bucket: about one pair in 2^shift).  Up to
// OVERFLOW_INLINE_MAX of them every owner picks its own out of the list -- exact, no atomics, no extra launch; beyond
// that (strongly clustered inputs) the last owner to finish sends the list through the reference's global atomics.
struct OwnerOverflow {
	uint32_t n;
	bool inline_scan;
};
TCNN_DEVICE OwnerOverflow owner_overflow(const OwnerSlice& own, const uint32_t* counters) {
	const uint32_t n = min(counters[own.overflow_counter], own.overflow_capacity);
	return {n, n <= OVERFLOW_INLINE_MAX};
}
// overflow records of this slice (level, index) through add(index, payload): the first chunk's owner takes them
template <uint32_t F, uint32_t THREADS, typename ADD>
TCNN_DEVICE void scan_overflow(const OwnerSlice& own, const OwnerOverflow& over, const uint32_t* __restrict__ overflow, uint32_t level, uint32_t bucket,
                               uint32_t chunk, ADD&& add) {
	if (over.inline_scan && chunk == 0u) {
		for (uint32_t t = threadIdx.x; t < over.n; t += THREADS) {
			const uint32_t* rec = overflow + (size_t)t * (BucketRecord<F>::WORDS + 1);
			if (rec[0] == level && (rec[1] >> own.shift) == bucket) add(rec[1], rec + 2);
		}
	}
}
// one record into entry `rel` of a 64-bit-per-value table [entries][F]
template <uint32_t F>
TCNN_DEVICE void add_record_wide(unsigned long long* tab, uint32_t rel, const uint32_t* payload, const OwnerScale& sc) {
	if constexpr (F == 1) {
		lds_atomic_add_u64(&tab[rel], (unsigned long long)to_fixed64(__builtin_bit_cast(float, payload[0]), sc));
	} else {
#pragma unroll
		for (uint32_t p = 0; p < BucketRecord<F>::PAYLOAD_WORDS; ++p) {
			const h2 v = bits_h2(payload[p]);
			lds_atomic_add_u64(&tab[rel * F + 2 * p], (unsigned long long)to_fixed64((float)v[0], sc));
			lds_atomic_add_u64(&tab[rel * F + 2 * p + 1], (unsigned long long)to_fixed64((float)v[1], sc));
		}
	}
}
// values 2 * e2 and 2 * e2 + 1 of such a table, as the gradient pair they become
TCNN_DEVICE h2 wide_pair(const unsigned char* lds_raw, uint32_t e2, const OwnerScale& sc) {
	const long long q0 = ((const long long*)lds_raw)[2 * e2], q1 = ((const long long*)lds_raw)[2 * e2 + 1];
	return h2{from_fixed64(q0, sc), from_fixed64(q1, sc)};
}
// one gradient pair leaves its slice: a plain store for a sole owner, a packed atomic where sample chunks share the slice (small tables
// only: (table size) x (chunks) updates per level)
TCNN_DEVICE void store_pair(half_t* __restrict__ grad, uint32_t e2, h2 v, uint32_t n_chunks, bool accumulate) {
	if (n_chunks == 1) {
		if (accumulate) v += *(const h2*)(grad + 2 * e2);
		*(h2*)(grad + 2 * e2) = v;
	} else if (v[0] != (half_t)0.0f || v[1] != (half_t)0.0f) {
		atomic_add_h2(grad + 2 * e2, v);
	}
}

// What every owner of a (bucket, chunk) does last.  Every thread read the counters before the barriers of the caller: they end
// the call zeroed.  The last owner to get here (all owners have read the overflow count by then) resets the two bookkeeping
// counters -- after draining a long overflow list with the reference's global atomics.
template <uint32_t F, uint32_t THREADS>
TCNN_DEVICE void bucket_owner_epilogue(const GridMeta& meta, const OwnerSlice& own, uint32_t queue, const OwnerOverflow& over, uint32_t* __restrict__ counters,
                                       const uint32_t* __restrict__ overflow, half_t* __restrict__ grid_gradient) {
	constexpr uint32_t PW = BucketRecord<F>::PAYLOAD_WORDS, OW = BucketRecord<F>::WORDS + 1;
	__shared__ uint32_t last_owner;
	__syncthreads();  // this slice's stores are issued
	if (threadIdx.x == 0) {
		counters[own.counter_base + queue] = 0u;
		if (!over.inline_scan) {  // the drain's atomics execute memory-side: the slices must be there first (release, agent scope)
#if !defined(TCNN_HOST_EMU)
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
		}
		last_owner = atomic_add_u32(&counters[own.overflow_counter + 1], 1u) == own.n_owner_blocks - 1u ? 1u : 0u;
	}
	__syncthreads();
	if (last_owner) {
		if (!over.inline_scan) {
#if !defined(TCNN_HOST_EMU)
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
			for (uint32_t t = threadIdx.x; t < over.n; t += THREADS) {
				const uint32_t* rec = overflow + (size_t)t * OW;
				half_t* __restrict__ g = grid_gradient + (size_t)meta.offset[rec[0]] * F;
				const uint32_t index = rec[1];
				if constexpr (F == 1) {
					const half_t v = (half_t)__builtin_bit_cast(float, rec[2]);
					atomic_add_h2(g + (index & ~1u), (index & 1u) ? h2{(half_t)0.0f, v} : h2{v, (half_t)0.0f});
				} else {
#pragma unroll
					for (uint32_t p = 0; p < PW; ++p) atomic_add_h2(g + (size_t)index * F + 2 * p, bits_h2(rec[2 + p]));
				}
			}
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			counters[own.overflow_counter] = 0u;
			counters[own.overflow_counter + 1] = 0u;
		}
		if constexpr (HALF_IS_BF16) {  // (every owner read its level's sum before it signed off)
			for (uint32_t t = threadIdx.x; t < 2u * LEVEL_SUM_PARTS * own.n_levels; t += THREADS) counters[own.level_sum_base + t] = 0u;
		}
	}
}

// pass B: the owner of (bucket, chunk) streams its queue into a 64-bit fixed-point LDS table
template <uint32_t D, uint32_t F>
TCNN_DEVICE void bucket_level(const GridMeta& meta, const Level<D>& lv, uint32_t level, uint32_t bucket, uint32_t chunk, const OwnerSlice& own,
                              uint32_t* __restrict__ counters, const uint32_t* __restrict__ queues, const uint32_t* __restrict__ overflow,
                              half_t* __restrict__ grid_gradient, bool accumulate, unsigned char* lds_raw) {
	constexpr uint32_t PW = BucketRecord<F>::PAYLOAD_WORDS, PWP = BucketRecord<F>::PAIR_WORDS;
	const OwnerOverflow over = owner_overflow(own, counters);
	const uint32_t entries_per_bucket = 1u << own.shift;
	const uint32_t slice_begin = bucket * entries_per_bucket;
	const uint32_t slice_count = slice_extent(slice_begin, entries_per_bucket, lv.hashmap_size);
	unsigned long long* tab = (unsigned long long*)lds_raw;  // [entries][F]
	const OwnerScale sc = owner_scale(own, counters);
	const uint32_t queue = owner_queue(own, bucket, chunk);
	const uint32_t count = min(counters[own.counter_base + queue], own.capacity);  // in flight while the table is cleared
	const uint32_t* __restrict__ q = owner_queue_records<F>(own, queues, queue);  // `count` PAIRS of records
	for (uint32_t e = threadIdx.x; e < slice_count * F / 2; e += SLICED_THREADS) ((u4*)lds_raw)[e] = u4{0u, 0u, 0u, 0u};  // slice_count * F is even
	__syncthreads();

	auto add_record = [&](uint32_t index, const uint32_t* payload) { add_record_wide<F>(tab, index & (entries_per_bucket - 1u), payload, sc); };
	{
		// U pair records (12 bytes each for F == 2) in flight per lane: the queue is streamed at memory speed, not at one
		// round trip per record
		constexpr uint32_t U = PWP <= 3 ? 8 : (PWP <= 5 ? 4 : 2);
		for (uint32_t base = threadIdx.x; base < count; base += SLICED_THREADS * U) {
			uint32_t rec[U][PWP];
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) {
				const uint32_t t = min(base + u * SLICED_THREADS, count - 1u);
#pragma unroll
				for (uint32_t w = 0; w < PWP; ++w) rec[u][w] = queue_load(q + (size_t)t * PWP + w);
			}
#pragma unroll
			for (uint32_t u = 0; u < U; ++u) {
				if (base + u * SLICED_THREADS >= count) continue;
				add_record(rec[u][0] & PAIR_INDEX_MASK, &rec[u][1]);
				if (rec[u][0] & PAIR_HAS_SECOND) add_record(pair_second_index<D>(lv, rec[u][0]), &rec[u][1 + PW]);
			}
		}
	}
	scan_overflow<F, SLICED_THREADS>(own, over, overflow, level, bucket, chunk, add_record);
	__syncthreads();

	half_t* __restrict__ grad = grid_gradient + ((size_t)own.table_offset + slice_begin) * F;
	const uint32_t n_halves = slice_count * F;  // a multiple of 8: level sizes are multiples of 8
	for (uint32_t e2 = threadIdx.x; e2 < n_halves / 2; e2 += SLICED_THREADS) store_pair(grad, e2, wide_pair(lds_raw, e2, sc), own.n_chunks, accumulate);
	bucket_owner_epilogue<F, SLICED_THREADS>(meta, own, queue, over, counters, overflow, grid_gradient);
}

}  // namespace tcnn_hip

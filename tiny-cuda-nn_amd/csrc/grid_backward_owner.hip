// grid_backward_owner.hip -- pass B of the bucketed backward, packed form: k_grid_bucket_owner, its launcher and the owner switches.
#include "grid_backward_owner.h"
#include "exp_diag.h"  // experiment switches: compile-time zeros in the product build

namespace tcnn_hip {

// ---------------------------------------------------------------------------------------------
// pass B, packed form (even F; what the bucketed backward runs unless grid_owner_mode() == 1).
//
// The form above spends one ds_add_u64 per VALUE (two per table entry at F = 2) and 16 bytes of LDS per entry, so a
// 8192-entry slice takes 128 KiB: one workgroup per CU, whose clear / stream / convert phases cannot overlap anything.
// Here the two features of a payload word share ONE 64-bit LDS word: the addend is the two's-complement number
// V1 * 2^32 + V0 (V = value * 2^24, an exact int32 while |value| < 128), so a single ds_add_u64 accumulates both, and the
// sums come apart again as S0 = sign-extended low word, S1 = (X - S0) >> 32 -- provided both lie inside int32.  They do
// whenever the absolute values of all addends of the slice sum to less than 2^31 per feature (= 128.0 in gradient
// units; the sum over a whole LEVEL is sum_i |dL/dy_i| -- about loss_scale * mean error -- and a slice sees 1/64 of
// it): every lane keeps that running bound in fp32, the workgroup adds the lanes up once, and a slice that fails the
// test (huge or non-finite gradients) is simply redone with the 64-bit-per-value table above, in sub-slices that fit the
// same LDS.  Same exact sums, same single rounding, bit-identical output either way; half the LDS atomics, half the LDS
// (64 KiB: two workgroups share a CU, one streaming while the other clears or converts), no fp64 arithmetic.
// ---------------------------------------------------------------------------------------------
#ifndef TCNN_OWNER_THREADS
#define TCNN_OWNER_THREADS 512
#endif
constexpr uint32_t OWNER_THREADS = TCNN_OWNER_THREADS;

#if defined(TCNN_HOST_EMU)
inline unsigned long owner_slice_stats[2] = {0, 0};  // emulator only: slices finished from the packed table / redone wide
#else
// slices the packed owner kernel had to redo with 64 bits per value since the process started (grid_owner_wide_slices()): the redo
// costs that slice twice the time, so a workload whose gradients keep failing the int32 bound should be visible
__device__ unsigned long long g_owner_wide_slices = 0ull;
#endif

// round(v * 2^k) (OwnerScale; IEEE half: k = 24, |v| < 128); saturates beyond (such a slice fails the bound and is redone in 64 bits).  A
// 16-bit float times 2^24 is an integer already when the type is IEEE half (11 significant bits, exponent >= -24): the conversion
// instruction alone (v_cvt_i32_f32 saturates and maps NaN to 0 -- written as asm because the C++ conversion is undefined out of range).
// The instruction drops the fraction (towards zero): what it is given is an integer already, by the type (IEEE half) or by the rintf.
// The host emulator runs the same two steps with the instruction restated in C++.
TCNN_DEVICE int to_fixed32(float v, const OwnerScale& sc) {
	float s = sc.up(v);
	if constexpr (HALF_IS_BF16) s = __builtin_rintf(s);  // bfloat16 records reach below 2^-k
#if defined(TCNN_HOST_EMU)
	if (s != s) return 0;
	if (s >= 2147483648.0f) return 2147483647;
	if (s <= -2147483648.0f) return -2147483647 - 1;
	return (int)s;
#else
	int r;
	asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(s));
	return r;
#endif
}
// IEEE half, packed table: both values of a payload word times 2^24 as fp32 -- v_fma_mix_f32 converts the 16-bit source and multiplies in
// ONE instruction (v_cvt_f32_f16 + v_mul_f32 before; exact either way: a power of two times at most 11 significant bits.  The fused add of
// +0 turns a product of -0 into +0, which neither the integer conversion nor the bound's absolute value can tell apart).
TCNN_DEVICE void half_pair_times_2_24(uint32_t word, float& s0, float& s1) {
#if defined(TCNN_HOST_EMU) || defined(TCNN_BF16)
	const h2 v = bits_h2(word);
	s0 = (float)v[0] * 16777216.0f;
	s1 = (float)v[1] * 16777216.0f;
#else
	const float two_24 = 16777216.0f;
	asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(s0) : "v"(word), "v"(two_24));
	asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(s1) : "v"(word), "v"(two_24));
#endif
}
// total += |s|: the absolute value as a source modifier of the add (the compiler clears the sign bits of a pair with two v_and_b32 to feed
// one packed add: three instructions for what two do)
TCNN_DEVICE void add_abs(float& total, float s) {
#if defined(TCNN_HOST_EMU)
	total += __builtin_fabsf(s);
#else
	asm("v_add_f32_e64 %0, %0, |%1|" : "+v"(total) : "v"(s));
#endif
}
// the truncating, saturating conversion of to_fixed32() alone, for a value that is an integer already
TCNN_DEVICE int fixed32_of_scaled(float s) {
#if defined(TCNN_HOST_EMU)
	if (s != s) return 0;
	if (s >= 2147483648.0f) return 2147483647;
	if (s <= -2147483648.0f) return -2147483647 - 1;
	return (int)s;
#else
	int r;
	asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(s));
	return r;
#endif
}
template <uint32_t D, uint32_t F, uint32_t THREADS>
TCNN_DEVICE void bucket_level_packed(const GridMeta& meta, const Level<D>& lv, uint32_t level, uint32_t bucket, uint32_t chunk,
                                     const OwnerSlice& own, uint32_t* __restrict__ counters, const uint32_t* queues,
                                     const uint32_t* __restrict__ overflow, half_t* __restrict__ grid_gradient, bool accumulate, unsigned char* lds_raw,
                                     uint32_t lds_bytes, bool force_wide) {
	static_assert(F % 2 == 0, "the packed owner pairs the features of a payload word");
	constexpr uint32_t PW = BucketRecord<F>::PAYLOAD_WORDS, PWP = BucketRecord<F>::PAIR_WORDS;
	constexpr uint32_t N_WAVES = THREADS / WAVE;
	__shared__ float bound_parts[N_WAVES][F];
	const uint32_t entries_per_bucket = 1u << own.shift;
	const uint32_t slice_begin = bucket * entries_per_bucket;
	const uint32_t slice_count = slice_extent(slice_begin, entries_per_bucket, lv.hashmap_size);
	const uint32_t cap = own.capacity, n_chunks = own.n_chunks;
	const uint32_t queue = owner_queue(own, bucket, chunk);
	// (not __restrict__, and neither is `queues`: loads the compiler may treat as invariant are moved wherever it likes -- it sank
	// the first round below the barrier, next to its use)
	const uint32_t* q = owner_queue_records<F>(own, queues, queue);  // `count` PAIRS of records
	half_t* __restrict__ grad = grid_gradient + ((size_t)own.table_offset + slice_begin) * F;

	// U pair records (12 bytes each for F == 2) in flight per lane.  The FIRST round is requested right here, before the queue's
	// length is known (a queue holds `cap` records of memory whatever its count; what lies beyond the count is never used): it
	// travels together with the counters and while the table is cleared, instead of one more memory round trip after them -- a
	// 196 KiB queue is only four rounds per lane, and a workgroup with nothing in flight is a workgroup not streaming
	// (profiles/r03_exp_notes.txt: the pass moved its 201 MB at 4.3 TB/s with everything but the loads compiled out).
	constexpr uint32_t STREAM_U = PWP <= 3 ? 8 : (PWP <= 5 ? 4 : 2);
	auto load_round = [&](uint32_t base, uint32_t last, uint32_t (&rec)[STREAM_U][PWP]) {
#pragma unroll
		for (uint32_t u = 0; u < STREAM_U; ++u) {
			const uint32_t t = min(base + u * THREADS, last);
#pragma unroll
			for (uint32_t w = 0; w < PWP; ++w) rec[u][w] = queue_load(q + (size_t)t * PWP + w);
		}
	};
	const OwnerOverflow over = owner_overflow(own, counters);
	const uint32_t count = min(counters[own.counter_base + queue], cap);  // in flight while the table is cleared
	constexpr uint32_t diag_owner = EXP_DIAG_OWNER;  // 0 in the product build (exp_diag.h)
	const OwnerScale sc = owner_scale(own, counters);
	bool safe = !force_wide;
	// the packed table is cleared first (LDS only), the first round requested behind it: nothing then stands between the loads and
	// their use but the barrier (cleared after the loads, the compiler parks part of a record in other registers and waits for it)
	// (both happen at the top of the `if (safe)` block below -- ONE block from the issue of the hand-made loads to their last use, so that no
	// control-flow path of the compiled code leads from an issued load to anything but its wait: scripts/check_asm_load_hazard.py checks that)
	// Three-word records (F <= 2) on the GPU: the stream is PIPELINED BY HAND, two half-rounds of STREAM_U / 2 records per lane that are
	// consumed and re-requested in turn -- while the records of one half go through the conversions and LDS atomics (45 VALU
	// instructions each; the four waves of a SIMD all want the ALU when their loads arrive), the other half's loads are on their
	// way.  Written in C++ the compiler rotates the record registers (copies at the loop's back edge) and waits for the loads it
	// has just issued before it copies them (tried twice, profiles/r03_exp_notes.txt 10b, r04_exp_notes.txt): hence loads the
	// compiler does not see (asm), into registers that keep their identity, with counted waits.  vmcnt counts in issue order, so
	// "at most 4 outstanding" means the OLDER half has landed whatever the compiler's own loads do around it.
#if !defined(TCNN_HOST_EMU) && !defined(TCNN_OWNER_PLAIN_STREAM)
	constexpr bool PIPELINED = PWP == 3 && STREAM_U == 8;
#else
	constexpr bool PIPELINED = false;
#endif
	typedef uint32_t rec3_t __attribute__((ext_vector_type(3)));
#ifndef TCNN_OWNER_GROUPS
#define TCNN_OWNER_GROUPS 2
#endif
	constexpr uint32_t NG = TCNN_OWNER_GROUPS;  // groups of 4 records in flight per lane (3 / 4 / 6 / 8 groups measured 0.0524 / 0.0538 / 0.0574 / 0.0710 ms against 0.0510: profiles/r04_exp_notes.txt 14d)
	rec3_t grp[NG][4];
	uint32_t first_round[PIPELINED ? 1 : STREAM_U][PWP];
#if !defined(TCNN_HOST_EMU)
	const uint64_t q_address = (uint64_t)(uintptr_t)q;  // wave-uniform: into a scalar register pair, the loads' base
	// (readfirstlane returns a signed int: without the casts the low word is sign-extended over the high one)
	const uint64_t q_scalar = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(q_address >> 32)) << 32) |
	                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)q_address);
	auto issue_half = [&](rec3_t (&h)[4], uint32_t first, uint32_t last) {
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u) {
			const uint32_t byte_offset = __umul24(min(first + u * THREADS, last), 12u);  // record index < 2^24: a queue holds < 2^31 records of < 2^32 bytes, see the check below
			asm volatile("global_load_dwordx3 %0, %1, %2 nt" : "=v"(h[u]) : "v"(byte_offset), "s"(q_scalar) : "memory");
		}
	};
	// (all NG groups outstanding: "at most 4 (NG - 1) loads outstanding" means the oldest group has landed)
	auto await_oldest_group = [&](rec3_t (&h)[4]) {
		asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]) : [n] "n"(4 * (NG - 1)) : "memory");
	};
#endif
	// streams the queue (and this slice's share of the overflow list) through `add(index, payload)`; `first`: the lane's first
	// round if it is in registers already (the first pass over the queue), null to load it here (the 64-bit redo)
	auto stream = [&](const uint32_t (*first)[PWP], auto&& add) {
		constexpr uint32_t U = STREAM_U;
		auto add_round = [&](uint32_t base, const uint32_t (&rec)[U][PWP]) {
			if (base + (U - 1) * THREADS < count) {  // all U records exist (every round but a lane's last): no per-record test
#pragma unroll
				for (uint32_t u = 0; u < U; ++u) {
					add(rec[u][0] & PAIR_INDEX_MASK, &rec[u][1]);
					if (rec[u][0] & PAIR_HAS_SECOND) add(pair_second_index<D>(lv, rec[u][0]), &rec[u][1 + PW]);
				}
			} else {
#pragma unroll
				for (uint32_t u = 0; u < U; ++u) {
					if (base + u * THREADS >= count) continue;
					add(rec[u][0] & PAIR_INDEX_MASK, &rec[u][1]);
					if (rec[u][0] & PAIR_HAS_SECOND) add(pair_second_index<D>(lv, rec[u][0]), &rec[u][1 + PW]);
				}
			}
		};
		uint32_t base = threadIdx.x;
		if (first) {
			if (base < count) add_round(base, *(const uint32_t (*)[U][PWP])first);
			base += THREADS * U;
		}
		for (; base < count; base += THREADS * U) {
			uint32_t rec[U][PWP];
			load_round(base, count - 1u, rec);
			add_round(base, rec);
		}
		scan_overflow<F, THREADS>(own, over, overflow, level, bucket, chunk, add);
	};
	// the same through the hand-pipelined halves (first pass over the queue only; its first two halves were requested above)
	auto stream_pipelined = [&](auto&& add) {
#if !defined(TCNN_HOST_EMU)
		// WHOLE: every record of the round exists (all rounds but a lane's last, by the loop's own condition): no test against the count
		// per record.  (The loop stays ONE copy: instantiated per table kind behind a branch, so that the second entry's index needs no
		// scalar branch per record, the compiler copied registers of loads still in flight on the way into the copies --
		// scripts/check_asm_load_hazard.py flagged it, and the GPU gave wrong sums.)
		auto add_half = [&](auto whole_tag, uint32_t first, const rec3_t (&h)[4]) {
			constexpr bool WHOLE = decltype(whole_tag)::value;
#pragma unroll
			for (uint32_t u = 0; u < 4; ++u) {
				if (!WHOLE && first + u * THREADS >= count) continue;
				const uint32_t rec[3] = {h[u][0], h[u][1], h[u][2]};
				add(rec[0] & PAIR_INDEX_MASK, &rec[1]);
				if (rec[0] & PAIR_HAS_SECOND) add(pair_second_index<D>(lv, rec[0]), &rec[1 + PW]);
			}
		};
		const uint32_t last = count ? count - 1u : 0u;
		// every round but the last re-requests its groups (workgroup-uniform trip count: every wave issues the same loads); the last
		// one only drains -- a request beyond the queue's end is a load instruction and a round trip the lane then has to wait out
		uint32_t round = 0;
		for (; round + 4u * NG * THREADS < count; round += 4u * NG * THREADS) {
			const uint32_t first = round + threadIdx.x;
#pragma unroll
			for (uint32_t k = 0; k < NG; ++k) {
				await_oldest_group(grp[k]);
				add_half(std::true_type{}, first + 4u * k * THREADS, grp[k]);
				issue_half(grp[k], first + 4u * (NG + k) * THREADS, last);
			}
		}
		// nothing of this lane's may still be on its way into registers the compiler is about to reuse
#pragma unroll
		for (uint32_t k = 0; k < NG; ++k) {
			asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(grp[k][0]), "+v"(grp[k][1]), "+v"(grp[k][2]), "+v"(grp[k][3]) : [n] "n"(4 * (NG - 1 - k)) : "memory");
			if (round < count) add_half(std::false_type{}, round + threadIdx.x + 4u * k * THREADS, grp[k]);
		}
#endif
		scan_overflow<F, THREADS>(own, over, overflow, level, bucket, chunk, add);
	};

	if (safe) {
		if (!(diag_owner & 1u)) {
			for (uint32_t e = threadIdx.x; e < slice_count * PW / 2; e += THREADS) ((u4*)lds_raw)[e] = u4{0u, 0u, 0u, 0u};  // slice_count is a multiple of 8
		}
		if constexpr (PIPELINED) {
#if !defined(TCNN_HOST_EMU)
			// (only the packed pass consumes them -- and nothing the compiler does not know of may stay in flight otherwise)
#pragma unroll
			for (uint32_t k = 0; k < NG; ++k) issue_half(grp[k], threadIdx.x + 4u * k * THREADS, cap - 1u);
#endif
		} else {
			load_round(threadIdx.x, cap - 1u, first_round);
		}
		unsigned long long* tab = (unsigned long long*)lds_raw;  // [entries][PW]: features 2p (low word) and 2p + 1 (high word)
		__syncthreads();  // the table is clear
		float bound[F];
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) bound[f] = 0.0f;
		constexpr float BOUND_UNITS = HALF_IS_BF16 ? 1.0f : 16777216.0f;  // what `bound` counts in: gradient units, or 2^-24 of them (IEEE half, below)
		auto add_packed = [&](uint32_t index, const uint32_t* payload) {
			const uint32_t rel = index & (entries_per_bucket - 1u);
#pragma unroll
			for (uint32_t p = 0; p < PW; ++p) {
				int v0, v1;
				if constexpr (HALF_IS_BF16) {
					const h2 v = bits_h2(payload[p]);
					const float f0 = (float)v[0], f1 = (float)v[1];
					bound[2 * p] += __builtin_fabsf(f0);
					bound[2 * p + 1] += __builtin_fabsf(f1);
					v0 = to_fixed32(f0, sc);
					v1 = to_fixed32(f1, sc);
				} else {
					// IEEE half: the bound is kept in the table's own units, sum |v * 2^24| -- the same sum times a power of two, rounded in the
					// same places -- so that one scaled value serves the bound and the conversion (BOUND_UNITS at the test below)
					float s0, s1;
					half_pair_times_2_24(payload[p], s0, s1);
					add_abs(bound[2 * p], s0);
					add_abs(bound[2 * p + 1], s1);
					v0 = fixed32_of_scaled(s0);
					v1 = fixed32_of_scaled(s1);
				}
				const unsigned long long x = ((unsigned long long)(uint32_t)(v1 + (v0 >> 31)) << 32) | (unsigned long long)(uint32_t)v0;
				if (!(diag_owner & 2u) || x == 0x123456789ull) lds_atomic_add_u64(&tab[rel * PW + p], x);
			}
		};
		if constexpr (PIPELINED) stream_pipelined(add_packed);
		else stream(first_round, add_packed);
		// the bound over the whole workgroup (NaN / Inf anywhere fail the comparison)
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) {
			const float w = wave_sum_f32(bound[f]);
			if (lane_id() == 0) bound_parts[threadIdx.x / WAVE][f] = w;
		}
		__syncthreads();  // also: every atomic of the slice has landed
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) {
			float total = 0.0f;
#pragma unroll
			for (uint32_t w = 0; w < N_WAVES; ++w) total += bound_parts[w][f];
			safe = safe && total < sc.safe_abs_sum() * BOUND_UNITS;
		}
		if (safe && !(diag_owner & 4u)) {
			auto unpack = [&](uint32_t e2) {
				const long long x = (long long)tab[e2];
				const int s0 = (int)(uint32_t)(unsigned long long)x;
				const int s1 = (int)((x - (long long)s0) >> 32);
				// int32 -> fp32 rounds to nearest even exactly as the fp64 -> fp32 conversion of the wide form does
				return h2{(half_t)sc.down((float)s0), (half_t)sc.down((float)s1)};
			};
			if (n_chunks == 1 && !accumulate && ((uintptr_t)grad & 15u) == 0u) {  // sole owner, overwrite: 16 bytes per lane (slice_count * PW is a multiple of 8)
				for (uint32_t e8 = threadIdx.x; e8 < slice_count * PW / 4; e8 += THREADS) {
					const h2 a = unpack(4 * e8), b = unpack(4 * e8 + 1), c = unpack(4 * e8 + 2), d = unpack(4 * e8 + 3);
					*(h8*)(grad + 8 * e8) = h8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
				}
			} else {
				for (uint32_t e2 = threadIdx.x; e2 < slice_count * PW; e2 += THREADS) store_pair(grad, e2, unpack(e2), n_chunks, accumulate);
			}
		}
	}
#if defined(TCNN_HOST_EMU)
	if (threadIdx.x == 0) owner_slice_stats[safe ? 0 : 1]++;
#else
	if (!safe && !force_wide && threadIdx.x == 0) atomicAdd(&g_owner_wide_slices, 1ull);
#endif
	if (!safe) {
		// 64 bits per value, `sub` entries at a time (the same LDS): each pass streams the queue again and keeps its own entries
		unsigned long long* tab = (unsigned long long*)lds_raw;  // [sub][F]
		const uint32_t sub = max(8u, (lds_bytes / (F * 8u)) & ~7u);
		for (uint32_t sub_begin = 0; sub_begin < slice_count; sub_begin += sub) {
			const uint32_t sub_count = min(sub, slice_count - sub_begin);
			__syncthreads();  // the table is free (bound test / previous pass's conversion)
			for (uint32_t e = threadIdx.x; e < sub_count * F / 2; e += THREADS) ((u4*)lds_raw)[e] = u4{0u, 0u, 0u, 0u};
			__syncthreads();
			stream(nullptr, [&](uint32_t index, const uint32_t* payload) {
				const uint32_t rel = (index & (entries_per_bucket - 1u)) - sub_begin;
				if (rel < sub_count) add_record_wide<F>(tab, rel, payload, sc);
			});
			__syncthreads();
			for (uint32_t e2 = threadIdx.x; e2 < sub_count * PW; e2 += THREADS) store_pair(grad, sub_begin * PW + e2, wide_pair(lds_raw, e2, sc), n_chunks, accumulate);
		}
	}
	if (diag_owner & 8u) {  // (racy on purpose: the list counter is reset by whoever gets here)
		if (threadIdx.x == 0) {
			counters[own.counter_base + queue] = 0u;
			counters[own.overflow_counter] = 0u;
		}
		return;
	}
	bucket_owner_epilogue<F, THREADS>(meta, own, queue, over, counters, overflow, grid_gradient);
}

// The workgroups of pass B that own a (bucket, chunk), packed form.  Launched as a 2-D grid -- blockIdx.y = the plan's item, blockIdx.x = the
// workgroup within it -- with everything a workgroup needs to know about its item in ONE descriptor in the kernel arguments: a single
// scalar load round before the queue's first records are requested.  (Round 5 looked the item up through the sliced kernel's plan: blocks per
// item -> block_begin[item] -> kind[item] -> level[item] -> n_slices[item] -> the level's table size -> the slot's queue geometry, six
// dependent loads, 1.6 us of a workgroup's 18.7 by the clock stamps of round 4 -- twice per launch, there are two generations of owners.)
// k_grid_backward_sliced (the other kinds of items, if the plan holds any) skips the bucket items when this kernel runs them.
struct OwnerItem {
	uint32_t level, slot, n_slices, n_blocks;      // n_blocks = n_slices x n_chunks workgroups belong to the item
	uint32_t hashmap_size, fast, offset, capacity;  // the level's table: entries, hashed power-of-two table?, first entry; pairs per queue
	uint32_t n_chunks, n_buckets, counter_base, pad;
	uint64_t queue_base;
};
struct OwnerItems {
	OwnerItem item[MAX_BUCKET_LEVELS];
};
template <uint32_t D, uint32_t F>
__global__ void __launch_bounds__(OWNER_THREADS) k_grid_bucket_owner(const GridMeta meta, const OwnerItems items, const int accumulate, const uint32_t shift,
                                                                      const uint32_t overflow_counter, const uint32_t overflow_capacity, const uint32_t n_owner_blocks,
                                                                      const uint32_t level_sum_base, const uint32_t n_bucket_levels, uint32_t* __restrict__ counters,
                                                                      const uint32_t* queues, const uint32_t* __restrict__ overflow, half_t* __restrict__ grid_gradient,
                                                                      const uint32_t lds_bytes, const int force_wide) {
	TCNN_DYN_LDS(lds_raw);
	const OwnerItem it = items.item[blockIdx.y];
	const uint32_t local_block = blockIdx.x;
	if (local_block >= it.n_blocks) return;
	const uint32_t slice = local_block % it.n_slices, chunk = local_block / it.n_slices;
	Level<D> lv = {};  // (what the owner reads of it: the table's size and kind -- pair_second_index, the slice's extent)
	lv.hashmap_size = it.hashmap_size;
	lv.mask = it.hashmap_size - 1u;
	lv.fast = it.fast != 0u;
	const OwnerSlice own = {it.capacity, it.n_chunks, it.n_buckets, it.counter_base, it.queue_base, it.offset, it.slot,
	                        shift, overflow_counter, overflow_capacity, n_owner_blocks, level_sum_base, n_bucket_levels};
	if constexpr (F % 2 == 0) {  // (never launched for odd F)
		bucket_level_packed<D, F, OWNER_THREADS>(meta, lv, it.level, slice, chunk, own, counters, queues, overflow, grid_gradient, accumulate != 0, lds_raw, lds_bytes,
		                                         force_wide != 0);
	}
}

void launch_bucket_owners(hipStream_t stream, const GridMeta& meta, const BackwardPlan& bp, bool accumulate, bool force_wide, uint32_t* counters,
                          const uint32_t* queues, const uint32_t* overflow, half_t* grid_gradient) {
	const SlicePlan& plan = bp.slices;
	const BucketPlan& bk = bp.buckets;
	const uint32_t lds = std::max((1u << bk.shift) * meta.n_feat * 4u, 8u * meta.n_feat * 8u);
	// one descriptor per bucket item, in plan order; the grid is (workgroups of the largest item) x (items)
	OwnerItems items = {};
	uint32_t n_items = 0, width = 0;
	for (uint32_t p = 0; p < plan.n_items; ++p) {
		if (plan.kind[p] != SLICE_BUCKET) continue;
		const uint32_t l = plan.level[p], j = plan.slot[p];
		const LevelGeometry geo = level_geometry(meta, l);
		OwnerItem& it = items.item[n_items++];
		it.level = l;
		it.slot = j;
		it.n_slices = plan.n_slices[p];
		it.n_blocks = plan.block_begin[p + 1] - plan.block_begin[p];
		it.hashmap_size = geo.entries;
		it.fast = geo.fast ? 1u : 0u;
		it.offset = meta.offset[l];
		it.capacity = bk.capacity[j];
		it.n_chunks = bk.n_chunks[j];
		it.n_buckets = bk.n_buckets[j];
		it.counter_base = bk.counter_base[j];
		it.queue_base = bk.queue_base[j];
		width = std::max(width, it.n_blocks);
	}
	grid_dispatch(meta, [&](auto D, auto F) {
		if constexpr (F % 2 == 0) {  // (the packed owner pairs the features: no instances for odd F)
			TCNN_SET_MAX_DYN_LDS((k_grid_bucket_owner<D, F>), lds);
			TCNN_LAUNCH((k_grid_bucket_owner<D, F>), dim3(width, n_items), dim3(OWNER_THREADS), lds, stream, meta, items, accumulate ? 1 : 0, bk.shift, bk.overflow_counter,
			            bk.overflow_capacity, bk.n_owner_blocks, bk.level_sum_base, bk.n_levels, counters, queues, overflow, grid_gradient, lds, force_wide ? 1 : 0);
		}
	});
}

unsigned long long grid_owner_wide_slices() {
#if defined(TCNN_HOST_EMU)
	return owner_slice_stats[1];
#else
	unsigned long long v = 0;
	if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_owner_wide_slices), sizeof(v)) != hipSuccess) throw std::runtime_error("grid_owner_wide_slices: could not read the counter");
	return v;
#endif
}

int& grid_owner_mode() {
	static int mode = 0;
	return mode;
}

}  // namespace tcnn_hip

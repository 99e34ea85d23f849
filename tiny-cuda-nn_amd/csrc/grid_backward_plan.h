// grid_backward_plan.h -- what the passes of the sliced / bucketed backward agree on: the work lists the host plans (SlicePlan, BucketPlan),
// the queue record and its pair encoding, the owners' fixed-point exponent and the level sums it is chosen from, and the host planner.
#pragma once
#include "grid_device.h"

#include <algorithm>
#include <vector>

namespace tcnn_hip {

#ifndef TCNN_SLICED_THREADS
#define TCNN_SLICED_THREADS 1024
#endif
constexpr uint32_t SLICED_THREADS = TCNN_SLICED_THREADS;
constexpr uint32_t SLICED_LDS_BYTES = 128 * 1024;      // default slice size
constexpr uint32_t SLICED_LDS_MAX_BYTES = 160 * 1024;  // one CU's LDS
constexpr double FIXED_SCALE = 16777216.0;             // 2^24: below the smallest fp16 subnormal

enum SliceKind : uint32_t { SLICE_FIXED64 = 0, SLICE_FLOAT = 1, SLICE_GLOBAL_ATOMIC = 2, SLICE_BUCKET = 3 };

// Work list of one launch, in dispatch order (long slice passes first, short work fills the tail).
struct SlicePlan {
	uint32_t n_items;
	uint32_t blocks_per_item;                // launch stride (max workgroups of any item) of a near-uniform plan, else 0
	uint32_t block_begin[MAX_N_LEVELS + 1];  // first workgroup of item p
	uint32_t n_slices[MAX_N_LEVELS];         // slices (FIXED64 / FLOAT) or sample tiles (GLOBAL_ATOMIC) of item p
	uint8_t level[MAX_N_LEVELS];             // grid level of item p
	uint8_t kind[MAX_N_LEVELS];              // SliceKind of item p
	uint8_t slot[MAX_N_LEVELS];              // SLICE_BUCKET: slot of the level in the BucketPlan
};

#ifndef TCNN_BUCKET_THREADS
#define TCNN_BUCKET_THREADS 256
#endif
constexpr uint32_t BUCKET_THREADS = TCNN_BUCKET_THREADS;
constexpr uint32_t MAX_BUCKET_LEVELS = 32;
#ifndef TCNN_BUCKET_RESIDENT_WGS
#define TCNN_BUCKET_RESIDENT_WGS 2048  // measured: 2 tiles in flight per resident slot beat 1, 1.5, 4 and 8 (profiles/r01_exp_scatter_wgs.txt)
#endif
constexpr uint32_t BUCKET_RESIDENT_WGS = TCNN_BUCKET_RESIDENT_WGS;  // persistent scatter workgroups over all levels
constexpr uint32_t MAX_BUCKETS_PER_LEVEL = 4096;
// overflow records up to which every bucket owner scans the list for its own (4 MiB of L2 reads per owner at the bound)
constexpr uint32_t OVERFLOW_INLINE_MAX = 1u << 18;
#ifndef TCNN_BUCKET_STAGE_BYTES
#define TCNN_BUCKET_STAGE_BYTES (32 * 1024)  // measured: 32 KiB (4 workgroups per CU) beats 64 and 16 KiB
#endif
constexpr uint32_t BUCKET_STAGE_BYTES = TCNN_BUCKET_STAGE_BYTES;  // LDS staging area of pass A

struct BucketPlan {
	uint32_t n_levels;  // bucketed levels
	uint32_t shift;     // log2(entries per bucket)
	uint32_t tiles;     // sample tiles per level in pass A
	uint32_t wgs_per_level;      // persistent pass-A workgroups per level (each walks tiles wg, wg + wgs_per_level, ...)
	uint32_t scatter_blocks;     // n_levels * wgs_per_level: pass-A blocks beyond these zero the gradients of chunked levels
	uint32_t overflow_counter;   // index of the overflow counter (== total number of queues); the one after it counts finished pass-C blocks
	uint32_t level_sum_base;     // (even) index of slot 0's 64-bit sums (LEVEL_SUM_PARTS per level) of |dL/dy| over the batch, 2^-32 units (OwnerScale; bfloat16 build only)
	uint32_t overflow_capacity;  // records
	uint32_t n_owner_blocks;     // workgroups of pass B that own a bucket (the last one to finish resets the bookkeeping counters)
	uint32_t packed_owner;       // pass B's bucket items run in k_grid_bucket_owner (packed accumulators), not in k_grid_backward_sliced
	uint8_t level[MAX_BUCKET_LEVELS];             // grid level of slot j
	uint32_t n_buckets[MAX_BUCKET_LEVELS];        // table slices
	uint32_t n_chunks[MAX_BUCKET_LEVELS];         // sample chunks: a queue belongs to one (chunk, bucket); > 1 only for small tables
	uint32_t tiles_per_chunk[MAX_BUCKET_LEVELS];
	uint32_t capacity[MAX_BUCKET_LEVELS];         // PAIRS of records per queue
	uint32_t counter_base[MAX_BUCKET_LEVELS];     // first counter of slot j; queue (chunk, bucket) uses counter chunk * n_buckets + bucket
	uint32_t zero_block_begin[MAX_BUCKET_LEVELS + 1];  // pass-A zeroing blocks of slot j (4 KiB each; none unless chunked && !accumulate)
	uint64_t queue_base[MAX_BUCKET_LEVELS];       // first pair of slot j's queues
};
constexpr uint32_t ZERO_BLOCK_HALVES = 2048;  // 4 KiB per zeroing block

// record = {entry index within the level, payload}: payload = F halves packed in pairs (F == 1: one fp32, the
// reference's grad_t for a single feature is float, grid.h:665)
//
// Queue unit: a PAIR of records -- the two corners that differ in dimension 0 only -- in 1 + 2 * PAYLOAD_WORDS words:
//   word 0 = index of the first entry (25 bits) | t << 25 | has_second << 30, then the two payloads.
// The second entry is DERIVED: dense-indexed levels: index + 1 (wrapping at the table size); hashed levels (prime[0] == 1,
// power-of-two table): index ^ (2^(t+1) - 1), t = number of trailing one bits of the cell's x coordinate.  12 bytes per
// pair for F == 2 instead of 16: the queues are the backward pass's HBM traffic.
TCNN_HOST_DEVICE constexpr uint32_t record_words(uint32_t F) { return 1 + (F + 1) / 2; }     // overflow-list record: one entry
TCNN_HOST_DEVICE constexpr uint32_t pair_words(uint32_t F) { return 1 + 2 * ((F + 1) / 2); }  // queue record: two entries
template <uint32_t F>
struct BucketRecord {
	static constexpr uint32_t PAYLOAD_WORDS = (F + 1) / 2, WORDS = record_words(F), PAIR_WORDS = pair_words(F);
};
constexpr uint32_t PAIR_INDEX_BITS = 25, PAIR_INDEX_MASK = (1u << PAIR_INDEX_BITS) - 1u, PAIR_HAS_SECOND = 1u << 30;
template <uint32_t D>
TCNN_DEVICE uint32_t pair_second_index(const Level<D>& lv, uint32_t word0) {
	const uint32_t i0 = word0 & PAIR_INDEX_MASK;
	if (lv.fast) return (i0 ^ ((2u << ((word0 >> PAIR_INDEX_BITS) & 31u)) - 1u)) & lv.mask;
	const uint32_t i1 = i0 + 1u;
	return i1 == lv.hashmap_size ? 0u : i1;
}
// samples per thread of pass A: as many as fit the staging area, at least one
TCNN_HOST_DEVICE constexpr uint32_t bucket_spt(uint32_t D, uint32_t F) {
	const uint32_t per_sample_bytes = ((1u << D) / 2u) * pair_words(F) * 4u;
	const uint32_t spt = BUCKET_STAGE_BYTES / (per_sample_bytes * BUCKET_THREADS);
	return spt < 1u ? 1u : (spt > 8u ? 8u : spt);
}

// The queues are written once and read once: stream them past the caches (non-temporal) so that they do not evict the
// optimizer state the step's last kernel re-reads.  TCNN_QUEUE_TEMPORAL=1 builds the plain variant for A/B runs.
#if defined(TCNN_HOST_EMU) || defined(TCNN_QUEUE_TEMPORAL)
TCNN_DEVICE void queue_store(uint32_t* p, uint32_t v) { *p = v; }
TCNN_DEVICE uint32_t queue_load(const uint32_t* p) { return *p; }
#else
TCNN_DEVICE void queue_store(uint32_t* p, uint32_t v) { __builtin_nontemporal_store(v, p); }
TCNN_DEVICE uint32_t queue_load(const uint32_t* p) { return __builtin_nontemporal_load(p); }
#endif
constexpr uint32_t BUCKET_INVALID_INDEX = 0xFFFFFFFFu;  // word 0 of a pair that does not exist / second record of a pair that has none
TCNN_DEVICE uint32_t h2_bits(h2 v) { return __builtin_bit_cast(uint32_t, v); }
TCNN_DEVICE h2 bits_h2(uint32_t v) { return __builtin_bit_cast(h2, v); }

// Fixed-point exponent of a bucket owner's accumulators (pass B): a record v is accumulated as the integer round(v * 2^k).
//   IEEE half: k = 24 for every slice -- a half times 2^24 is an integer already (11 significant bits, exponent >= -24): exact sums.
//   bfloat16 (-DTCNN_BF16): the type reaches down to 2^-133, and at a fixed 2^-24 records below 2^-25 vanished and small ones lost most of
//   their eight bits (round 5's stress-shape test had to tolerate entries that the oracle touched and the GPU left at zero).  k is chosen per
//   slice from what pass A measured: the level's sum of |dL/dy| over the batch (a 64-bit integer sum, so the same k every run) divided by
//   the level's slices, with a factor 8 of headroom over that uniform share -- k = 30 - ceil(log2(8 * share)), 20 <= k <= 40.  At the
//   stress shape: k = 31 - 34 for the hashed levels, resolution 2^-31 and finer against records of 1e-7 and up.  A slice whose records
//   exceed the headroom (clustered samples) fails the int32 bound test as before and is redone with 64 bits per value at the same k.
//   What is summed is the magnitude of what the scatter emits: |dL/dy| in the first-order pass (the corner weights of a sample add up to
//   one), |dL/dy| * sum over the corners of |weight| in the second-order pass, whose weights carry ddx * scale (each sample clamped to
//   LEVEL_SUM_CLAMP either way).  The sum is kept in 2^-32 units in 64 bits: a workgroup's total is clamped below 2^32 before it is
//   converted (level_sum_units), and a sum that would pass 2^64 -- 2^20 samples at the clamp -- SATURATES at 2^64 - 1 instead of
//   wrapping to a small value (level_sum_add, and the sum over the parts in owner_scale): such a level gets the coarsest exponent its
//   slice count allows (k = 20 for up to 2^26 slices) and never the k = 40 a wrapped sum of zero would have chosen.
//   Range (bfloat16): a record whose scaled value |v| * 2^k does not stay below 9e18 (~2^63) cannot enter a 64-bit sum and is DROPPED
//   (to_fixed64).  With k >= 20 every record below 2^42 (4.4e12) is carried; above that the gradient of the entries it touches is not
//   defined (include/tcnn_hip.h states the range, tests/test_emu_bf16.py pins the edge).
struct OwnerScale {
	int k;
	TCNN_DEVICE float up(float v) const { return HALF_IS_BF16 ? __builtin_ldexpf(v, k) : v * 16777216.0f; }
	TCNN_DEVICE float down(float v) const { return HALF_IS_BF16 ? __builtin_ldexpf(v, -k) : v * (1.0f / 16777216.0f); }
	TCNN_DEVICE float safe_abs_sum() const { return HALF_IS_BF16 ? __builtin_ldexpf(0.9375f, 31 - k) : 120.0f; }  // < 2^31 / 2^k, with room for the bound's own rounding
	TCNN_DEVICE double up64() const { return HALF_IS_BF16 ? __builtin_ldexp(1.0, k) : 16777216.0; }
	TCNN_DEVICE double down64() const { return HALF_IS_BF16 ? __builtin_ldexp(1.0, -k) : 1.0 / 16777216.0; }
};
constexpr uint32_t LEVEL_SUM_PARTS = 8;  // words a level's sum is spread over (the scatter's workgroups add into word blockIdx % 8)
constexpr float LEVEL_SUM_CLAMP = 4096.0f;  // per sample: 2^18 .. 2^20 samples of it stay inside 64 bits at 2^-32 units
// a workgroup's fp32 total -> 2^-32 units: clamped below 2^32 first (the conversion of a larger value is undefined), nothing for
// zero, negative values and NaN
TCNN_HOST_DEVICE unsigned long long level_sum_units(float total) {
	if (!(total > 0.0f)) return 0ull;
	return (unsigned long long)((double)__builtin_fminf(total, 4294967040.0f) * 4294967296.0);  // (the largest fp32 below 2^32)
}
TCNN_HOST_DEVICE unsigned long long saturating_add_u64(unsigned long long a, unsigned long long b) {
	const unsigned long long s = a + b;
	return s < a ? ~0ull : s;
}
// adds into one of a level's sum words; sticky at 2^64 - 1: whoever sees the word wrap sets it to the maximum, and every later add wraps
// again and does the same (the owners read the word in a later launch, after the last of them)
TCNN_DEVICE void level_sum_add(unsigned long long* word, unsigned long long units) {
	if (units == 0ull) return;
#if defined(TCNN_HOST_EMU)
	*word = saturating_add_u64(*word, units);
#else
	const unsigned long long old = atomicAdd(word, units);
	if (old + units < old) atomicMax(word, ~0ull);
#endif
}

// Host-side plan of one sliced / bucketed launch sequence.
struct BackwardPlan {
	SlicePlan slices = {};
	BucketPlan buckets = {};
	uint32_t lds_slice_bytes = 0, blocks = 0;
	std::vector<uint32_t> n_chunks;  // per item
	// workspace layout (bytes from its start)
	size_t n_counters = 0, overflow_offset = 0, workspace_bytes = 0;  // queues at offset 0 of the workspace
};

inline BackwardPlan make_backward_plan(const GridMeta& meta, uint32_t n, bool packed, bool bucketed, bool accumulate, uint32_t lds_slice_bytes) {
	const uint32_t F = meta.n_feat;
	packed = packed && (F % 2 == 0);
	if (lds_slice_bytes == 0 || lds_slice_bytes > SLICED_LDS_MAX_BYTES) lds_slice_bytes = SLICED_LDS_BYTES;
	const uint32_t float_entry_bytes = F * (packed ? (uint32_t)sizeof(half_t) : (uint32_t)sizeof(float));
	const uint32_t fixed_entry_bytes = F * (uint32_t)sizeof(unsigned long long);
	lds_slice_bytes = std::max(lds_slice_bytes / fixed_entry_bytes, 8u) * fixed_entry_bytes;
	const uint32_t cap_fixed = lds_slice_bytes / fixed_entry_bytes, cap_float = lds_slice_bytes / float_entry_bytes;  // entries per slice
	uint32_t bucket_shift = 0;  // buckets hold a power-of-two number of entries (bucket = index >> shift)
	while ((2u << bucket_shift) <= cap_fixed) ++bucket_shift;
	const uint32_t n_corners = meta.interp == (uint32_t)InterpolationType::Nearest ? 1u : (1u << meta.n_dims);

	BackwardPlan bp;
	bp.lds_slice_bytes = lds_slice_bytes;
	BucketPlan& bk = bp.buckets;
	bk.shift = bucket_shift;
	bk.tiles = div_round_up(n, bucket_spt(meta.n_dims, F) * BUCKET_THREADS);
	uint32_t n_counters = 0, n_zero_blocks = 0;
	uint64_t n_queue_records = 0, n_records = 0;

	// Per level: accumulator kind by expected LDS-atomic density (see the comments above the kernels).
	struct Item {
		uint32_t level, kind, n_slices, n_chunks, slot;
	};
	std::vector<Item> items;
	for (uint32_t l = 0; l < meta.n_levels; ++l) {
		const LevelGeometry geo = level_geometry(meta, l);
		const uint32_t entries = geo.entries;
		const uint32_t n_fixed = div_round_up(entries, cap_fixed);
		const uint32_t n_buckets = div_round_up(entries, 1u << bucket_shift);
		Item it = {l, SLICE_FIXED64, n_fixed, 1u, 0u};
		if (bucketed && bk.n_levels < MAX_BUCKET_LEVELS && n_buckets <= MAX_BUCKETS_PER_LEVEL && entries <= (1u << PAIR_INDEX_BITS)) {
			// corners are derived once, binned by (table slice, sample chunk), accumulated by the queue's owner.
			// Large tables: one owner per slice (plain stores).  Small tables have few slices: the samples are also
			// split so that an owner sees ~32 Ki records; the owners of a slice then combine with packed-half atomics.
			const uint32_t j = bk.n_levels++;
			const uint64_t level_records = (uint64_t)n * n_corners;
			const uint64_t per_bucket = level_records / n_buckets;
			uint32_t n_chunks = per_bucket <= 65536 ? 1u : (uint32_t)std::min<uint64_t>(div_round_up<uint64_t>(per_bucket, 32768), bk.tiles);
			const uint32_t tiles_per_chunk = div_round_up(bk.tiles, n_chunks);
			n_chunks = div_round_up(bk.tiles, tiles_per_chunk);
			const uint64_t level_pairs = (uint64_t)n * std::max(1u, n_corners / 2u);  // queue unit: a pair of records
			const uint64_t expected = level_pairs / ((uint64_t)n_buckets * n_chunks);
			const uint64_t capacity = next_multiple<uint64_t>(2 * expected + 512, 64);
			// (queue positions are multiplied with 24-bit multiplies in the owner pass; the 2^32 records checked below come first for every
			// table with more than a few buckets, and small tables are chunked to ~32 Ki records per queue)
			if (capacity >= (1ull << 24)) throw std::runtime_error("grid_backward: batch too large for the bucketed backward");
			bk.level[j] = (uint8_t)l;
			bk.n_buckets[j] = n_buckets;
			bk.n_chunks[j] = n_chunks;
			bk.tiles_per_chunk[j] = tiles_per_chunk;
			bk.capacity[j] = (uint32_t)capacity;
			bk.counter_base[j] = n_counters;
			bk.queue_base[j] = n_queue_records;
			bk.zero_block_begin[j] = n_zero_blocks;
			if (n_chunks > 1 && !accumulate) n_zero_blocks += div_round_up(entries * F, ZERO_BLOCK_HALVES);
			n_counters += n_buckets * n_chunks;
			n_queue_records += capacity * n_buckets * n_chunks;
			n_records += level_records;
			it.kind = SLICE_BUCKET;
			it.n_slices = n_buckets;
			it.n_chunks = n_chunks;
			it.slot = j;
		} else if (n_fixed <= 8) {
			// small table: every corner of every sample hits the slice(s) -> dense atomics -> fixed point;
			// <= 4 slices also split the SAMPLES over up to 16 workgroups (few flush atomics)
			if (n_fixed <= 4) it.n_chunks = std::max(1u, std::min(16u / n_fixed, div_round_up(n, 2048u)));
		} else if (geo.hashed) {
			// hashed level: corners scatter over the table -> >= 16 float slices see <= 1/16 of them (sparse atomics)
			it.kind = SLICE_FLOAT;
			it.n_slices = std::max(16u, div_round_up(entries, cap_float));
		} else {
			it.kind = SLICE_GLOBAL_ATOMIC;
			it.n_slices = std::max(1u, div_round_up(n, SLICED_THREADS * 4u));  // sample tiles
		}
		items.push_back(it);
	}
	if (n_records > 0xFFFFFFFFull) throw std::runtime_error("grid_backward: batch too large for the bucketed backward");
	// persistent scatter workgroups (four fit a CU's LDS at a time; twice that many are launched)
	bk.wgs_per_level = bk.n_levels ? std::max(1u, std::min(bk.tiles, div_round_up(BUCKET_RESIDENT_WGS, bk.n_levels))) : 1u;
	bk.scatter_blocks = bk.n_levels * bk.wgs_per_level;
	bk.zero_block_begin[bk.n_levels] = n_zero_blocks;
	bk.overflow_counter = n_counters;
	bk.overflow_capacity = (uint32_t)n_records;
	bk.level_sum_base = (n_counters + 2u + 1u) & ~1u;
	bp.n_counters = bk.n_levels ? bk.level_sum_base + 2u * LEVEL_SUM_PARTS * MAX_BUCKET_LEVELS : 0;
	bp.overflow_offset = next_multiple<size_t>(n_queue_records * pair_words(F) * sizeof(uint32_t), 256);
	bp.workspace_bytes = bk.n_levels ? bp.overflow_offset + next_multiple<size_t>(n_records * (record_words(F) + 1) * sizeof(uint32_t), 256) : 0;

	// long passes first (bucket owners, float slices), the short work (fixed-point chunks, atomic tiles) fills the tail
	auto is_long = [](const Item& it) { return it.kind == SLICE_FLOAT || it.kind == SLICE_BUCKET; };
	std::stable_sort(items.begin(), items.end(), [&](const Item& a, const Item& b) { return is_long(a) > is_long(b); });

	SlicePlan& plan = bp.slices;
	plan.n_items = (uint32_t)items.size();
	uint32_t blocks = 0;
	for (uint32_t p = 0; p < plan.n_items; ++p) {
		const Item& it = items[p];
		plan.block_begin[p] = blocks;
		plan.n_slices[p] = it.n_slices;
		plan.level[p] = (uint8_t)it.level;
		plan.kind[p] = (uint8_t)it.kind;
		plan.slot[p] = (uint8_t)it.slot;
		bp.n_chunks.push_back(it.n_chunks);
		blocks += it.n_slices * it.n_chunks;
		if (it.kind == SLICE_BUCKET) bp.buckets.n_owner_blocks += it.n_slices * it.n_chunks;
	}
	plan.block_begin[plan.n_items] = blocks;
	uint32_t widest = 1;
	for (uint32_t p = 0; p < plan.n_items; ++p) widest = std::max(widest, plan.block_begin[p + 1] - plan.block_begin[p]);
	if ((uint64_t)plan.n_items * widest * 10 <= (uint64_t)blocks * 11) {  // <= 10 % padding: index by arithmetic
		plan.blocks_per_item = widest;
		bp.blocks = plan.n_items * widest;
	} else {
		plan.blocks_per_item = 0;
		bp.blocks = blocks;
	}
	return bp;
}

// The two passes of the bucketed mode, each launched from the file that holds its kernel (grid_backward_scatter.hip, grid_backward_owner.hip);
// grid_backward.hip runs them in turn.  `counters`, `queues`, `overflow`: the three parts of the GridBackwardWorkspace.
void launch_bucket_scatter(hipStream_t stream, const GridMeta& meta, const GridIO& io, const BucketPlan& plan, const half_t* dL_dy, uint32_t* counters,
                           uint32_t* queues, uint32_t* overflow, half_t* grid_gradient, bool accumulate);
// pass B of the plan's bucket items in the packed kernel; force_wide: every slice through its 64-bit redo (grid_owner_mode() == 2)
void launch_bucket_owners(hipStream_t stream, const GridMeta& meta, const BackwardPlan& bp, bool accumulate, bool force_wide, uint32_t* counters,
                          const uint32_t* queues, const uint32_t* overflow, half_t* grid_gradient);

}  // namespace tcnn_hip

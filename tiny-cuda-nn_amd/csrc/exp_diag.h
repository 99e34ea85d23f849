// exp_diag.h -- the experiment switches of the kernels: timing ladders that skip ONE phase of a kernel so that its stage time says what
// the phase costs (profiles/r03_exp_notes.txt section 10, r04_exp_notes.txt).  The results of such a build are WRONG ON PURPOSE.
//
// In the product build this header is empty of effect: the switches are compile-time zeros, the code they guard is dead (the ISA of the
// shipped kernels is the same with and without the guarded lines).  An experiment build passes -DTCNN_EXPERIMENT together with a switch
// (scripts/build_variant_one.sh adds the flag for every -DTCNN_EXP_* it is given):
//   * a switch without the flag is a compile error;
//   * csrc/Makefile, which builds the shipped libraries, refuses the flag;
//   * an object built with it exports `tcnn_experiment_build_marker`: tests/test_library.py requires the shipped libraries to have no
//     such symbol, tinycudann._C.is_experiment_build() tells a process which kind it loaded and bench.py says so in its line.
#pragma once
#include <cstdint>

#if defined(TCNN_EXPERIMENT)
extern "C" __attribute__((weak, visibility("default"))) int tcnn_experiment_build_marker = 1;
#else
#if defined(TCNN_EXP_DIAG_SCATTER) || defined(TCNN_EXP_DIAG_OWNER) || defined(TCNN_EXP_COUNT_ZERO_PAIRS)
#error "TCNN_EXP_* switches exist in experiment builds only: add -DTCNN_EXPERIMENT (scripts/build_variant_one.sh does)"
#endif
#endif

namespace tcnn_hip {
// k_grid_bucket_scatter: bit 0 no queue stores, bit 1 no reservation atomics, bit 2 no reordering stores, bit 3 no rank atomics
#if defined(TCNN_EXP_DIAG_SCATTER)
constexpr uint32_t EXP_DIAG_SCATTER = TCNN_EXP_DIAG_SCATTER;
#else
constexpr uint32_t EXP_DIAG_SCATTER = 0u;
#endif
// k_grid_bucket_owner: bit 0 no table clear, bit 1 no LDS atomics, bit 2 no conversion / store, bit 3 no last-owner protocol
#if defined(TCNN_EXP_DIAG_OWNER)
constexpr uint32_t EXP_DIAG_OWNER = TCNN_EXP_DIAG_OWNER;
#else
constexpr uint32_t EXP_DIAG_OWNER = 0u;
#endif
// k_grid_bucket_scatter with -DTCNN_EXP_COUNT_ZERO_PAIRS: counts, per level, the pair records it derives and those whose payloads are all
// +-0 (global atomics per pair: the kernel's TIME means nothing in such a build, its results are the shipped ones);
// tcnn_exp_zero_pair_counts() reads the table (scripts/exp_zero_records.py).  The table and its reader are defined HERE: the switch goes
// to the ONE object that holds the scatter (scripts/build_variant_one.sh ... grid_backward_scatter), which includes this header after
// grid_backward_plan.h.
#if defined(TCNN_EXP_COUNT_ZERO_PAIRS)
constexpr bool EXP_COUNT_ZERO_PAIRS = true;
__device__ unsigned long long g_exp_pair_counts[MAX_N_LEVELS][2];
TCNN_DEVICE void exp_count_pair(uint32_t level, bool zero) {
	atomicAdd(&g_exp_pair_counts[level][0], 1ull);
	if (zero) atomicAdd(&g_exp_pair_counts[level][1], 1ull);
}
// out: [MAX_N_LEVELS][2] = {pairs, all-zero pairs} since the last reset (may be null); returns MAX_N_LEVELS, or -1
extern "C" __attribute__((visibility("default"), used)) int tcnn_exp_zero_pair_counts(unsigned long long* out, int reset) {
	if (hipDeviceSynchronize() != hipSuccess) return -1;
	if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_exp_pair_counts), sizeof(g_exp_pair_counts)) != hipSuccess) return -1;
	if (reset) {
		static const unsigned long long zeros[MAX_N_LEVELS][2] = {};
		if (hipMemcpyToSymbol(HIP_SYMBOL(g_exp_pair_counts), zeros, sizeof(zeros)) != hipSuccess) return -1;
	}
	return (int)MAX_N_LEVELS;
}
#else
constexpr bool EXP_COUNT_ZERO_PAIRS = false;
constexpr void exp_count_pair(uint32_t, bool) {}  // (constexpr: callable from host and device code alike)
#endif
}  // namespace tcnn_hip

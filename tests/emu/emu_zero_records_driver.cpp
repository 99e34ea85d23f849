// emu_zero_records_driver.cpp -- the bucketed grid backward (csrc/grid_backward_scatter.hip, grid_backward_owner.hip) built for the host under
// the SIMT emulator (hip_emu.h), behind one entry point that also reports how many pair records the scatter queued and how many records it
// sent through the overflow list.  Built twice per 16-bit type: as shipped, and with -DTCNN_TEST_KEEP_ZERO_RECORDS (every record is kept, as
// before all-zero records were dropped): tests/test_emu_zero_records.py compares the two bit for bit.  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#define TCNN_HOST_EMU 1
#include "../../tiny-cuda-nn_amd/csrc/grid_kernels.hip"

#include <vector>

using namespace tcnn_hip;

#pragma GCC visibility push(default)
extern "C" {

// (the layout of emu.py's EmuGrid)
struct EmuGrid {
	uint32_t n_dims, n_levels, n_feat, grid_type, interp;
	float max_level;
	const uint32_t* offset;      // [L+1]
	const float* scale;          // [L]
	const uint32_t* resolution;  // [L]
};

static GridMeta make_meta(const EmuGrid* e) {
	GridMeta m = {};
	m.n_dims = e->n_dims;
	m.n_levels = e->n_levels;
	m.n_feat = e->n_feat;
	m.grid_type = e->grid_type;
	m.interp = e->interp & 0xFFu;
	m.stochastic = (e->interp >> 8) & 1u;
	m.max_level = e->max_level;
	for (uint32_t l = 0; l <= e->n_levels; ++l) m.offset[l] = e->offset[l];
	for (uint32_t l = 0; l < e->n_levels; ++l) {
		m.scale[l] = e->scale[l];
		m.resolution[l] = e->resolution[l];
	}
	return m;
}

// what the scatter left in the counters, read between the two passes (the emulator's launches are synchronous)
struct Probe {
	const uint32_t* counters;
	uint32_t n_queues;  // == BucketPlan::overflow_counter
	uint64_t queued_pairs, overflow_records;
};
static void after_scatter(void* user, int phase, int begin) {
	Probe* p = (Probe*)user;
	if (phase != 0 || begin != 0) return;
	for (uint32_t q = 0; q < p->n_queues; ++q) p->queued_pairs += p->counters[q];
	p->overflow_records += p->counters[p->n_queues];
}

int emuzr_keeps_zero_records() {
#if defined(TCNN_TEST_KEEP_ZERO_RECORDS)
	return 1;
#else
	return 0;
#endif
}

// Bucketed backward.  ddx: [n][D] or null (null: first order).  dL_dy feature-major [L*F][n].  grad_half [n_params]: overwritten, or added to
// when accumulate != 0.  stats[0]: pair records reserved in the queues, stats[1]: records pushed to the overflow list.  Fails if a counter
// is left non-zero or a level is not in the bucket plan.
int emuzr_grid_backward(const EmuGrid* e, const float* positions, const float* ddx, uint32_t n, const uint16_t* dL_dy, uint16_t* grad_half, int accumulate,
                        uint64_t* stats) {
	try {
		const GridMeta meta = make_meta(e);
		GridIO io = {positions, e->n_dims, 1, n, n, 1u};
		if (ddx) {
			io.ddx = ddx;
			io.ddx_stride_i = e->n_dims;
			io.ddx_stride_d = 1;
		}
		const BackwardPlan bp = make_backward_plan(meta, n, meta.n_feat % 2 == 0, true, accumulate != 0, 0);
		for (uint32_t p = 0; p < bp.slices.n_items; ++p) {
			if (bp.slices.kind[p] != SLICE_BUCKET) throw std::runtime_error("a level is outside the bucket plan");
		}
		GridBackwardWorkspace ws = grid_backward_workspace_size(meta, n, GridBackwardMode::Bucketed, 0);
		std::vector<unsigned char> scratch(ws.scratch_bytes + 16, 0xCD);  // garbage-filled: the call must not rely on clean scratch
		std::vector<uint32_t> counters(ws.n_counters + 1, 0u);            // zero on entry, zero on exit (checked below)
		ws.scratch = scratch.data();
		ws.counters = counters.data();
		Probe probe = {counters.data(), bp.buckets.overflow_counter, 0, 0};
		ws.phase_hook = after_scatter;
		ws.hook_user = &probe;
		grid_backward(nullptr, meta, io, (const half_t*)dL_dy, (half_t*)grad_half, accumulate != 0, GridBackwardMode::Bucketed, 0, ws);
		for (uint32_t c : counters) {
			if (c != 0u) throw std::runtime_error("bucketed backward left a non-zero counter behind");
		}
		stats[0] = probe.queued_pairs;
		stats[1] = probe.overflow_records;
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuzr_grid_backward: %s\n", ex.what());
		return 1;
	}
	return 0;
}

// chunks per bucketed level of the plan, [n_levels] (the test wants a chunked level and unchunked ones)
int emuzr_level_chunks(const EmuGrid* e, uint32_t n, int accumulate, uint32_t* out) {
	try {
		const GridMeta meta = make_meta(e);
		const BackwardPlan bp = make_backward_plan(meta, n, meta.n_feat % 2 == 0, true, accumulate != 0, 0);
		for (uint32_t l = 0; l < meta.n_levels; ++l) out[l] = 0u;
		for (uint32_t j = 0; j < bp.buckets.n_levels; ++j) out[bp.buckets.level[j]] = bp.buckets.n_chunks[j];
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuzr_level_chunks: %s\n", ex.what());
		return 1;
	}
	return 0;
}

}  // extern "C"
#pragma GCC visibility pop

// emu_driver_grid.cpp -- the grid encoding's part of the emulator's driver (emu_driver.h): csrc/grid_kernels.hip as one unit, and the
// probes of single device functions.  Also the only part of the -DTCNN_TEST_KEEP_ZERO_RECORDS libraries (every record is kept, as before
// all-zero records were dropped: tests/test_emu_zero_records.py compares the two bit for bit).  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#include "emu_driver.h"
#include "../../tiny-cuda-nn_amd/csrc/grid_kernels.hip"

#include <vector>

using namespace tcnn_hip;

namespace {

GridIO make_io(const EmuGrid* e, const float* positions, uint32_t n, uint32_t stride_k, uint32_t stride_i, const float* max_level, const float* ddx = nullptr) {
	GridIO io = {positions, e->n_dims, 1, n, stride_k, stride_i};
	io.max_level = max_level;
	if (ddx) {
		io.ddx = ddx;
		io.ddx_stride_i = e->n_dims;
		io.ddx_stride_d = 1;
	}
	return io;
}

// The workspace of one grid_backward call: scratch filled with garbage (the call must not rely on clean scratch), counters zero on entry
// and -- check() -- zero on exit.
struct Workspace {
	GridBackwardWorkspace ws;
	std::vector<unsigned char> scratch;
	std::vector<uint32_t> counters;
	Workspace(const GridMeta& meta, uint32_t n, GridBackwardMode mode, uint32_t lds_budget)
		: ws(grid_backward_workspace_size(meta, n, mode, lds_budget)), scratch(ws.scratch_bytes + 16, 0xCD), counters(ws.n_counters + 1, 0u) {
		ws.scratch = scratch.data();
		ws.counters = counters.data();
	}
	void check() const {
		for (uint32_t c : counters) {
			if (c != 0u) throw std::runtime_error("bucketed backward left a non-zero counter behind");
		}
	}
};

// what the scatter left in the counters, read between the two passes (the emulator's launches are synchronous)
struct Probe {
	const uint32_t* counters;
	uint32_t n_queues;  // == BucketPlan::overflow_counter
	uint64_t queued_pairs, overflow_records;
};
void after_scatter(void* user, int phase, int begin) {
	Probe* p = (Probe*)user;
	if (phase != 0 || begin != 0) return;
	for (uint32_t q = 0; q < p->n_queues; ++q) p->queued_pairs += p->counters[q];
	p->overflow_records += p->counters[p->n_queues];
}

}  // namespace

// (the library is built with hidden visibility -- emu.py says why; only the entry points below are exported)
#pragma GCC visibility push(default)
extern "C" {

// ---- probes of single device functions ------------------------------------------------------------------------
unsigned long long emu_level_sum_units(float total) { return level_sum_units(total); }
unsigned long long emu_saturating_add_u64(unsigned long long a, unsigned long long b) { return saturating_add_u64(a, b); }
// a[i] += b[i] through the packed 16-bit atomic of the emulator (n even)
void emu_atomic_add_h2(uint64_t n, uint16_t* a, const uint16_t* b) {
	for (uint64_t i = 0; i + 1 < n; i += 2) atomic_add_h2((half_t*)a + i, *(const h2*)((const half_t*)b + i));
}
void emu_fma_h(uint64_t n, const uint16_t* a, const uint16_t* b, const uint16_t* c, uint16_t* out) {
	for (uint64_t i = 0; i < n; ++i) ((half_t*)out)[i] = fma_h(((const half_t*)a)[i], ((const half_t*)b)[i], ((const half_t*)c)[i]);
}

// ---- the grid encoding: max_level is [n] (GridIO::max_level) or null wherever it appears ------------------------
// positions: [n][D] ; out: feature-major [L*F][n] when soa != 0 else sample-major [n][out_stride]
// dy_dx == null: the tiled gather (tile and segment search); dy_dx given: the reference-form kernel.
int emu_grid_forward(const EmuGrid* e, const float* max_level, const float* positions, uint32_t n, const uint16_t* params, uint16_t* out, int soa, uint32_t out_stride,
                     float* dy_dx) {
	return emu_call(__func__, [&] {
		grid_forward(nullptr, make_meta(e), make_io(e, positions, n, soa ? n : 1u, soa ? 1u : out_stride, max_level), (const half_t*)params, (half_t*)out, dy_dx);
	});
}

// The tiled gather's work plan (make_forward_plan, host code of the library): segments[x][k] = {level, tile_begin, tile_end} for XCD x.
// out: [8][FWD_MAX_SEGMENTS][3] u32, n_segments: [8]; returns the sample tiles per level (0 on failure).
uint32_t emu_grid_forward_plan(const EmuGrid* e, uint32_t n, uint32_t tile_samples, uint32_t* n_segments, uint32_t* out, uint32_t max_segments) {
	uint32_t tiles = 0;
	emu_call(__func__, [&] {
		const ForwardPlan plan = make_forward_plan(make_meta(e), n, tile_samples);
		for (uint32_t x = 0; x < 8; ++x) {
			n_segments[x] = plan.n_segments[x];
			for (uint32_t k = 0; k < plan.n_segments[x] && k < max_segments; ++k) {
				out[(x * max_segments + k) * 3 + 0] = plan.segments[x][k].level;
				out[(x * max_segments + k) * 3 + 1] = plan.segments[x][k].tile_begin;
				out[(x * max_segments + k) * 3 + 2] = plan.segments[x][k].tile_end;
			}
		}
		tiles = plan.tiles;
	});
	return tiles;
}

// The host plan of a backward call, per level: out[l] = {kind (SliceKind: 0 fixed-point slices, 1 fp32 / packed slices, 2 global atomics,
// 3 bucketed), table slices, sample chunks per slice}.  mode / accumulate / lds_budget as grid_backward() takes them.
int emu_grid_backward_plan(const EmuGrid* e, uint32_t n, int mode, int accumulate, uint32_t lds_budget, uint32_t* out) {
	return emu_call(__func__, [&] {
		const bool packed = mode != (int)GridBackwardMode::SlicedF32, bucketed = mode == (int)GridBackwardMode::Bucketed;
		const BackwardPlan bp = make_backward_plan(make_meta(e), n, packed, bucketed, accumulate != 0, lds_budget);
		for (uint32_t p = 0; p < bp.slices.n_items; ++p) {
			uint32_t* o = out + 3u * bp.slices.level[p];
			o[0] = bp.slices.kind[p];
			o[1] = bp.slices.n_slices[p];
			o[2] = bp.n_chunks[p];
		}
	});
}

// slices the packed owner kernel finished from its packed table / redid with 64 bits per value, since the last call (by whichever entry
// point ran a bucketed backward in between: a test calls this once to clear, runs its pass, and calls it again)
void emu_grid_owner_stats(unsigned long* packed_wide) {
	for (int i = 0; i < 2; ++i) {
		packed_wide[i] = owner_slice_stats[i];
		owner_slice_stats[i] = 0;
	}
}

// owner: the accumulator form of the bucket owners (grid_owner_mode()), set for this call; every other entry point that runs a bucketed
// backward sets the default (0, packed).
int emu_grid_backward(const EmuGrid* e, const float* max_level, const float* positions, uint32_t n, const uint16_t* dL_dy, int soa, uint32_t dy_stride, uint16_t* grad_half,
                      int accumulate, int mode, uint32_t lds_budget, int owner) {
	return emu_call(__func__, [&] {
		const GridMeta meta = make_meta(e);
		Workspace w(meta, n, (GridBackwardMode)mode, lds_budget);
		grid_owner_mode() = owner;
		grid_backward(nullptr, meta, make_io(e, positions, n, soa ? n : 1u, soa ? 1u : dy_stride, max_level), (const half_t*)dL_dy, (half_t*)grad_half, accumulate != 0,
		              (GridBackwardMode)mode, lds_budget, w.ws);
		w.check();
	});
}

// second order (grid.h:352-655): any of grad_half (the parameter scatter with the second-order weight) / dL_ddLdy / dL_dx (the position
// kernel) may be null.  dL_dy and dL_ddLdy feature-major [K][n]; dy_dx is read for dL_ddLdy only.
int emu_grid_backward_backward(const EmuGrid* e, const float* max_level, const float* positions, const float* ddx, uint32_t n, const uint16_t* dL_dy, const uint16_t* params,
                               const float* dy_dx, uint16_t* grad_half, uint16_t* dL_ddLdy, float* dL_dx) {
	return emu_call(__func__, [&] {
		const GridMeta meta = make_meta(e);
		const GridIO io = make_io(e, positions, n, n, 1u, max_level, ddx);
		if (grad_half) {
			Workspace w(meta, n, GridBackwardMode::Bucketed, 0);
			grid_owner_mode() = 0;
			grid_backward(nullptr, meta, io, (const half_t*)dL_dy, (half_t*)grad_half, false, GridBackwardMode::Bucketed, 0, w.ws);
			w.check();
		}
		if (dL_ddLdy) grid_backward_backward_dLdoutput(nullptr, e->n_dims, e->n_levels * e->n_feat, 0, io, dy_dx, (half_t*)dL_ddLdy);
		if (dL_dx) grid_backward_backward_input(nullptr, meta, io, (const half_t*)dL_dy, (const half_t*)params, dL_dx, e->n_dims, 1);
	});
}

int emu_grid_backward_input(const EmuGrid* e, uint32_t n, const uint16_t* dL_dy, int soa, uint32_t dy_stride, const float* dy_dx, float* dL_dx) {
	grid_backward_input(nullptr, e->n_dims, e->n_levels * e->n_feat, make_io(e, nullptr, n, soa ? n : 1u, soa ? 1u : dy_stride, nullptr), (const half_t*)dL_dy, dy_dx, dL_dx,
	                    e->n_dims, 1);
	return 0;
}

// GridEncodingTemplated<float>: fp32 parameters / features / gradients (sample-major [n][stride] features and gradients)
int emu_grid_forward_f32(const EmuGrid* e, const float* max_level, const float* positions, uint32_t n, const float* params, float* out, uint32_t out_stride, float* dy_dx) {
	return emu_call(__func__, [&] { grid_forward(nullptr, make_meta(e), make_io(e, positions, n, 1u, out_stride, max_level), params, out, dy_dx); });
}
int emu_grid_backward_f32(const EmuGrid* e, const float* max_level, const float* positions, uint32_t n, const float* dL_dy, uint32_t dy_stride, float* grad, int accumulate) {
	return emu_call(__func__, [&] { grid_backward(nullptr, make_meta(e), make_io(e, positions, n, 1u, dy_stride, max_level), dL_dy, grad, accumulate != 0); });
}
int emu_grid_backward_input_f32(const EmuGrid* e, uint32_t n, const float* dL_dy, uint32_t dy_stride, const float* dy_dx, float* dL_dx) {
	grid_backward_input(nullptr, e->n_dims, e->n_levels * e->n_feat, make_io(e, nullptr, n, 1u, dy_stride, nullptr), dL_dy, dy_dx, dL_dx, e->n_dims, 1);
	return 0;
}

// The second-order pass of an fp32 grid encoding (the three T = float kernels) in the layout tcnn_module_backward_backward_input passes.
// positions, ddx: [n][D]; dL_dy, dL_ddLdy: [n][stride] (stride >= L*F; the columns beyond are padding); dy_dx: [L*F][n][D] as the forward
// pass stores it; params, grad: [n_params].  grad (overwritten), dL_ddLdy and dL_dx [n][D] may each be null.
int emuso_second_order_f32(const EmuGrid* e, const float* max_level, const float* positions, const float* ddx, uint32_t n, const float* dL_dy, uint32_t stride,
                           const float* params, const float* dy_dx, float* grad, float* dL_ddLdy, float* dL_dx) {
	return emu_call(__func__, [&] {
		const GridMeta meta = make_meta(e);
		const GridIO io = make_io(e, positions, n, 1u, stride, max_level, ddx);
		const uint32_t n_features = e->n_levels * e->n_feat;
		if (dL_ddLdy) grid_backward_backward_dLdoutput(nullptr, e->n_dims, n_features, stride - n_features, io, dy_dx, dL_ddLdy);
		if (grad) grid_backward(nullptr, meta, io, dL_dy, grad, false);
		if (dL_dx) grid_backward_backward_input(nullptr, meta, io, dL_dy, params, dL_dx, e->n_dims, 1);
	});
}

int emu_grid_indices(const EmuGrid* e, const float* positions, uint32_t n, uint32_t* indices) {
	grid_indices(nullptr, make_meta(e), make_io(e, positions, n, n, 1, nullptr), indices);
	return 0;
}

// ---- the bucketed backward with its queue statistics, as shipped and in the -DTCNN_TEST_KEEP_ZERO_RECORDS libraries ----------------------
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
	return emu_call(__func__, [&] {
		const GridMeta meta = make_meta(e);
		const BackwardPlan bp = make_backward_plan(meta, n, meta.n_feat % 2 == 0, true, accumulate != 0, 0);
		for (uint32_t p = 0; p < bp.slices.n_items; ++p) {
			if (bp.slices.kind[p] != SLICE_BUCKET) throw std::runtime_error("a level is outside the bucket plan");
		}
		Workspace w(meta, n, GridBackwardMode::Bucketed, 0);
		Probe probe = {w.counters.data(), bp.buckets.overflow_counter, 0, 0};
		w.ws.phase_hook = after_scatter;
		w.ws.hook_user = &probe;
		grid_owner_mode() = 0;
		grid_backward(nullptr, meta, make_io(e, positions, n, n, 1u, nullptr, ddx), (const half_t*)dL_dy, (half_t*)grad_half, accumulate != 0, GridBackwardMode::Bucketed, 0, w.ws);
		w.check();
		stats[0] = probe.queued_pairs;
		stats[1] = probe.overflow_records;
	});
}

// chunks per bucketed level of the plan, [n_levels] (the test wants a chunked level and unchunked ones)
int emuzr_level_chunks(const EmuGrid* e, uint32_t n, int accumulate, uint32_t* out) {
	return emu_call(__func__, [&] {
		const GridMeta meta = make_meta(e);
		const BackwardPlan bp = make_backward_plan(meta, n, meta.n_feat % 2 == 0, true, accumulate != 0, 0);
		for (uint32_t l = 0; l < meta.n_levels; ++l) out[l] = 0u;
		for (uint32_t j = 0; j < bp.buckets.n_levels; ++j) out[bp.buckets.level[j]] = bp.buckets.n_chunks[j];
	});
}

}  // extern "C"
#pragma GCC visibility pop

// emu_max_level_driver.cpp -- the grid encoding's kernels (csrc/grid_*.hip) built for the host under the SIMT emulator (hip_emu.h) and
// run with a per-sample max_level array (GridIO::max_level), behind a flat C interface (host pointers only).  A library of its own next
// to emu_driver.cpp's, whose entry points take no such array.  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
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

// max_level: [n] or null.  positions: [n][D]; out: feature-major [L*F][n] when soa != 0 else sample-major [n][out_stride].
// dy_dx == null with soa or not: the tiled gather (tile and segment search); dy_dx given: the reference-form kernel.
int emuml_grid_forward(const EmuGrid* e, const float* max_level, const float* positions, uint32_t n, const uint16_t* params, uint16_t* out, int soa, uint32_t out_stride,
                       float* dy_dx) {
	try {
		GridIO io = {positions, e->n_dims, 1, n, soa ? n : 1u, soa ? 1u : out_stride};
		io.max_level = max_level;
		grid_forward(nullptr, make_meta(e), io, (const half_t*)params, (half_t*)out, dy_dx);
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuml_grid_forward: %s\n", ex.what());
		return 1;
	}
	return 0;
}

int emuml_grid_forward_f32(const EmuGrid* e, const float* max_level, const float* positions, uint32_t n, const float* params, float* out, uint32_t out_stride, float* dy_dx) {
	try {
		GridIO io = {positions, e->n_dims, 1, n, 1u, out_stride};
		io.max_level = max_level;
		grid_forward_f32(nullptr, make_meta(e), io, params, out, dy_dx);
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuml_grid_forward_f32: %s\n", ex.what());
		return 1;
	}
	return 0;
}

// dL_dy feature-major [L*F][n]; grad_half [n_params], overwritten (pre-filled with garbage by the caller); mode as GridBackwardMode
int emuml_grid_backward(const EmuGrid* e, const float* max_level, const float* positions, uint32_t n, const uint16_t* dL_dy, uint16_t* grad_half, int mode, uint32_t lds_budget) {
	try {
		GridIO io = {positions, e->n_dims, 1, n, n, 1u};
		io.max_level = max_level;
		const GridMeta meta = make_meta(e);
		GridBackwardWorkspace ws = grid_backward_workspace_size(meta, n, (GridBackwardMode)mode, lds_budget);
		std::vector<unsigned char> scratch(ws.scratch_bytes + 16, 0xCD);  // garbage-filled: the call must not rely on clean scratch
		std::vector<uint32_t> counters(ws.n_counters + 1, 0u);            // zero on entry, zero on exit (checked below)
		if (ws.scratch_bytes) {
			ws.scratch = scratch.data();
			ws.counters = counters.data();
		}
		grid_backward(nullptr, meta, io, (const half_t*)dL_dy, (half_t*)grad_half, false, (GridBackwardMode)mode, lds_budget, ws);
		for (uint32_t c : counters) {
			if (c != 0u) throw std::runtime_error("bucketed backward left a non-zero counter behind");
		}
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuml_grid_backward: %s\n", ex.what());
		return 1;
	}
	return 0;
}

int emuml_grid_backward_f32(const EmuGrid* e, const float* max_level, const float* positions, uint32_t n, const float* dL_dy, uint32_t dy_stride, float* grad) {
	try {
		GridIO io = {positions, e->n_dims, 1, n, 1u, dy_stride};
		io.max_level = max_level;
		grid_backward_f32(nullptr, make_meta(e), io, dL_dy, grad, false);
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuml_grid_backward_f32: %s\n", ex.what());
		return 1;
	}
	return 0;
}

// second order (grid.h:352-655): grad_half (the parameter scatter with the second-order weight) and dL_dx (the position kernel) may each be null.
// dL_dy feature-major [L*F][n].
int emuml_grid_backward_backward(const EmuGrid* e, const float* max_level, const float* positions, const float* ddx, uint32_t n, const uint16_t* dL_dy, const uint16_t* params,
                                 uint16_t* grad_half, float* dL_dx) {
	try {
		const GridMeta meta = make_meta(e);
		GridIO io = {positions, e->n_dims, 1, n, n, 1u};
		io.max_level = max_level;
		io.ddx = ddx;
		io.ddx_stride_i = e->n_dims;
		io.ddx_stride_d = 1;
		if (grad_half) {
			GridBackwardWorkspace ws = grid_backward_workspace_size(meta, n, GridBackwardMode::Bucketed, 0);
			std::vector<unsigned char> scratch(ws.scratch_bytes + 16, 0xCD);
			std::vector<uint32_t> counters(ws.n_counters + 1, 0u);
			ws.scratch = scratch.data();
			ws.counters = counters.data();
			grid_backward(nullptr, meta, io, (const half_t*)dL_dy, (half_t*)grad_half, false, GridBackwardMode::Bucketed, 0, ws);
		}
		if (dL_dx) grid_backward_backward_input(nullptr, meta, io, (const half_t*)dL_dy, (const half_t*)params, dL_dx, e->n_dims, 1);
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuml_grid_backward_backward: %s\n", ex.what());
		return 1;
	}
	return 0;
}

}  // extern "C"
#pragma GCC visibility pop

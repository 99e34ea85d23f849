// emu_second_order_f32_driver.cpp -- the second-order pass of an fp32 grid encoding (csrc/grid_second_order.hip, csrc/grid_backward.hip: the
// three T = float kernels) built for the host under the SIMT emulator (hip_emu.h), behind a flat C interface (host pointers only), in the
// layout tcnn_module_backward_backward_input passes: sample-major matrices of `stride` columns.  A library of its own next to
// emu_driver.cpp's.  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#define TCNN_HOST_EMU 1
#include "../../tiny-cuda-nn_amd/csrc/grid_kernels.hip"

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

// max_level: [n] or null.  positions, ddx: [n][D]; dL_dy, dL_ddLdy: [n][stride] (stride >= L*F; the columns beyond are padding); dy_dx:
// [L*F][n][D] as the forward pass stores it; params, grad: [n_params].  grad (overwritten), dL_ddLdy and dL_dx [n][D] may each be null.
int emuso_second_order_f32(const EmuGrid* e, const float* max_level, const float* positions, const float* ddx, uint32_t n, const float* dL_dy, uint32_t stride,
                           const float* params, const float* dy_dx, float* grad, float* dL_ddLdy, float* dL_dx) {
	try {
		const GridMeta meta = make_meta(e);
		GridIO io = {positions, e->n_dims, 1, n, 1u, stride};
		io.max_level = max_level;
		io.ddx = ddx;
		io.ddx_stride_i = e->n_dims;
		io.ddx_stride_d = 1;
		const uint32_t n_features = e->n_levels * e->n_feat;
		if (dL_ddLdy) grid_backward_backward_dLdoutput(nullptr, e->n_dims, n_features, stride - n_features, io, dy_dx, dL_ddLdy);
		if (grad) grid_backward_f32(nullptr, meta, io, dL_dy, grad, false);
		if (dL_dx) grid_backward_backward_input_f32(nullptr, meta, io, dL_dy, params, dL_dx, e->n_dims, 1);
	} catch (const std::exception& ex) {
		fprintf(stderr, "emuso_second_order_f32: %s\n", ex.what());
		return 1;
	}
	return 0;
}

}  // extern "C"
#pragma GCC visibility pop

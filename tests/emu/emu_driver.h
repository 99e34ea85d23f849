// emu_driver.h -- what the parts of the host emulator's driver share.  The driver builds the gfx950 kernel SOURCES for the host under
// the SIMT emulator (hip_emu.h) and exposes them to pytest through a flat C interface (host pointers only).  Its parts, one object per
// kernel family, all linked into ONE library per build variant (emu.py lists them and says which variants there are):
//   emu_driver_grid.cpp  the grid encoding (csrc/grid_kernels.hip) and the probes of single device functions
//   emu_driver_mlp.cpp   the network kernels (csrc/mlp_kernels.hip, mlp_train_wave.hip, mlp_train_wide.hip)
//   emu_driver_misc.cpp  the elementwise, composite and optimizer kernels, the trainer snapshot
//   emu_driver_half_input.cpp  csrc/half_input_kernels.hip (file-local names that clash with the optimizer kernels')
// A NEW ENTRY POINT goes into the part that already includes its kernels, its numpy front-end into emu.py (or the feature module next to
// it that calls emu.lib()): no new driver file, no new library.  The parts share the library's state (::emu::g, grid_owner_mode(),
// owner_slice_stats): an entry point sets what it depends on, never relies on a fresh library.  TEST INFRASTRUCTURE ONLY -- see hip_emu.h.
#pragma once
#define TCNN_HOST_EMU 1
#include "../../tiny-cuda-nn_amd/csrc/grid_kernels.h"
#include "../../tiny-cuda-nn_amd/csrc/mlp_kernels.h"

#include <cstdio>
#include <exception>
#include <type_traits>

// (the layout of emu.py's EmuGrid)
struct EmuGrid {
	uint32_t n_dims, n_levels, n_feat, grid_type, interp;
	float max_level;
	const uint32_t* offset;      // [L+1]
	const float* scale;          // [L]
	const uint32_t* resolution;  // [L]
};

inline tcnn_hip::GridMeta make_meta(const EmuGrid* e) {
	tcnn_hip::GridMeta m = {};
	m.n_dims = e->n_dims;
	m.n_levels = e->n_levels;
	m.n_feat = e->n_feat;
	m.grid_type = e->grid_type;
	m.interp = e->interp & 0xFFu;
	m.stochastic = (e->interp >> 8) & 1u;  // emu.py packs the flag into the interpolation word
	m.max_level = e->max_level;
	for (uint32_t l = 0; l <= e->n_levels; ++l) m.offset[l] = e->offset[l];
	for (uint32_t l = 0; l < e->n_levels; ++l) {
		m.scale[l] = e->scale[l];
		m.resolution[l] = e->resolution[l];
	}
	return m;
}

// (the layout of emu.py's EmuMlp)
struct EmuMlp {
	uint32_t in_width, width, padded_out, n_hidden_matmuls, activation, output_activation;
};
inline tcnn_hip::MlpMeta make_mlp(const EmuMlp* e) {
	return tcnn_hip::MlpMeta{e->in_width, e->width, e->padded_out, e->n_hidden_matmuls, e->activation, e->output_activation};
}

// An entry point's body -> its return code: 0, or what the body returns (2: no kernel instance takes the case); 1 with the message on
// stderr if it throws.
template <typename Body>
int emu_call(const char* name, Body&& body) {
	try {
		if constexpr (std::is_void_v<decltype(body())>) {
			body();
			return 0;
		} else {
			return body();
		}
	} catch (const std::exception& ex) {
		fprintf(stderr, "%s: %s\n", name, ex.what());
		return 1;
	}
}

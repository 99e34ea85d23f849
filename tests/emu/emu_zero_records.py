"""The emulated bucketed grid backward with its queue statistics (tests/emu/emu_driver_grid.cpp, emuzr_*), as shipped (emu.lib) and
with -DTCNN_TEST_KEEP_ZERO_RECORDS (emu.lib_keep: every record is kept, as before all-zero records were dropped).
TEST INFRASTRUCTURE ONLY.

`g` is an emu.Grid."""
import ctypes as C

import numpy as np

import emu
from emu import Grid, _p, available  # noqa: F401  (re-exported for the tests)


def grid_backward(g, positions, dL_dy_h, ddx=None, grad_init=None, keep=False, bf16=False):
    """Bucketed backward.  dL_dy_h [n][L*F] bit patterns; ddx [n][D]: the second-order scatter; grad_init: bit patterns to accumulate into
    (GradientMode::Accumulate), None -> Overwrite into a buffer pre-filled with garbage.
    -> (the gradient's bit patterns, pair records queued, records pushed to the overflow list).  The driver fails on a counter left non-zero."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n = positions.shape[0]
    dy = np.ascontiguousarray(np.asarray(dL_dy_h, dtype=np.uint16).T)
    grad = np.full(og.n_params, 0x3C00, dtype=np.uint16) if grad_init is None else np.array(grad_init, dtype=np.uint16)
    stats = np.zeros(2, dtype=np.uint64)
    ddx = None if ddx is None else np.ascontiguousarray(ddx, dtype=np.float32)
    lib = emu.lib_keep(bf16) if keep else emu.lib(bool(bf16))
    assert lib.emuzr_grid_backward(C.byref(g.c), _p(positions), _p(ddx), C.c_uint32(n), _p(dy), _p(grad), C.c_int(int(grad_init is not None)), _p(stats)) == 0
    return grad, int(stats[0]), int(stats[1])


def level_chunks(g, n, accumulate=False):
    """sample chunks per level of the bucket plan (> 1: several owners per table slice, combined with atomics)"""
    out = np.zeros(g.og.n_levels, dtype=np.uint32)
    assert emu.lib(False).emuzr_level_chunks(C.byref(g.c), C.c_uint32(n), C.c_int(int(accumulate)), _p(out)) == 0
    return out

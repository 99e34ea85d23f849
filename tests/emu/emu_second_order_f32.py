"""The emulated second-order pass of an fp32 grid encoding (tests/emu/emu_driver_grid.cpp, emuso_second_order_f32).  The kernels hold no
16-bit type, so the fp16 and the -DTCNN_BF16 library must agree bit for bit.  TEST INFRASTRUCTURE ONLY.

`g` is an emu.Grid (its scalar max_level travels in the struct); `max_level` a float32 array with one entry per sample, or None."""
import ctypes as C

import numpy as np

import emu
from emu import Grid, _ml, _p, available  # noqa: F401  (re-exported for the tests)


def second_order(g, max_level, params, positions, ddx, dL_dy, dy_dx=None, bf16=False):
    """params [n_params], dL_dy [n][stride >= L*F] fp32; dy_dx [n][L*F][D] (the oracle's layout) or None
    -> (dL_dparams [n_params], dL_ddLdoutput [n][stride] or None, dL_dinput [n][D]); every output is pre-filled with garbage."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    ddx = np.ascontiguousarray(ddx, dtype=np.float32)
    dL_dy = np.ascontiguousarray(dL_dy, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=np.float32)
    n, stride = dL_dy.shape
    grad = np.full(og.n_params, 7.0, dtype=np.float32)
    dx = np.full((n, og.n_dims), 7.0, dtype=np.float32)
    dLddy = j = None
    if dy_dx is not None:
        j = np.ascontiguousarray(np.transpose(np.asarray(dy_dx, dtype=np.float32), (1, 0, 2)))  # -> [L*F][n][D]
        dLddy = np.full((n, stride), 7.0, dtype=np.float32)
    assert emu.lib(bool(bf16)).emuso_second_order_f32(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), _p(ddx), C.c_uint32(n), _p(dL_dy), C.c_uint32(stride), _p(params), _p(j),
                                                      _p(grad), _p(dLddy), _p(dx)) == 0
    return grad, dLddy, dx

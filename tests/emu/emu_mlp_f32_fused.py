"""numpy front-end of the fused fp32 network kernels (csrc/mlp_f32_fused.hip, mlp_f32_fused_backward.hip, mlp_f32_fused_second_order.hip) on
the host SIMT emulator.  TEST INFRASTRUCTURE ONLY.

The entry points (emuf32f_*) call mlp_f32_fused_forward / _backward / _backward_backward directly: forward and backward are in the network's
driver part, emu_driver_mlp.cpp, of the one library that emu.py builds and loads, the second-order pass in emu_driver_mlp_second_order.cpp
next to the layer-by-layer pass (emu_mlp_second_order.py builds and loads that library).  The emulator's build sets
-DTCNN_F32F_MAX_BLOCKS=2: at most two persistent workgroups, so three sample tiles are shares of two and one.  The layer-by-layer kernels
on the same arguments are emu_mlp_f32 / emu_mlp_second_order, with the same signatures."""
import ctypes as C

import numpy as np

import emu
import emu_mlp_second_order
from emu_mlp_f32 import _p, available, meta  # noqa: F401  (re-exported for the tests)

lib = emu.lib
RESIDENT_FORWARD, RESIDENT_BACKWARD_WITH_DINPUT, RESIDENT_BACKWARD_WITHOUT_DINPUT, RESIDENT_LIMIT = 0, 1, 2, 3


def supported(m, n):
    return bool(lib().emuf32f_supported(C.byref(m), C.c_uint32(n)))


def n_partials(m, n):
    """mlp_f32_fused_n_partials"""
    return int(lib().emuf32f_n_partials(C.byref(m), C.c_uint32(n)))


def max_blocks():
    """F32F_MAX_BLOCKS of this build: the persistent workgroups of a chain launch"""
    return int(lib().emuf32f_max_blocks())


def lds_floats(m, which):
    """floats of LDS with every matrix resident, for the pass RESIDENT_* names; RESIDENT_LIMIT: what fits, above it the pass stages"""
    return int(lib().emuf32f_lds_floats(C.byref(m), C.c_uint32(which)))


def forward(m, params, input_fm, save=True):
    """-> (hidden stack or None, output [n][padded_out]); input feature-major [in_width][n]"""
    params, input_fm = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(input_fm, np.float32)
    n = input_fm.shape[1]
    hidden = np.full(int(lib().emuf32_saved_activation_floats(C.byref(m), C.c_uint32(n))), np.nan, np.float32) if save else None
    out = np.full((n, m.padded_out), np.nan, np.float32)
    assert lib().emuf32f_mlp_forward(C.byref(m), C.c_uint32(n), _p(params), _p(input_fm), _p(hidden), _p(out), None, C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)) == 0
    return hidden, out


def inference_trimmed(m, params, input_fm, dims, row_major=False, slack=3):
    """inference into a trimmed matrix with a stride `slack` above its leading dimension -> (the matrix as [n][dims], the whole buffer, its
    mask of elements that belong to the matrix)"""
    params, input_fm = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(input_fm, np.float32)
    n = input_fm.shape[1]
    if row_major:  # [dims][stride]
        stride = n + slack
        buf = np.full((dims, stride), np.nan, np.float32)
        stride_i, stride_j, view = 1, stride, buf[:, :n].T
    else:  # [n][stride]
        stride = dims + slack
        buf = np.full((n, stride), np.nan, np.float32)
        stride_i, stride_j, view = stride, 1, buf[:, :dims]
    assert lib().emuf32f_mlp_forward(C.byref(m), C.c_uint32(n), _p(params), _p(input_fm), None, None, _p(buf), C.c_uint32(dims), C.c_uint32(stride_i), C.c_uint32(stride_j)) == 0
    mask = np.zeros(buf.shape, bool)
    (mask[:, :n] if row_major else mask[:, :dims])[...] = True
    return view, buf, mask


def backward(m, params, input_fm, hidden, dL_doutput, grads_init=None, output=None, want_dinput=True, want_grads=True):
    """-> (grads [n_params], dL_dinput feature-major [in_width][n]), None where not asked for.  grads_init: accumulate into a copy of it;
    else overwrite garbage."""
    params, input_fm = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(input_fm, np.float32)
    n = input_fm.shape[1]
    dinput = np.full((m.in_width, n), np.nan, np.float32) if want_dinput else None
    grads = None
    if want_grads:
        grads = np.full(params.shape, 7.0, np.float32) if grads_init is None else np.ascontiguousarray(grads_init, np.float32).copy()
    assert lib().emuf32f_mlp_backward(C.byref(m), C.c_uint32(n), _p(params), _p(input_fm), _p(hidden), _p(np.ascontiguousarray(dL_doutput, np.float32)), _p(dinput), _p(grads),
                                      C.c_int(int(grads_init is not None)), _p(None if output is None else np.ascontiguousarray(output, np.float32))) == 0
    return grads, dinput


def backward_backward(m, params, input_fm, hidden, v_fm, dL_doutput, want_ddy=True, want_dinput=True, want_grads=True):
    """-> (dL_ddLdoutput [n][padded_out], dL_dinput feature-major [in_width][n], grads [n_params]), None where not asked for; every result
    is pre-filled with garbage.  input_fm, v_fm feature-major [in_width][n]; dL_doutput [n][padded_out]."""
    params, input_fm, v_fm = (np.ascontiguousarray(a, np.float32) for a in (params, input_fm, v_fm))
    n = input_fm.shape[1]
    ddy = np.full((n, m.padded_out), np.nan, np.float32) if want_ddy else None
    dinput = np.full((m.in_width, n), np.nan, np.float32) if want_dinput else None
    grads = np.full(params.shape, 7.0, np.float32) if want_grads else None
    dy = None if dL_doutput is None else np.ascontiguousarray(dL_doutput, np.float32)
    assert emu_mlp_second_order.lib().emuf32f_backward_backward(C.byref(m), C.c_uint32(n), _p(params), _p(input_fm), _p(hidden), _p(v_fm), _p(dy), _p(ddy), _p(dinput),
                                                                _p(grads)) == 0
    return ddy, dinput, grads

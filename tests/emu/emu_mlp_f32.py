"""numpy front-end of the fp32 network kernels (csrc/mlp_general_fp32.hip) on the host SIMT emulator.  TEST INFRASTRUCTURE ONLY.

The entry points (emuf32_*) are in the network's driver part, emu_driver_mlp.cpp, of the one emulator library that emu.py builds and loads."""
import ctypes as C

import numpy as np

import emu


def available():
    return emu.available()


lib = emu.lib


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"] and a.dtype == np.float32
    return a.ctypes.data_as(C.c_void_p)


def meta(in_width, width, padded_out, n_hidden, activation=1, output_activation=0):
    return emu.EmuMlp(in_width, width, padded_out, n_hidden - 1, activation, output_activation)


def n_partials(m, n):
    return int(lib().emuf32_n_partials(C.byref(m), C.c_uint32(n)))


def forward(m, params, input_fm, save=True):
    """-> (hidden stack or None, output [n][padded_out]); input feature-major [in_width][n]"""
    params, input_fm = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(input_fm, np.float32)
    n = input_fm.shape[1]
    hidden = np.full(int(lib().emuf32_saved_activation_floats(C.byref(m), C.c_uint32(n))), np.nan, np.float32) if save else None
    out = np.full((n, m.padded_out), np.nan, np.float32)
    assert lib().emuf32_mlp_forward(C.byref(m), C.c_uint32(n), _p(params), _p(input_fm), _p(hidden), _p(out), None, C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)) == 0
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
    assert lib().emuf32_mlp_forward(C.byref(m), C.c_uint32(n), _p(params), _p(input_fm), None, None, _p(buf), C.c_uint32(dims), C.c_uint32(stride_i), C.c_uint32(stride_j)) == 0
    mask = np.zeros(buf.shape, bool)
    (mask[:, :n] if row_major else mask[:, :dims])[...] = True
    return view, buf, mask


def backward(m, params, input_fm, hidden, dL_doutput, grads_init=None, output=None, want_dinput=True):
    """-> (grads [n_params], dL_dinput feature-major [in_width][n]).  grads_init: accumulate into a copy of it; else overwrite garbage."""
    params, input_fm = np.ascontiguousarray(params, np.float32), np.ascontiguousarray(input_fm, np.float32)
    n = input_fm.shape[1]
    dinput = np.full((m.in_width, n), np.nan, np.float32) if want_dinput else None
    grads = np.full(params.shape, 7.0, np.float32) if grads_init is None else np.ascontiguousarray(grads_init, np.float32).copy()
    assert lib().emuf32_mlp_backward(C.byref(m), C.c_uint32(n), _p(params), _p(input_fm), _p(hidden), _p(np.ascontiguousarray(dL_doutput, np.float32)), _p(dinput), _p(grads),
                                     C.c_int(int(grads_init is not None)), _p(None if output is None else np.ascontiguousarray(output, np.float32))) == 0
    return grads, dinput

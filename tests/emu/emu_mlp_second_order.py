"""numpy front-end of the fp32 network's second-order pass (csrc/mlp_general_fp32.hip mlp_f32_backward_backward) on the host SIMT emulator.
TEST INFRASTRUCTURE ONLY.

The entry points (emumso_*) are in a driver part of their own, emu_driver_mlp_second_order.cpp, built here into a library of its own with
emu.py's compile and link command lines; the forward pass that fills the saved activations is emu_mlp_f32's, from emu.py's library."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import emu
import emu_mlp_f32
from emu_mlp_f32 import available, forward, meta  # noqa: F401  (re-exported for the tests)

_PART = os.path.join(emu._HERE, "emu_driver_mlp_second_order.cpp")
_LIB = os.path.join(emu._HERE, "libtcnn_emu_mlp_second_order.so")
_lib = None


def build(force=False):
    srcs = [os.path.join(emu._HERE, f) for f in os.listdir(emu._HERE) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(emu._CSRC, f) for f in os.listdir(emu._CSRC) if f.endswith((".hip", ".h"))]
    if not force and os.path.exists(_LIB) and os.path.getmtime(_LIB) >= max(os.path.getmtime(s) for s in srcs):
        return
    with tempfile.TemporaryDirectory(dir=emu._HERE) as tmp:
        obj = os.path.join(tmp, "emu_driver_mlp_second_order.o")
        subprocess.check_call(emu._COMPILE + [_PART, "-o", obj])
        subprocess.check_call(emu._LINK + [obj, "-o", _LIB])


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_LIB)
        _lib.emumso_workspace_floats.restype = C.c_uint64
        _lib.emumso_has_curvature.restype = C.c_uint32
    return _lib


_p = emu_mlp_f32._p


def has_curvature(m):
    return bool(lib().emumso_has_curvature(C.byref(m)))


def workspace_floats(m, n):
    return int(lib().emumso_workspace_floats(C.byref(m), C.c_uint32(n)))


def backward_backward(m, params, input_fm, hidden, v_fm, dL_doutput, want_ddy=True, want_dinput=True, want_grads=True):
    """-> (dL_ddLdoutput [n][padded_out], dL_dinput feature-major [in_width][n], grads [n_params]), None where not asked for; every result
    is pre-filled with garbage.  input_fm, v_fm feature-major [in_width][n]; dL_doutput [n][padded_out] or None."""
    params, input_fm, v_fm = (np.ascontiguousarray(a, np.float32) for a in (params, input_fm, v_fm))
    n = input_fm.shape[1]
    ddy = np.full((n, m.padded_out), np.nan, np.float32) if want_ddy else None
    dinput = np.full((m.in_width, n), np.nan, np.float32) if want_dinput else None
    grads = np.full(params.shape, 7.0, np.float32) if want_grads else None
    dy = None if dL_doutput is None else np.ascontiguousarray(dL_doutput, np.float32)
    assert lib().emumso_backward_backward(C.byref(m), C.c_uint32(n), _p(params), _p(input_fm), _p(hidden), _p(v_fm), _p(dy), _p(ddy), _p(dinput), _p(grads)) == 0
    return ddy, dinput, grads

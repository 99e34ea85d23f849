"""numpy front-end for the host-emulator build of the grid kernels run with a per-sample max_level array
(tests/emu/emu_max_level_driver.cpp): a library of its own, built the way tests/emu/emu.py builds the main one (same compiler, same
flags), IEEE fp16 and -DTCNN_BF16.  TEST INFRASTRUCTURE ONLY.

`g` is an emu.Grid (its scalar max_level travels in the struct); `max_level` a float32 array with one entry per sample, or None."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu
from emu import ATOMIC, BUCKETED, SLICED_F16, SLICED_F32, Grid  # noqa: F401  (re-exported for the tests)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "tiny-cuda-nn_amd", "csrc")
_LIBS = {False: os.path.join(_HERE, "libtcnn_emu_max_level.so"), True: os.path.join(_HERE, "libtcnn_emu_max_level_bf16.so")}
_DRIVER = os.path.join(_HERE, "emu_max_level_driver.cpp")
_loaded = {}


def available():
    return emu.available()


def build(force=False):
    sources = [_DRIVER, os.path.join(_HERE, "hip_emu.h")] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))]
    newest = max(os.path.getmtime(s) for s in sources)
    running = []
    for bf16, path in _LIBS.items():
        if force or not os.path.exists(path) or os.path.getmtime(path) < newest:
            cmd = emu._build_command(path, ["-DTCNN_BF16"] if bf16 else [], True)
            cmd[cmd.index(os.path.join(_HERE, "emu_driver.cpp"))] = _DRIVER
            running.append((cmd, subprocess.Popen(cmd)))
    failed = [c for c, p in running if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])


def lib(bf16=False):
    if bf16 not in _loaded:
        build()
        _loaded[bf16] = C.CDLL(_LIBS[bf16])
    return _loaded[bf16]


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def _ml(max_level, n):
    if max_level is None:
        return None
    max_level = np.ascontiguousarray(max_level, dtype=np.float32)
    assert max_level.shape == (n,)
    return max_level


def grid_forward(g, max_level, params_h, positions, soa=True, want_dy_dx=False, bf16=False):
    """-> features [n][L*F] (bit patterns), and dy_dx [L*F][n][D] if asked for.  Without dy_dx the tiled gather runs, with it the reference-form kernel."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n = positions.shape[0]
    k = og.n_levels * og.n_features_per_level
    out = np.full((k, n) if soa else (n, k), 0x7E00, dtype=np.uint16)  # every element must be written
    dy_dx = np.full((k, n, og.n_dims), np.nan, dtype=np.float32) if want_dy_dx else None
    ml = _ml(max_level, n)
    assert lib(bf16).emuml_grid_forward(C.byref(g.c), _p(ml), _p(positions), C.c_uint32(n), _p(np.ascontiguousarray(params_h, dtype=np.uint16)), _p(out), C.c_int(int(soa)),
                                        C.c_uint32(n if soa else k), _p(dy_dx)) == 0
    out = np.ascontiguousarray(out.T) if soa else out
    return (out, dy_dx) if want_dy_dx else out


def grid_forward_f32(g, max_level, params, positions, want_dy_dx=False):
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n = positions.shape[0]
    k = og.n_levels * og.n_features_per_level
    out = np.full((n, k), np.nan, dtype=np.float32)
    dy_dx = np.full((k, n, og.n_dims), np.nan, dtype=np.float32) if want_dy_dx else None
    assert lib().emuml_grid_forward_f32(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), C.c_uint32(n), _p(np.ascontiguousarray(params, dtype=np.float32)), _p(out),
                                        C.c_uint32(k), _p(dy_dx)) == 0
    return (out, dy_dx) if want_dy_dx else out


def grid_backward(g, max_level, positions, dL_dy_h, mode=BUCKETED, lds_budget=0):
    """dL_dy_h [n][L*F] bit patterns -> the grid gradient's bit patterns (Overwrite into a buffer pre-filled with garbage)."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n = positions.shape[0]
    dy = np.ascontiguousarray(np.asarray(dL_dy_h, dtype=np.uint16).T)
    grad = np.full(og.n_params, 0x3C00, dtype=np.uint16)
    assert lib().emuml_grid_backward(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), C.c_uint32(n), _p(dy), _p(grad), C.c_int(mode), C.c_uint32(lds_budget)) == 0
    return grad


def grid_backward_f32(g, max_level, positions, dL_dy):
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n = positions.shape[0]
    dL_dy = np.ascontiguousarray(dL_dy, dtype=np.float32)
    grad = np.full(og.n_params, 7.0, dtype=np.float32)
    assert lib().emuml_grid_backward_f32(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), C.c_uint32(n), _p(dL_dy), C.c_uint32(dL_dy.shape[1]), _p(grad)) == 0
    return grad


def grid_backward_backward(g, max_level, positions, ddx, dL_dy_h, params_h, want_params=True, want_input=True):
    """Second order: (the parameter gradient's bit patterns or None, dL_dx [n][D] or None).  dL_dy_h [n][L*F] bit patterns."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    ddx = np.ascontiguousarray(ddx, dtype=np.float32)
    n = positions.shape[0]
    dy = np.ascontiguousarray(np.asarray(dL_dy_h, dtype=np.uint16).T)
    grad = np.full(og.n_params, 0x3C00, dtype=np.uint16) if want_params else None
    dx = np.full((n, og.n_dims), 7.0, dtype=np.float32) if want_input else None
    assert lib().emuml_grid_backward_backward(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), _p(ddx), C.c_uint32(n), _p(dy),
                                              _p(np.ascontiguousarray(params_h, dtype=np.uint16)), _p(grad), _p(dx)) == 0
    return grad, dx

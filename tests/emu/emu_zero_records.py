"""numpy front-end for the host-emulator build of the bucketed grid backward behind tests/emu/emu_zero_records_driver.cpp: four libraries,
{as shipped, -DTCNN_TEST_KEEP_ZERO_RECORDS (every record is kept, as before all-zero records were dropped)} x {IEEE fp16, -DTCNN_BF16},
built the way tests/emu/emu.py builds the main one (same compiler, same flags).  TEST INFRASTRUCTURE ONLY.

`g` is an emu.Grid."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu
from emu import Grid  # noqa: F401  (re-exported for the tests)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "tiny-cuda-nn_amd", "csrc")
_DRIVER = os.path.join(_HERE, "emu_zero_records_driver.cpp")
# (keep, bf16) -> library
_LIBS = {(keep, bf16): os.path.join(_HERE, "libtcnn_emu_zero_records%s%s.so" % ("_keep" if keep else "", "_bf16" if bf16 else ""))
         for keep in (False, True) for bf16 in (False, True)}
_loaded = {}


def available():
    return emu.available()


def build(force=False):
    sources = [_DRIVER, os.path.join(_HERE, "hip_emu.h")] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))]
    newest = max(os.path.getmtime(s) for s in sources)
    running = []
    for (keep, bf16), path in _LIBS.items():
        if force or not os.path.exists(path) or os.path.getmtime(path) < newest:
            cmd = emu._build_command(path, (["-DTCNN_TEST_KEEP_ZERO_RECORDS"] if keep else []) + (["-DTCNN_BF16"] if bf16 else []), True)
            cmd[cmd.index(os.path.join(_HERE, "emu_driver.cpp"))] = _DRIVER
            running.append((cmd, subprocess.Popen(cmd)))
    failed = [c for c, p in running if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])


def lib(keep=False, bf16=False):
    key = (bool(keep), bool(bf16))
    if key not in _loaded:
        build()
        _loaded[key] = C.CDLL(_LIBS[key])
        assert _loaded[key].emuzr_keeps_zero_records() == int(key[0])
    return _loaded[key]


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


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
    assert lib(keep, bf16).emuzr_grid_backward(C.byref(g.c), _p(positions), _p(ddx), C.c_uint32(n), _p(dy), _p(grad), C.c_int(int(grad_init is not None)), _p(stats)) == 0
    return grad, int(stats[0]), int(stats[1])


def level_chunks(g, n, accumulate=False):
    """sample chunks per level of the bucket plan (> 1: several owners per table slice, combined with atomics)"""
    out = np.zeros(g.og.n_levels, dtype=np.uint32)
    assert lib().emuzr_level_chunks(C.byref(g.c), C.c_uint32(n), C.c_int(int(accumulate)), _p(out)) == 0
    return out

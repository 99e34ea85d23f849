"""numpy front-end for the host-emulator build of the fp32 grid encoding's second-order kernels (tests/emu/emu_second_order_f32_driver.cpp): a
library of its own, built the way tests/emu/emu_max_level.py builds its own (same compiler, same flags), IEEE fp16 and -DTCNN_BF16 -- the
kernels hold no 16-bit type, so the two builds must agree bit for bit.  TEST INFRASTRUCTURE ONLY.

`g` is an emu.Grid (its scalar max_level travels in the struct); `max_level` a float32 array with one entry per sample, or None."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu
from emu import Grid  # noqa: F401  (re-exported for the tests)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "tiny-cuda-nn_amd", "csrc")
_LIBS = {False: os.path.join(_HERE, "libtcnn_emu_second_order_f32.so"), True: os.path.join(_HERE, "libtcnn_emu_second_order_f32_bf16.so")}
_DRIVER = os.path.join(_HERE, "emu_second_order_f32_driver.cpp")
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


def second_order(g, max_level, params, positions, ddx, dL_dy, dy_dx=None, bf16=False):
    """params [n_params], dL_dy [n][stride >= L*F] fp32; dy_dx [n][L*F][D] (the oracle's layout) or None
    -> (dL_dparams [n_params], dL_ddLdoutput [n][stride] or None, dL_dinput [n][D]); every output is pre-filled with garbage."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    ddx = np.ascontiguousarray(ddx, dtype=np.float32)
    dL_dy = np.ascontiguousarray(dL_dy, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=np.float32)
    n, stride = dL_dy.shape
    if max_level is not None:
        max_level = np.ascontiguousarray(max_level, dtype=np.float32)
        assert max_level.shape == (n,)
    grad = np.full(og.n_params, 7.0, dtype=np.float32)
    dx = np.full((n, og.n_dims), 7.0, dtype=np.float32)
    dLddy = j = None
    if dy_dx is not None:
        j = np.ascontiguousarray(np.transpose(np.asarray(dy_dx, dtype=np.float32), (1, 0, 2)))  # -> [L*F][n][D]
        dLddy = np.full((n, stride), 7.0, dtype=np.float32)
    assert lib(bf16).emuso_second_order_f32(C.byref(g.c), _p(max_level), _p(positions), _p(ddx), C.c_uint32(n), _p(dL_dy), C.c_uint32(stride), _p(params), _p(j),
                                            _p(grad), _p(dLddy), _p(dx)) == 0
    return grad, dLddy, dx

"""numpy front-end for the host-emulator build of the network launchers behind tests/emu/emu_wide_outputs_driver.cpp: inference straight
into the caller's fp32 matrix (mlp_forward_f32).  A library of its own, built the way tests/emu/emu.py builds the main one (same compiler,
same flags), IEEE fp16 and -DTCNN_BF16.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "tiny-cuda-nn_amd", "csrc")
_LIBS = {False: os.path.join(_HERE, "libtcnn_emu_wide_outputs.so"), True: os.path.join(_HERE, "libtcnn_emu_wide_outputs_bf16.so")}
_DRIVER = os.path.join(_HERE, "emu_wide_outputs_driver.cpp")
_loaded = {}

COLUMN_MAJOR, ROW_MAJOR = 0, 1  # of the caller's n_output_dims x batch matrix (tcnn_network_inference_matrices)


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


def mlp_forward_f32(om, params_h, input_soa_h, dims, layout=COLUMN_MAJOR, stride=None, offset_floats=0, bf16=False):
    """The network's inference into an fp32 matrix of `dims` x n in either layout of the C ABI: column-major (a sample's outputs contiguous,
    samples `stride` >= dims floats apart) or row-major (an output's samples contiguous, outputs `stride` >= n floats apart).
    offset_floats shifts the matrix' first element off the buffer's 64-byte alignment.  Returns (the [n][dims] view of the result, the whole
    buffer -- pre-filled with NaN, so that a store outside the matrix' elements shows).  None where no kernel stores fp32 itself."""
    input_soa_h = np.ascontiguousarray(input_soa_h)
    n = input_soa_h.shape[1]
    cm = layout == COLUMN_MAJOR
    stride = stride or (dims if cm else n)
    assert stride >= (dims if cm else n)
    rows = n if cm else dims
    raw = np.full(rows * stride + offset_floats + 16, np.nan, dtype=np.float32)
    base = (-raw.ctypes.data // 4) % 16  # first 64-byte aligned element
    buf = raw[base:base + rows * stride + offset_floats]
    m = emu.mlp_meta(om)
    r = lib(bf16).emuwo_mlp_forward_f32(C.byref(m), C.c_uint32(n), np.ascontiguousarray(params_h).ctypes.data_as(C.c_void_p), input_soa_h.ctypes.data_as(C.c_void_p),
                                        C.c_void_p(buf.ctypes.data + 4 * offset_floats), C.c_uint32(dims), C.c_uint32(stride if cm else 1), C.c_uint32(1 if cm else stride))
    if r == 2:
        return None
    assert r == 0
    matrix = buf[offset_floats:].reshape(rows, stride)
    return (matrix[:, :dims] if cm else matrix[:, :n].T), buf

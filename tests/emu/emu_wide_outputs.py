"""The emulated network launchers' inference straight into the caller's fp32 matrix (mlp_forward_f32; tests/emu/emu_driver_mlp.cpp,
emuwo_mlp_forward_f32).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

import emu
from emu import _p, available  # noqa: F401

COLUMN_MAJOR, ROW_MAJOR = 0, 1  # of the caller's n_output_dims x batch matrix (tcnn_network_inference_matrices)


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
    r = emu.lib(bool(bf16)).emuwo_mlp_forward_f32(C.byref(m), C.c_uint32(n), _p(np.ascontiguousarray(params_h)), _p(input_soa_h), C.c_void_p(buf.ctypes.data + 4 * offset_floats),
                                                  C.c_uint32(dims), C.c_uint32(stride if cm else 1), C.c_uint32(1 if cm else stride))
    if r == 2:
        return None
    assert r == 0
    matrix = buf[offset_floats:].reshape(rows, stride)
    return (matrix[:, :dims] if cm else matrix[:, :n].T), buf

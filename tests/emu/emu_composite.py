"""The emulated kernels of csrc/composite_kernels.hip (tests/emu/emu_driver_misc.cpp, emuc_*).  TEST INFRASTRUCTURE ONLY.

Value matrices are numpy [n, rows] (sample-major, as the oracle's); `soa` runs the kernel on the feature-major transpose the network
reads.  dtype uint16: the 16-bit type's bit patterns; float32: the fp32 encodings' kernels."""
import ctypes as C

import numpy as np

from emu import _p, available, lib  # noqa: F401

IDENTITY, ONEBLOB, FREQUENCY, TRIANGLE_WAVE = 0, 1, 2, 3  # composite_kernels.h EncodingPartKind
KINDS = {"Identity": IDENTITY, "OneBlob": ONEBLOB, "Frequency": FREQUENCY, "TriangleWave": TRIANGLE_WAVE}


def _to_kernel(v, soa):
    return np.ascontiguousarray(v.T if soa else v)


def _from_kernel(v, soa):
    return np.ascontiguousarray(v.T) if soa else v


def _table(parts):
    return np.ascontiguousarray([[KINDS[p["kind"]], p["begin"], p["dims"], p["row"], p["padded"], p.get("n_bins", p.get("n_frequencies", 0))] for p in parts], dtype=np.uint32)


def triangle_wave_forward(x, n_frequencies, padded, soa=True, fp32=False, bf16=False):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    out = np.zeros((padded, n) if soa else (n, padded), dtype=np.float32 if fp32 else np.uint16)
    assert lib(bf16).emuc_triangle_wave_forward(C.c_uint32(n), C.c_uint32(d), C.c_uint32(n_frequencies), C.c_uint32(padded), _p(x), _p(out), C.c_int(int(soa)), C.c_int(int(fp32))) == 0
    return _from_kernel(out, soa)


def triangle_wave_backward(x, n_frequencies, dL_dy, soa=True, bf16=False):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    dy = _to_kernel(dL_dy, soa)
    out = np.full((n, d), 7.0, dtype=np.float32)
    assert lib(bf16).emuc_triangle_wave_backward(C.c_uint32(n), C.c_uint32(d), C.c_uint32(n_frequencies), C.c_uint32(dL_dy.shape[1]), _p(dy), C.c_int(int(soa)),
                                                 C.c_int(int(dy.dtype == np.float32)), _p(x), _p(out)) == 0
    return out


def parts_forward(parts, x, width, soa=True, fp32=False, bf16=False, fill=0):
    """rows no part writes keep `fill`"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    out = np.full((width, n) if soa else (n, width), fill, dtype=np.float32 if fp32 else np.uint16)
    t = _table(parts)
    assert lib(bf16).emuc_parts_forward(C.c_uint32(len(parts)), _p(t), C.c_uint32(n), C.c_uint32(d), C.c_uint32(width), _p(x), _p(out), C.c_int(int(soa)), C.c_int(int(fp32))) == 0
    return _from_kernel(out, soa)


def parts_backward(parts, x, dL_dy, soa=True, bf16=False):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    dy = _to_kernel(dL_dy, soa)
    out = np.full((n, d), 7.0, dtype=np.float32)
    t = _table(parts)
    assert lib(bf16).emuc_parts_backward(C.c_uint32(len(parts)), _p(t), C.c_uint32(n), C.c_uint32(d), C.c_uint32(dL_dy.shape[1]), _p(dy), C.c_int(int(soa)),
                                         C.c_int(int(dy.dtype == np.float32)), _p(x), _p(out)) == 0
    return out


def reduce_forward(to_reduce, width, product, soa=True, bf16=False):
    n, total = to_reduce.shape
    v = _to_kernel(to_reduce, soa)
    out = np.zeros((width, n) if soa else (n, width), dtype=v.dtype)
    assert lib(bf16).emuc_reduce_forward(C.c_int(int(product)), C.c_uint32(n), C.c_uint32(width), C.c_uint32(total // width), _p(v), _p(out), C.c_int(int(soa)),
                                         C.c_int(int(v.dtype == np.float32))) == 0
    return _from_kernel(out, soa)


def reduce_backward(to_reduce, dL_dreduced, width, product, soa=True, bf16=False):
    n, total = to_reduce.shape
    v, dy = _to_kernel(to_reduce, soa), _to_kernel(dL_dreduced, soa)
    out = np.zeros_like(v)
    assert lib(bf16).emuc_reduce_backward(C.c_int(int(product)), C.c_uint32(n), C.c_uint32(width), C.c_uint32(total // width), _p(v), _p(out), _p(dy), C.c_int(int(soa)),
                                          C.c_int(int(v.dtype == np.float32))) == 0
    return _from_kernel(out, soa)

"""numpy front-end for the host-emulator build of csrc/half_input_kernels.hip (tests/emu/emu_half_input_driver.cpp): a library of its own,
built the way tests/emu/emu.py builds the main one (same compiler, same flags).  The kernels move 16-bit words whatever they encode, so ONE
build serves fp16 and bf16; the padding's bit pattern is an argument.  TEST INFRASTRUCTURE ONLY.

Matrices are numpy uint16.  `offset` (in elements) places the caller-side matrix that far into a 16-byte aligned buffer, so that the
kernels' 2-byte paths run; every output lies between guard words that the calls check, so a store outside the matrix fails the call."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "tiny-cuda-nn_amd", "csrc")
_LIB = os.path.join(_HERE, "libtcnn_emu_half_input.so")
_SOURCES = [os.path.join(_HERE, "emu_half_input_driver.cpp"), os.path.join(_HERE, "hip_emu.h")] + \
           [os.path.join(_CSRC, f) for f in ("half_input_kernels.hip", "half_input_kernels.h", "tcnn_device.h")]
ONE = {False: 0x3C00, True: 0x3F80}  # 1.0 in fp16 / bf16
_GUARD, _GUARD_WORDS = 0xA5C3, 64
_loaded = []


def available():
    return emu.available()


def build(force=False):
    newest = max(os.path.getmtime(s) for s in _SOURCES)
    if force or not os.path.exists(_LIB) or os.path.getmtime(_LIB) < newest:
        cmd = emu._build_command(_LIB, [], True)
        cmd[cmd.index(os.path.join(_HERE, "emu_driver.cpp"))] = _SOURCES[0]
        subprocess.check_call(cmd)


def lib():
    if not _loaded:
        build()
        _loaded.append(C.CDLL(_LIB))
    return _loaded[0]


def _aligned(n_words, offset):
    """(buffer, view of n_words uint16 that starts `offset` elements behind a 16-byte boundary, with guard words on both sides)"""
    buf = np.full(n_words + 2 * _GUARD_WORDS + 16 + offset, _GUARD, dtype=np.uint16)
    start = (-(buf.ctypes.data // 2) % 8) + _GUARD_WORDS // 8 * 8 + offset
    return buf, buf[start:start + n_words], start


def _guards_intact(buf, start, n_words):
    return bool(np.all(buf[:start] == _GUARD) and np.all(buf[start + n_words:] == _GUARD))


def _p(a):
    return C.c_void_p(a.ctypes.data)


def pad(x, padded, bf16=False, in_offset=0, out_offset=0):
    """x [n, n_dims] -> the feature-major matrix the network reads, as numpy [padded, n]"""
    n, d = x.shape
    _, src, _ = _aligned(n * d, in_offset)
    src[:] = x.reshape(-1)
    buf, dst, start = _aligned(padded * n, out_offset)
    assert lib().emuh_pad(C.c_uint32(n), C.c_uint32(d), C.c_uint32(padded), _p(src), _p(dst), C.c_uint32(ONE[bf16])) == 0
    assert _guards_intact(buf, start, padded * n), "half_input_pad wrote outside its output"
    return dst.reshape(padded, n).copy()


def unpad(dL_dy, n_dims, in_offset=0, out_offset=0):
    """dL_dy numpy [padded, n] (feature-major) -> dL_dx [n, n_dims]"""
    padded, n = dL_dy.shape
    _, src, _ = _aligned(padded * n, in_offset)
    src[:] = dL_dy.reshape(-1)
    buf, dst, start = _aligned(n * n_dims, out_offset)
    assert lib().emuh_unpad(C.c_uint32(n), C.c_uint32(n_dims), _p(src), _p(dst)) == 0
    assert _guards_intact(buf, start, n * n_dims), "half_input_unpad wrote outside its output"
    return dst.reshape(n, n_dims).copy()

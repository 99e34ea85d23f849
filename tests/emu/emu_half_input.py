"""The emulated kernels of csrc/half_input_kernels.hip (tests/emu/emu_driver_misc.cpp, emuh_*).  The kernels move 16-bit words whatever
they encode, so the fp16 library serves both 16-bit types; the padding's bit pattern is an argument.  TEST INFRASTRUCTURE ONLY.

Matrices are numpy uint16.  `offset` (in elements) places the caller-side matrix that far into a 16-byte aligned buffer, so that the
kernels' 2-byte paths run; every output lies between guard words that the calls check, so a store outside the matrix fails the call."""
import ctypes as C

import numpy as np

from emu import _p, available, lib  # noqa: F401

ONE = {False: 0x3C00, True: 0x3F80}  # 1.0 in fp16 / bf16
_GUARD, _GUARD_WORDS = 0xA5C3, 64


def _aligned(n_words, offset):
    """(buffer, view of n_words uint16 that starts `offset` elements behind a 16-byte boundary, with guard words on both sides)"""
    buf = np.full(n_words + 2 * _GUARD_WORDS + 16 + offset, _GUARD, dtype=np.uint16)
    start = (-(buf.ctypes.data // 2) % 8) + _GUARD_WORDS // 8 * 8 + offset
    return buf, buf[start:start + n_words], start


def _guards_intact(buf, start, n_words):
    return bool(np.all(buf[:start] == _GUARD) and np.all(buf[start + n_words:] == _GUARD))


def pad(x, padded, bf16=False, in_offset=0, out_offset=0):
    """x [n, n_dims] -> the feature-major matrix the network reads, as numpy [padded, n]"""
    n, d = x.shape
    _, src, _ = _aligned(n * d, in_offset)
    src[:] = x.reshape(-1)
    buf, dst, start = _aligned(padded * n, out_offset)
    assert lib(False).emuh_pad(C.c_uint32(n), C.c_uint32(d), C.c_uint32(padded), _p(src), _p(dst), C.c_uint32(ONE[bf16])) == 0
    assert _guards_intact(buf, start, padded * n), "half_input_pad wrote outside its output"
    return dst.reshape(padded, n).copy()


def unpad(dL_dy, n_dims, in_offset=0, out_offset=0):
    """dL_dy numpy [padded, n] (feature-major) -> dL_dx [n, n_dims]"""
    padded, n = dL_dy.shape
    _, src, _ = _aligned(padded * n, in_offset)
    src[:] = dL_dy.reshape(-1)
    buf, dst, start = _aligned(n * n_dims, out_offset)
    assert lib(False).emuh_unpad(C.c_uint32(n), C.c_uint32(n_dims), _p(src), _p(dst)) == 0
    assert _guards_intact(buf, start, n * n_dims), "half_input_unpad wrote outside its output"
    return dst.reshape(n, n_dims).copy()

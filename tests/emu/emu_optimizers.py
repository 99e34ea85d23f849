"""The emulated kernels of csrc/optimizer_kernels.hip (tests/emu/emu_driver_misc.cpp, emuo_*).  TEST INFRASTRUCTURE ONLY.

`Kernels(bf16)` offers the kernels under the names tests/optimizer_reference.py gives its numpy restatements, so that its optimizer
classes (the wrappers' host logic) can run on either.  Arrays are updated in place; 16-bit values are uint16."""
import ctypes as C

import numpy as np

from emu import _p, available, lib  # noqa: F401


def aligned_zeros(n, dtype):
    return _aligned(n, dtype)


def _aligned(n, dtype, offset_elems=0):
    """n elements whose first one lies `offset_elems` elements behind a 64-byte boundary (numpy alone promises 16 bytes at most)"""
    size = np.dtype(dtype).itemsize
    raw = np.zeros((n + offset_elems) * size + 64, np.uint8)
    start = (-raw.ctypes.data) % 64 + offset_elems * size
    return raw[start:start + n * size].view(dtype)


def aligned_copy(a, offset_elems=0):
    out = _aligned(a.size, a.dtype, offset_elems)
    out[:] = a.ravel()
    return out


def sgd_step(loss_scale, learning_rate, l2_reg, w32, w16, g16, begin=0, end=0xFFFFFFFF, bf16=False):
    assert lib(bf16).emuo_sgd_step(C.c_uint32(w32.size), C.c_float(loss_scale), C.c_float(learning_rate), C.c_float(l2_reg), _p(w32), _p(w16), _p(g16), C.c_uint32(begin),
                                   C.c_uint32(end)) == 0


def reduce_blocks(bf16=False):
    f = lib(bf16).emuo_novograd_reduce_blocks
    f.restype = C.c_uint32
    return int(f())


def novograd_step(begins, h, loss_scale, first_step, w32, w16, g16, m1, moments_in, bf16=False):
    """-> the layers' new second moments"""
    begins = np.ascontiguousarray(begins, np.uint32)
    n_layers = begins.size - 1
    hyper = np.array([h["learning_rate"], h["beta1"], h["beta2"], h["epsilon"], h["relative_decay"], h["absolute_decay"]], np.float32)
    moments_in = np.ascontiguousarray(moments_in, np.float32)
    out = np.zeros(n_layers, np.float32)
    partials = np.zeros(n_layers * reduce_blocks(bf16), np.float32)
    assert lib(bf16).emuo_novograd_step(C.c_uint32(n_layers), _p(begins), _p(hyper), C.c_float(loss_scale), C.c_int(int(first_step)), _p(w32), _p(w16), _p(g16), _p(m1),
                                        _p(moments_in), _p(out), _p(partials)) == 0
    return out


def lookahead_pull(alpha, w32, w16, slow16, bf16=False):
    assert lib(bf16).emuo_lookahead_step(C.c_uint32(w32.size), C.c_float(alpha), _p(w32), _p(w16), _p(slow16)) == 0


def average_step(n_samples, w16, sample16, average16, bf16=False):
    assert lib(bf16).emuo_average_step(C.c_uint32(w16.size), C.c_uint32(n_samples), _p(w16), _p(sample16), _p(average16)) == 0


def batched_accumulate(first, multiplier, g16, pool, bf16=False):
    assert lib(bf16).emuo_batched_accumulate(C.c_uint32(g16.size), C.c_int(int(first)), C.c_uint32(multiplier), _p(g16), _p(pool)) == 0


def batched_cast(pool, g16, bf16=False):
    assert lib(bf16).emuo_batched_cast(C.c_uint32(pool.size), _p(pool), _p(g16)) == 0


class Kernels:
    """the emulated kernels with the signatures of tests/optimizer_reference.py's numpy ones"""

    def __init__(self, bf16):
        self.bf16 = bf16

    def sgd_step(self, loss_scale, learning_rate, l2_reg, w32, w16, g16):
        sgd_step(loss_scale, learning_rate, l2_reg, w32, w16, g16, bf16=self.bf16)

    def lookahead_pull(self, alpha, w32, w16, slow16):
        lookahead_pull(alpha, w32, w16, slow16, bf16=self.bf16)

    def average_step(self, n_samples, w16, sample16, average16):
        average_step(n_samples, w16, sample16, average16, bf16=self.bf16)

    def batched_accumulate(self, first, multiplier, g16, pool):
        batched_accumulate(first, multiplier, g16, pool, bf16=self.bf16)

    def batched_cast(self, pool, g16):
        batched_cast(pool, g16, bf16=self.bf16)

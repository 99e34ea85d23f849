"""The emulated kernels of csrc/optimizer_kernels_f32.hip (tests/emu/emu_driver_optimizers_f32.cpp, emuf_*).  TEST INFRASTRUCTURE ONLY.

The driver is a part of its own, built here into a library of its own with emu.py's compile and link command lines.  `Kernels()` offers
the kernels under the names tests/optimizer_f32_reference.py gives its numpy restatements, so that its optimizer classes (the wrappers'
host logic) can run on either.  Arrays are float32 and updated in place."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import emu
from emu import EmuAdam, _p, available  # noqa: F401
from emu_optimizers import aligned_copy, aligned_zeros  # noqa: F401

_PART = os.path.join(emu._HERE, "emu_driver_optimizers_f32.cpp")
_LIB = os.path.join(emu._HERE, "libtcnn_emu_optimizers_f32.so")
_lib = None


def build(force=False):
    srcs = [os.path.join(emu._HERE, f) for f in os.listdir(emu._HERE) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(emu._CSRC, f) for f in os.listdir(emu._CSRC) if f.endswith((".hip", ".h"))]
    if not force and os.path.exists(_LIB) and os.path.getmtime(_LIB) >= max(os.path.getmtime(s) for s in srcs):
        return
    with tempfile.TemporaryDirectory(dir=emu._HERE) as tmp:
        obj = os.path.join(tmp, "emu_driver_optimizers_f32.o")
        subprocess.check_call(emu._COMPILE + [_PART, "-o", obj])
        subprocess.check_call(emu._LINK + [obj, "-o", _LIB])


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_LIB)
        _lib.emuf_novograd_reduce_blocks.restype = C.c_uint32
    return _lib


def _f(a):
    assert a.dtype == np.float32
    return _p(a)


def adam_step(oh, n_matrix, loss_scale, current_step, w, g, m1, m2, steps, begin=0, end=0xFFFFFFFF):
    """oh: oracle AdamHyper (the fields of emu.EmuAdam)"""
    e = EmuAdam(*[getattr(oh, f[0]) for f in EmuAdam._fields_])
    assert steps.dtype == np.uint32
    assert lib().emuf_adam_step(C.byref(e), C.c_uint32(w.size), C.c_uint32(n_matrix), C.c_float(loss_scale), C.c_uint32(current_step), _f(w), _f(g), _f(m1), _f(m2), _p(steps),
                                C.c_uint32(begin), C.c_uint32(end)) == 0


def sgd_step(loss_scale, learning_rate, l2_reg, w, g, begin=0, end=0xFFFFFFFF):
    assert lib().emuf_sgd_step(C.c_uint32(w.size), C.c_float(loss_scale), C.c_float(learning_rate), C.c_float(l2_reg), _f(w), _f(g), C.c_uint32(begin), C.c_uint32(end)) == 0


def novograd_step(begins, h, loss_scale, first_step, w, g, m1, moments_in):
    """-> the layers' new second moments"""
    begins = np.ascontiguousarray(begins, np.uint32)
    n_layers = begins.size - 1
    hyper = np.array([h["learning_rate"], h["beta1"], h["beta2"], h["epsilon"], h["relative_decay"], h["absolute_decay"]], np.float32)
    moments_in = np.ascontiguousarray(moments_in, np.float32)
    out = np.zeros(n_layers, np.float32)
    partials = np.zeros(n_layers * int(lib().emuf_novograd_reduce_blocks()), np.float32)
    assert lib().emuf_novograd_step(C.c_uint32(n_layers), _p(begins), _p(hyper), C.c_float(loss_scale), C.c_int(int(first_step)), _f(w), _f(g), _f(m1), _p(moments_in), _p(out),
                                    _p(partials)) == 0
    return out


def ema_step(decay, current_step, w, ema):
    assert lib().emuf_ema_step(C.c_uint32(w.size), C.c_float(decay), C.c_uint32(current_step), _f(w), _f(ema)) == 0


def lookahead_pull(alpha, w, slow):
    assert lib().emuf_lookahead_step(C.c_uint32(w.size), C.c_float(alpha), _f(w), _f(slow)) == 0


def average_step(n_samples, w, sample, average):
    assert lib().emuf_average_step(C.c_uint32(w.size), C.c_uint32(n_samples), _f(w), _f(sample), _f(average)) == 0


def batched_accumulate(first, multiplier, g, pool):
    assert lib().emuf_batched_accumulate(C.c_uint32(g.size), C.c_int(int(first)), C.c_uint32(multiplier), _f(g), _f(pool)) == 0


def batched_cast(pool, g):
    assert lib().emuf_batched_cast(C.c_uint32(pool.size), _f(pool), _f(g)) == 0


def loss(loss_type, prediction, target, dims, loss_scale=128.0, data_pdf=None):
    """the fp32 kernel -> (values [n][stride], gradients [n][stride] float32); outputs pre-filled with garbage"""
    prediction = aligned_copy(np.ascontiguousarray(prediction, np.float32)).reshape(prediction.shape)
    n, stride = prediction.shape
    values, grads = aligned_zeros(n * stride, np.float32).reshape(n, stride), aligned_zeros(n * stride, np.float32).reshape(n, stride)
    values[:], grads[:] = np.nan, np.nan
    assert lib().emuf_loss(C.c_int(loss_type), C.c_uint32(n), C.c_uint32(stride), C.c_uint32(dims), C.c_float(loss_scale), _p(prediction),
                           _p(np.ascontiguousarray(target, np.float32)), _p(None if data_pdf is None else np.ascontiguousarray(data_pdf, np.float32)), _p(values), _p(grads)) == 0
    return values, grads


def loss_half(loss_type, prediction_h, target, dims, loss_scale=128.0, data_pdf=None):
    """the 16-bit (fp16) kernel on bit patterns -> (values float32, gradients uint16)"""
    prediction_h = aligned_copy(np.ascontiguousarray(prediction_h, np.uint16)).reshape(prediction_h.shape)
    n, stride = prediction_h.shape
    values, grads = aligned_zeros(n * stride, np.float32).reshape(n, stride), aligned_zeros(n * stride, np.uint16).reshape(n, stride)
    assert lib().emuf_loss_half(C.c_int(loss_type), C.c_uint32(n), C.c_uint32(stride), C.c_uint32(dims), C.c_float(loss_scale), _p(prediction_h),
                                _p(np.ascontiguousarray(target, np.float32)), _p(None if data_pdf is None else np.ascontiguousarray(data_pdf, np.float32)), _p(values), _p(grads)) == 0
    return values, grads


class Kernels:
    """the emulated kernels with the signatures of tests/optimizer_f32_reference.py's numpy ones"""
    sgd_step = staticmethod(lambda loss_scale, learning_rate, l2_reg, w, g: sgd_step(loss_scale, learning_rate, l2_reg, w, g))
    lookahead_pull = staticmethod(lookahead_pull)
    average_step = staticmethod(average_step)
    batched_accumulate = staticmethod(batched_accumulate)
    batched_cast = staticmethod(batched_cast)
    ema_step = staticmethod(ema_step)

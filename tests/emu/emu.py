"""numpy front-end for the host SIMT emulator build of the gfx950 kernel sources (tests/emu/hip_emu.h).

TEST INFRASTRUCTURE ONLY.  Lets `pytest -m "not gpu"` run the real kernel code (indexing, MFMA fragment
bookkeeping, LDS tiles, barriers) on a machine without a GPU and compare it with the CPU oracle.

This module is the one builder and the one loader of the emulator's libraries: build(), available(), lib(bf16), lib_keep(bf16).  The
feature modules next to it (emu_max_level, emu_zero_records, ...) hold numpy front-ends only and call lib().  A new entry point goes into
the driver part that includes its kernels (emu_driver.h lists the parts) and its front-end here or into such a module.
"""
import ctypes as C
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "tiny-cuda-nn_amd", "csrc")
_CLANG = "/opt/rocm/lib/llvm/bin/clang++"
# The driver's parts (emu_driver.h says what goes where), heaviest first.  Each is compiled to an object of its own, side by side.
_PARTS = ("emu_driver_grid.cpp", "emu_driver_mlp.cpp", "emu_driver_misc.cpp", "emu_driver_half_input.cpp")
# The libraries, one per real build variant: (keep, bf16) -> (file, parts, defines).  IEEE fp16 as libtcnn_hip.so or -DTCNN_BF16 as
# libtcnn_hip_bf16.so; the "keep" pair is the grid part alone with the test-only switch -DTCNN_TEST_KEEP_ZERO_RECORDS.
_VARIANTS = {(keep, bf16): (os.path.join(_HERE, "libtcnn_emu%s%s.so" % ("_keep" if keep else "", "_bf16" if bf16 else "")),
                            _PARTS[:1] if keep else _PARTS,
                            (["-DTCNN_TEST_KEEP_ZERO_RECORDS"] if keep else []) + (["-DTCNN_BF16"] if bf16 else []))
             for keep in (False, True) for bf16 in (False, True)}
# All libraries define the same functions and the emulator keeps global state (::emu::g, an inline variable: one instance per library).
# Everything is compiled with hidden visibility except the driver's extern "C" entry points, and linked with -Bsymbolic: no library
# exports its state or can bind to another's, so all can live in one process (ctypes loads them RTLD_LOCAL).
_COMPILE = [_CLANG, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "-Wno-pass-failed",
            "-DTCNN_MLP_WAVE_BLOCKS=3",  # few workgroups: the persistent strip loop runs uneven shares
            "-I" + _HERE, "-I" + _CSRC, "-c"]
_LINK = [_CLANG, "-shared", "-fPIC", "-Wl,-Bsymbolic"]
_MAX_JOBS = 16


def build(force=False):
    """Builds every emulator library that is missing or older than one of its sources (the driver, hip_emu.h, csrc/*.hip, csrc/*.h)."""
    srcs = [os.path.join(_HERE, f) for f in os.listdir(_HERE) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))]
    newest = max(os.path.getmtime(s) for s in srcs)
    stale = [v for v in _VARIANTS.values() if force or not os.path.exists(v[0]) or os.path.getmtime(v[0]) < newest]
    if not stale:
        return
    with tempfile.TemporaryDirectory(dir=_HERE) as tmp:
        compiles, links = [], []
        for path, parts, defines in stale:
            objects = [os.path.join(tmp, "%s.%s.o" % (os.path.basename(path), part)) for part in parts]
            compiles += [(_PARTS.index(part), _COMPILE + defines + [os.path.join(_HERE, part), "-o", o]) for part, o in zip(parts, objects)]
            links.append(_LINK + objects + ["-o", path])
        with ThreadPoolExecutor(min(_MAX_JOBS, os.cpu_count() or 1)) as pool:  # (list(): a failed command raises here)
            list(pool.map(subprocess.check_call, [c for _, c in sorted(compiles, key=lambda c: c[0])]))
            list(pool.map(subprocess.check_call, links))


def available():
    return os.path.exists(_CLANG)


class EmuGrid(C.Structure):
    _fields_ = [("n_dims", C.c_uint32), ("n_levels", C.c_uint32), ("n_feat", C.c_uint32), ("grid_type", C.c_uint32),
                ("interp", C.c_uint32), ("max_level", C.c_float), ("offset", C.c_void_p), ("scale", C.c_void_p),
                ("resolution", C.c_void_p)]


class EmuMlp(C.Structure):
    _fields_ = [("in_width", C.c_uint32), ("width", C.c_uint32), ("padded_out", C.c_uint32),
                ("n_hidden_matmuls", C.c_uint32), ("activation", C.c_uint32), ("output_activation", C.c_uint32)]


class EmuAdam(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("learning_rate", "beta1", "beta2", "epsilon", "l2_reg", "non_matrix_l2_reg",
                                         "relative_weight_decay", "absolute_weight_decay", "weight_clipping_magnitude",
                                         "gradient_clipping_magnitude", "non_matrix_learning_rate_factor")] + \
               [(k, C.c_int) for k in ("adabound", "optimize_matrix_params", "optimize_non_matrix_params",
                                       "skip_zero_grad_non_matrix_params")]


_libs = {}
_bf16 = False


def set_bf16(on):
    """Selects the library the functions of this module call from here on: the bfloat16 build (True) or the fp16 one (False, the default).
    Returns the previous choice.  A module that tests the bf16 build switches in a module-scoped fixture and restores on the way out."""
    global _bf16
    previous, _bf16 = _bf16, bool(on)
    return previous


def _load(keep, bf16):
    key = (bool(keep), bool(bf16))
    if key not in _libs:
        build()
        _libs[key] = C.CDLL(_VARIANTS[key][0])
        assert _libs[key].emuzr_keeps_zero_records() == int(key[0])
        if not key[0]:  # (the fp32 network's entry points that do not return int: emu_mlp_f32.py)
            _libs[key].emuf32_saved_activation_floats.restype = C.c_uint64
            _libs[key].emuf32_n_partials.restype = C.c_uint32
    return _libs[key]


def lib(bf16=None):
    """The library: the bfloat16 build (True), the fp16 one (False), or whichever set_bf16 chose (None)."""
    return _load(False, _bf16 if bf16 is None else bf16)


def lib_keep(bf16):
    """The grid part built with -DTCNN_TEST_KEEP_ZERO_RECORDS."""
    return _load(True, bf16)


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class Grid:
    """Wraps an oracle grid description (oracle.Grid) for the emulated kernels."""

    def __init__(self, og, max_level=1.0, stochastic_interpolation=False):
        self.og = og
        L = og.n_levels
        self._off = np.array(og.offsets[: L + 1], dtype=np.uint32)
        self._scale = np.array(og.scale[:L], dtype=np.float32)
        self._res = np.array(og.resolution[:L], dtype=np.uint32)
        # bit 8 of the interpolation word carries stochastic_interpolation to the driver (GridMeta::stochastic)
        self.c = EmuGrid(og.n_dims, L, og.n_features_per_level, og.grid_type, og.interpolation | (0x100 if stochastic_interpolation else 0), max_level,
                         self._off.ctypes.data, self._scale.ctypes.data, self._res.ctypes.data)


# In the grid functions `max_level` is a float32 array with one entry per sample (GridIO::max_level) or None (g's scalar holds), and
# `bf16` chooses the library as lib() does.  Outputs are pre-filled with garbage: every element must be written.
def _ml(max_level, n):
    if max_level is None:
        return None
    max_level = np.ascontiguousarray(max_level, dtype=np.float32)
    assert max_level.shape == (n,)
    return max_level


def grid_forward(g, params_h, positions, soa=True, out_stride=None, want_dy_dx=False, max_level=None, bf16=None):
    """-> features, feature-major [L*F][n] (soa) or sample-major [n][out_stride], and dy_dx [L*F][n][D] if asked for.  Without dy_dx the
    tiled gather runs, with it the reference-form kernel."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n = positions.shape[0]
    k = og.n_levels * og.n_features_per_level
    stride = n if soa else (out_stride or k)
    out = np.full((k, n) if soa else (n, stride), 0x7E00, dtype=np.uint16)
    dy_dx = np.full((k, n, og.n_dims), np.nan, dtype=np.float32) if want_dy_dx else None
    assert lib(bf16).emu_grid_forward(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), C.c_uint32(n), _p(np.ascontiguousarray(params_h, dtype=np.uint16)), _p(out),
                                      C.c_int(int(soa)), C.c_uint32(stride), _p(dy_dx)) == 0
    return (out, dy_dx) if want_dy_dx else out


def grid_forward_plan(g, n, tile_samples=512):
    """The tiled gather's work plan: (tiles per level, [[(level, tile_begin, tile_end), ...] for each of the 8 XCDs])."""
    max_segments = 32
    n_seg = np.zeros(8, dtype=np.uint32)
    out = np.zeros((8, max_segments, 3), dtype=np.uint32)
    fn = lib().emu_grid_forward_plan
    fn.restype = C.c_uint32
    tiles = fn(C.byref(g.c), C.c_uint32(n), C.c_uint32(tile_samples), _p(n_seg), _p(out), C.c_uint32(max_segments))
    assert tiles > 0
    return int(tiles), [[tuple(int(v) for v in out[x, k]) for k in range(int(n_seg[x]))] for x in range(8)]


def grid_forward_f32(g, params, positions, out_stride=None, want_dy_dx=False, max_level=None, bf16=None):
    """k_grid_forward_f32: fp32 parameters -> fp32 features [n][out_stride] (+ dy_dx [k][n][D])."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=np.float32)
    n = positions.shape[0]
    k = og.n_levels * og.n_features_per_level
    stride = out_stride or k
    out = np.full((n, stride), np.nan, dtype=np.float32)
    dy_dx = np.full((k, n, og.n_dims), np.nan, dtype=np.float32) if want_dy_dx else None
    assert lib(bf16).emu_grid_forward_f32(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), C.c_uint32(n), _p(params), _p(out), C.c_uint32(stride), _p(dy_dx)) == 0
    return (out, dy_dx) if want_dy_dx else out


def grid_backward_f32(g, positions, dL_dy, accumulate_into=None, max_level=None, bf16=None):
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    dL_dy = np.ascontiguousarray(dL_dy, dtype=np.float32)
    n = positions.shape[0]
    grad = np.full(og.n_params, 7.0, dtype=np.float32) if accumulate_into is None else accumulate_into  # overwrite mode must clear what is there
    assert lib(bf16).emu_grid_backward_f32(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), C.c_uint32(n), _p(dL_dy), C.c_uint32(dL_dy.shape[1]), _p(grad),
                                           C.c_int(int(accumulate_into is not None))) == 0
    return grad


def grid_backward_input_f32(g, dL_dy, dy_dx):
    og = g.og
    dL_dy = np.ascontiguousarray(dL_dy, dtype=np.float32)
    n = dL_dy.shape[0]
    out = np.zeros((n, og.n_dims), dtype=np.float32)
    assert lib().emu_grid_backward_input_f32(C.byref(g.c), C.c_uint32(n), _p(dL_dy), C.c_uint32(dL_dy.shape[1]), _p(dy_dx), _p(out)) == 0
    return out


SLICED_F32, SLICED_F16, ATOMIC, BUCKETED = 0, 1, 2, 3


OWNER_PACKED, OWNER_FIXED64, OWNER_WIDE = 0, 1, 2


def grid_owner_stats():
    """(slices finished from the packed table, slices redone with 64 bits per value) since the last call."""
    v = (C.c_ulong * 2)()
    lib().emu_grid_owner_stats(v)
    return int(v[0]), int(v[1])


def grid_backward(g, positions, dL_dy_h, soa=True, mode=SLICED_F32, lds_budget=0, grad_init=None, owner=OWNER_PACKED, max_level=None, bf16=None):
    """owner: accumulator form of the bucket owners (grid_kernels.h grid_owner_mode), set for this call.  grad_init: half bit patterns to accumulate into
    (GradientMode::Accumulate); None -> Overwrite into a buffer pre-filled with garbage (the kernel must not rely on a zeroed gradient buffer)."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n = positions.shape[0]
    dL_dy_h = np.ascontiguousarray(dL_dy_h, dtype=np.uint16)
    grad_h = np.full(og.n_params, 0x3C00, dtype=np.uint16) if grad_init is None else grad_init.copy()
    stride = dL_dy_h.shape[1] if not soa else n
    assert lib(bf16).emu_grid_backward(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), C.c_uint32(n), _p(dL_dy_h), C.c_int(int(soa)), C.c_uint32(stride), _p(grad_h),
                                       C.c_int(int(grad_init is not None)), C.c_int(mode), C.c_uint32(lds_budget), C.c_int(int(owner))) == 0
    return grad_h


def grid_backward_backward(g, positions, ddx, dL_dy_soa_h, params_h, dy_dx_kn, want_params=True, want_input=True, max_level=None, bf16=None):
    """Second-order pass.  dL_dy / dL_ddLdy feature-major [K][n]; dy_dx in the kernels' [K][n][D] layout, or None: no dL_ddLdy.
    Returns (grad_half, dL_ddLdy, dL_dx), each None where not asked for."""
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    ddx = np.ascontiguousarray(ddx, dtype=np.float32)
    n = positions.shape[0]
    dy = np.ascontiguousarray(dL_dy_soa_h, dtype=np.uint16)
    grad = np.full(og.n_params, 0x3C00, dtype=np.uint16) if want_params else None
    dLddy = np.full_like(dy, 0x7E00) if dy_dx_kn is not None else None
    dx = np.full((n, og.n_dims), 7.0, dtype=np.float32) if want_input else None
    assert lib(bf16).emu_grid_backward_backward(C.byref(g.c), _p(_ml(max_level, n)), _p(positions), _p(ddx), C.c_uint32(n), _p(dy), _p(np.ascontiguousarray(params_h, dtype=np.uint16)),
                                                _p(None if dy_dx_kn is None else np.ascontiguousarray(dy_dx_kn, dtype=np.float32)), _p(grad), _p(dLddy), _p(dx)) == 0
    return grad, dLddy, dx


PLAN_FIXED64, PLAN_FLOAT, PLAN_GLOBAL_ATOMIC, PLAN_BUCKET = 0, 1, 2, 3


def grid_backward_plan(g, n, mode=BUCKETED, accumulate=False, lds_budget=0):
    """The host plan of a backward call (make_backward_plan, host code of the library): per level (kind, table slices, sample chunks
    per slice), kind one of PLAN_*.  Mode ATOMIC has no plan (every record is a global atomic)."""
    out = np.zeros((g.og.n_levels, 3), dtype=np.uint32)
    assert lib().emu_grid_backward_plan(C.byref(g.c), C.c_uint32(n), C.c_int(mode), C.c_int(int(accumulate)), C.c_uint32(lds_budget), _p(out)) == 0
    return out


def level_sum_units(total):
    """level_sum_units() of grid_backward_plan.h: a workgroup's fp32 total of clamped |record| -> 2^-32 units in 64 bits"""
    fn = lib().emu_level_sum_units
    fn.restype = C.c_uint64
    return int(fn(C.c_float(total)))


def saturating_add_u64(a, b):
    fn = lib().emu_saturating_add_u64
    fn.restype = C.c_uint64
    return int(fn(C.c_uint64(a), C.c_uint64(b)))


def atomic_add_h2(a_bits, b_bits):
    """a + b through the emulator's packed 16-bit atomic add, on arrays of bit patterns"""
    n = len(a_bits)
    a = np.zeros(n + (n & 1), dtype=np.uint16)
    b = np.zeros_like(a)
    a[:n], b[:n] = a_bits, b_bits
    lib().emu_atomic_add_h2(C.c_uint64(a.size), _p(a), _p(b))
    return a[:n]


def fma_h(a_bits, b_bits, c_bits):
    a, b, c = (np.ascontiguousarray(v, dtype=np.uint16) for v in (a_bits, b_bits, c_bits))
    out = np.zeros_like(a)
    lib().emu_fma_h(C.c_uint64(a.size), _p(a), _p(b), _p(c), _p(out))
    return out


def grid_backward_input(g, dL_dy_soa_h, dy_dx):
    og = g.og
    n = dL_dy_soa_h.shape[1]
    out = np.zeros((n, og.n_dims), dtype=np.float32)
    lib().emu_grid_backward_input(C.byref(g.c), C.c_uint32(n), _p(np.ascontiguousarray(dL_dy_soa_h)), C.c_int(1),
                                  C.c_uint32(n), _p(dy_dx), _p(out))
    return out


def grid_indices(g, positions):
    og = g.og
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n = positions.shape[0]
    idx = np.zeros((n, og.n_levels, 1 << og.n_dims), dtype=np.uint32)
    lib().emu_grid_indices(C.byref(g.c), _p(positions), C.c_uint32(n), _p(idx))
    return idx


def mlp_meta(om):
    """oracle.Mlp -> EmuMlp"""
    return EmuMlp(om.in_width, om.width, om.padded_out, om.n_hidden - 1, om.activation, om.output_activation)


def mlp_forward(om, params_h, input_soa_h, save_hidden=True):
    n = input_soa_h.shape[1]
    hidden = np.zeros((om.n_hidden, n, om.width), dtype=np.uint16) if save_hidden else None
    out = np.zeros((n, om.padded_out), dtype=np.uint16)
    m = mlp_meta(om)
    r = lib().emu_mlp_forward(C.byref(m), C.c_uint32(n), _p(params_h), _p(np.ascontiguousarray(input_soa_h)), _p(hidden), _p(out))
    assert r == 0
    return hidden, out


def mlp_backward(om, params_h, input_soa_h, hidden, dL_doutput_h, want_dinput=True, want_grads=True, grads_init=None, output=None):
    """dL_doutput_h: gradient w.r.t. the network output; `output` is needed when the output activation is not None."""
    n = input_soa_h.shape[1]
    dinput = np.zeros((om.in_width, n), dtype=np.uint16) if want_dinput else None
    grads = None
    if want_grads:
        grads = np.zeros(om.n_params, dtype=np.uint16) if grads_init is None else grads_init.copy()
    m = mlp_meta(om)
    r = lib().emu_mlp_backward(C.byref(m), C.c_uint32(n), _p(params_h), _p(np.ascontiguousarray(input_soa_h)), _p(hidden),
                               _p(np.ascontiguousarray(dL_doutput_h)), _p(dinput), _p(grads), C.c_int(int(grads_init is not None)),
                               _p(None if output is None else np.ascontiguousarray(output)))
    assert r == 0
    return grads, dinput


def mlp_train(om, params_h, input_soa_h, loss_type, target, dims, loss_scale=128.0, data_pdf=None, n_total=None, want_dinput=True,
              external_dL_doutput=None):
    """Fused forward + loss + backward (k_mlp_train).  Returns (output, dL_doutput, dL_dinput, grads, loss_sum) or None if unsupported.
    external_dL_doutput [n][16]: no loss, the backward half continues from the caller's gradient (target may be None)."""
    n = input_soa_h.shape[1]
    out = np.zeros((n, om.padded_out), dtype=np.uint16)
    dy = np.zeros((n, om.padded_out), dtype=np.uint16)
    dinput = np.zeros((om.in_width, n), dtype=np.uint16) if want_dinput else None
    grads = np.full(om.n_params, 0x3C00, dtype=np.uint16)
    s = np.zeros(1, dtype=np.float32)
    m = mlp_meta(om)
    r = lib().emu_mlp_train(C.byref(m), C.c_uint32(n), _p(params_h), _p(np.ascontiguousarray(input_soa_h)), C.c_int(loss_type),
                            _p(np.ascontiguousarray(target, dtype=np.float32) if target is not None else None), _p(data_pdf), C.c_uint32(dims),
                            C.c_float(loss_scale), C.c_uint32(n_total if n_total is not None else n * dims), _p(out), _p(dy), _p(dinput), _p(grads), _p(s),
                            _p(np.ascontiguousarray(external_dL_doutput) if external_dL_doutput is not None else None))
    if r == 2:
        return None
    assert r == 0
    return out, dy, dinput, grads, float(s[0])


def mlp_infer_f32_input(om, params_h, x, scale=1.0, offset=0.0, dims=None):
    """k_mlp_infer_wave reading an unpadded Identity encoding's fp32 input itself.  dims=None: the padded 16-bit output [n][16];
    otherwise the caller's fp32 matrix [n][dims].  None where no instance takes the shape."""
    x = np.require(x, dtype=np.float32, requirements=["C", "ALIGNED"])
    n = x.shape[0]
    out_h = np.zeros((n, om.padded_out), dtype=np.uint16) if dims is None else None
    out_f = np.zeros((n, dims), dtype=np.float32) if dims is not None else None
    m = mlp_meta(om)
    r = lib().emu_mlp_infer_f32_input(C.byref(m), C.c_uint32(n), _p(params_h), _p(x), C.c_float(scale), C.c_float(offset), _p(out_h), _p(out_f),
                                      C.c_uint32(dims or 0))
    if r == 2:
        return None
    assert r == 0
    return out_h if dims is None else out_f


def mlp_train_f32_input(om, params_h, x, scale, offset, loss_type, target, dims, loss_scale=128.0, data_pdf=None, n_total=None, want_dinput=True, want_enc=True):
    """mlp_train with the network kernel loading the fp32 sample-major input of an unpadded Identity encoding itself (MlpF32Input).
    Returns (output, dL_doutput, dL_dinput, grads, loss_sum, enc_out) or None where no instance offers it."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    out = np.zeros((n, om.padded_out), dtype=np.uint16)
    dy = np.zeros((n, om.padded_out), dtype=np.uint16)
    dinput = np.zeros((om.in_width, n), dtype=np.uint16) if want_dinput else None
    enc = np.full((om.in_width, n), 0x7E00, dtype=np.uint16) if want_enc else None
    grads = np.full(om.n_params, 0x3C00, dtype=np.uint16)
    s = np.zeros(1, dtype=np.float32)
    m = mlp_meta(om)
    r = lib().emu_mlp_train_f32_input(C.byref(m), C.c_uint32(n), _p(params_h), _p(x), C.c_float(scale), C.c_float(offset), C.c_int(loss_type),
                                      _p(np.ascontiguousarray(target, dtype=np.float32)), _p(data_pdf), C.c_uint32(dims), C.c_float(loss_scale),
                                      C.c_uint32(n_total if n_total is not None else n * dims), _p(out), _p(dy), _p(dinput), _p(grads), _p(s), _p(enc))
    if r == 2:
        return None
    assert r == 0
    return out, dy, dinput, grads, float(s[0]), enc


def loss(loss_type, prediction_h, target, dims, loss_scale=128.0, data_pdf=None, n_total=None):
    prediction_h = np.ascontiguousarray(prediction_h, dtype=np.uint16)
    n, stride = prediction_h.shape
    values = np.zeros((n, stride), dtype=np.float32)
    grads = np.zeros((n, stride), dtype=np.uint16)
    s = np.zeros(1, dtype=np.float32)
    lib().emu_loss(C.c_int(loss_type), C.c_uint32(n), C.c_uint32(stride), C.c_uint32(dims), C.c_float(loss_scale), _p(prediction_h),
                   _p(np.ascontiguousarray(target, dtype=np.float32)), _p(data_pdf), _p(values), _p(grads), _p(s),
                   C.c_uint32(n_total if n_total is not None else n * dims))
    return values, grads, float(s[0])


STEPS_COUNTERS, STEPS_DEFICITS32, STEPS_DEFICITS8 = 0, 1, 2  # elementwise_kernels.h AdamStepsForm


def adam_step(oh, n_matrix, loss_scale, current_step, w32, w16, grads_h, m1, m2, steps, steps_are_deficits=False, deficits8=None):
    """steps_are_deficits: False / True (32-bit deficits) or an AdamStepsForm; deficits8: the byte array of the byte form."""
    e = EmuAdam(*[getattr(oh, f[0]) for f in EmuAdam._fields_])
    lib().emu_adam_step(C.byref(e), C.c_uint32(w32.size), C.c_uint32(n_matrix), C.c_float(loss_scale), C.c_uint32(current_step),
                        _p(w32), _p(w16), _p(grads_h), _p(m1), _p(m2), _p(steps), C.c_int(int(steps_are_deficits)), _p(deficits8),
                        C.c_int(int(_adam_half_follows_master)))


_adam_half_follows_master = False


def set_adam_half_follows_master(on):
    """AdamCore::half_follows_master of the following adam_step calls: skipped parameters of a partly stepped lane get their 16-bit weight
    from the fp32 master weight instead of reading it back."""
    global _adam_half_follows_master
    _adam_half_follows_master = bool(on)


def adam_convert_steps(steps_done, steps, deficits8, form_from, form_to):
    """per-parameter step counters: any AdamStepsForm -> any other, in place"""
    lib().emu_adam_convert_steps(C.c_uint32(steps.size), C.c_uint32(steps_done), _p(steps), _p(deficits8), C.c_int(form_from), C.c_int(form_to))


def adam_flip_steps(steps_done, steps):
    """counters <-> deficits, in place"""
    lib().emu_adam_flip_steps(C.c_uint32(steps.size), C.c_uint32(steps_done), _p(steps))


def generate_random_uniform(rng, n, lower, upper):
    """rng: oracle.Pcg32 (state, inc) -- advanced in place like the device helper"""
    st, inc = C.c_uint64(rng.state), C.c_uint64(rng.inc)
    out = np.zeros(n, dtype=np.float32)
    lib().emu_generate_random_uniform(C.byref(st), C.byref(inc), C.c_uint64(n), _p(out), C.c_float(lower), C.c_float(upper))
    rng.state, rng.inc = st.value, inc.value
    return out


def cast_f32_to_f16(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(x.shape, dtype=np.uint16)
    lib().emu_cast_f32_to_f16(C.c_uint64(x.size), _p(x), _p(out))
    return out


def frequency_forward(x, n_frequencies, padded=None):
    """feature-major half [padded, n]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    padded = padded or x.shape[1] * n_frequencies * 2
    out = np.zeros((padded, x.shape[0]), dtype=np.uint16)
    lib().emu_frequency_forward(C.c_uint32(x.shape[0]), C.c_uint32(x.shape[1]), C.c_uint32(n_frequencies), C.c_uint32(padded), _p(x), _p(out))
    return out


def frequency_backward(x, n_frequencies, dL_dy_soa_h):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros_like(x)
    lib().emu_frequency_backward(C.c_uint32(x.shape[0]), C.c_uint32(x.shape[1]), C.c_uint32(n_frequencies), _p(np.ascontiguousarray(dL_dy_soa_h, dtype=np.uint16)), _p(x), _p(out))
    return out


def oneblob_forward(x, n_bins, padded=None):
    """feature-major half [padded, n]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    padded = padded or x.shape[1] * n_bins
    out = np.zeros((padded, x.shape[0]), dtype=np.uint16)
    lib().emu_oneblob_forward(C.c_uint32(x.shape[0]), C.c_uint32(x.shape[1]), C.c_uint32(n_bins), C.c_uint32(padded), _p(x), _p(out))
    return out


def oneblob_backward(x, n_bins, dL_dy_soa_h):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros_like(x)
    lib().emu_oneblob_backward(C.c_uint32(x.shape[0]), C.c_uint32(x.shape[1]), C.c_uint32(n_bins), _p(np.ascontiguousarray(dL_dy_soa_h, dtype=np.uint16)), _p(x), _p(out))
    return out


def identity_forward(x, padded):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros((padded, x.shape[0]), dtype=np.uint16)
    lib().emu_identity_forward(C.c_uint32(x.shape[0]), C.c_uint32(x.shape[1]), C.c_uint32(padded), _p(x), _p(out))
    return out

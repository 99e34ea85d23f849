"""The emulated grid kernels (tests/emu/emu.py) run with a per-sample max_level array, in the layouts tests/max_level_reference.py uses:
value matrices sample-major [n][L*F].  TEST INFRASTRUCTURE ONLY.

`g` is an emu.Grid (its scalar max_level travels in the struct); `max_level` a float32 array with one entry per sample, or None."""
import numpy as np

import emu
from emu import ATOMIC, BUCKETED, SLICED_F16, SLICED_F32, Grid, available  # noqa: F401  (re-exported for the tests)


def _soa(dL_dy_h):
    return np.ascontiguousarray(np.asarray(dL_dy_h, dtype=np.uint16).T)


def grid_forward(g, max_level, params_h, positions, soa=True, want_dy_dx=False, bf16=False):
    """-> features [n][L*F] (bit patterns), and dy_dx [L*F][n][D] if asked for.  `soa`: the kernel writes feature-major."""
    r = emu.grid_forward(g, params_h, positions, soa=soa, want_dy_dx=want_dy_dx, max_level=max_level, bf16=bf16)
    out, dy_dx = r if want_dy_dx else (r, None)
    out = np.ascontiguousarray(out.T) if soa else out
    return (out, dy_dx) if want_dy_dx else out


def grid_forward_f32(g, max_level, params, positions, want_dy_dx=False):
    return emu.grid_forward_f32(g, params, positions, want_dy_dx=want_dy_dx, max_level=max_level, bf16=False)


def grid_backward(g, max_level, positions, dL_dy_h, mode=BUCKETED, lds_budget=0):
    """dL_dy_h [n][L*F] bit patterns -> the grid gradient's bit patterns (Overwrite into a buffer pre-filled with garbage)."""
    return emu.grid_backward(g, positions, _soa(dL_dy_h), mode=mode, lds_budget=lds_budget, max_level=max_level, bf16=False)


def grid_backward_f32(g, max_level, positions, dL_dy):
    return emu.grid_backward_f32(g, positions, dL_dy, max_level=max_level, bf16=False)


def grid_backward_backward(g, max_level, positions, ddx, dL_dy_h, params_h, want_params=True, want_input=True):
    """Second order: (the parameter gradient's bit patterns or None, dL_dx [n][D] or None).  dL_dy_h [n][L*F] bit patterns."""
    grad, _, dx = emu.grid_backward_backward(g, positions, ddx, _soa(dL_dy_h), params_h, None, want_params=want_params, want_input=want_input, max_level=max_level, bf16=False)
    return grad, dx

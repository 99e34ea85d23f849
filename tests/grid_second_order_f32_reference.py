"""The second-order pass of an fp32 grid encoding (the reference's T = float instances of kernel_grid_backward_input_backward_grid,
_backward_input and _backward_dLdoutput, grid.h:352-655), restated in numpy for fp32 parameters and an fp32 dL_dy.  The oracle has no such
pass; what it does pin is taken from it: Grid.scale / resolution / offsets / n_features_per_level of oracle.grid_init and the corner indices
of oracle.grid_indices (bit d of a corner number selects the upper neighbour along d).

The position is formed in fp32 exactly as the kernels form it: pos = fmaf(scale, x, 0.5f) -- np.float32(np.float64(scale) * np.float64(x) +
0.5) is that fma for fp32 operands --, then floor and fraction (an exact fp32 subtraction).  The weights, smoothstep and its first and second
derivative are derived from that fp32 fraction, and everything after the fraction is float64.

With t_d the fraction along d, w_d = (1 - S(t_d), S(t_d)), S the interpolation function (the identity for Linear), s_d(c) = +1 for the
upper and -1 for the lower corner along d, and v(c) = sum_f grid[c][f] * dL_dy[f], per sample and level:
  dL_dparams[c][f] += scale * sum_d ddx[d] S'(t_d) s_d(c) prod_{e != d} w_e(c) * dL_dy[f]
  dL_dinput[a]     += scale^2 sum_c ( ddx[a] S''(t_a) s_a prod_{e != a} w_e v(c) + sum_{b != a} ddx[b] S'(t_b) S'(t_a) s_a s_b prod_{e != a, b} w_e v(c) )
  dL_ddLdoutput[k]  = sum_d dy_dx[k][d] * ddx[d]        (dy_dx: what the fp32 forward pass stored, an input here)
Nearest has no second order: every result is zero and no table entry is touched.

Magnitudes.  mag_p, mag_y and mag_x are the same sums with every term taken by its absolute value: |w_e|, |S'|, |S''| = |6 - 12t|, |ddx|,
|dL_dy|, |grid|.  Nothing is added to them.  (A kernel that forms 1 - S(t) or 6 - 12t by subtracting a rounded value does not stay within
a few 2^-24 of such a term when it is small; the fp32 kernels form them as S(1 - t) and 12 * (0.5 - t), see csrc/grid_device.h.)

cancel_p is NOT part of any magnitude and no bar of the fp32 kernels uses it: it is how far dL_dparams moves, in the worst case, when every
lower Smoothstep weight is off by the ABSOLUTE amount `lower_weight_abs_error` (zero, and cancel_p all zeros, unless asked for).  The CPU pin
against the oracle needs it: the oracle forms that weight as 1 - S(t) from an fp32 S(t).

second_order() returns a Result: dL_dparams [n_params], dL_ddLdoutput [n, L*F] (None without dy_dx), dL_dinput [n, D], the same sums taken
over absolute values (above) as mag_p, mag_y, mag_x, and hits [n_params], the
number of (sample, level, corner) contributions per table entry, repeated for its F features.  `off` is the [n, L] mask of
tests/max_level_reference.py::off_mask: an off (sample, level) pair contributes nothing (the mask is monotone, so this is also the position
kernel's break at the first off level), and dy_dx is taken as zero there."""
from collections import namedtuple

import numpy as np

from max_level_reference import feature_mask, off_mask  # noqa: F401  (off_mask: re-exported for the tests)
from oracle import oracle as O

Result = namedtuple("Result", "dL_dparams dL_ddLdoutput dL_dinput mag_p mag_y mag_x hits cancel_p")


def fractions(og, positions):
    """[n, L, D] float32: pos - floor(pos) with pos = fmaf(scale_l, x, 0.5f)"""
    x = np.asarray(positions, dtype=np.float32).astype(np.float64)
    scale = np.array([og.scale[l] for l in range(og.n_levels)], dtype=np.float32).astype(np.float64)
    pos = (scale[None, :, None] * x[:, None, :] + 0.5).astype(np.float32)
    frac = pos - np.floor(pos)
    assert frac.dtype == np.float32
    return frac


def second_order(og, params, positions, ddx, dL_dy, off=None, dy_dx=None, lower_weight_abs_error=0.0):
    params = np.asarray(params)
    dL_dy = np.asarray(dL_dy)
    ddx = np.asarray(ddx)
    assert params.dtype == np.float32 and dL_dy.dtype == np.float32 and ddx.dtype == np.float32
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    n, D = positions.shape
    L, F, C = og.n_levels, og.n_features_per_level, 1 << og.n_dims
    assert D == og.n_dims and dL_dy.shape[0] == n and dL_dy.shape[1] >= L * F
    if off is None:
        off = np.zeros((n, L), dtype=bool)
    dd = ddx.astype(np.float64)
    table = params.astype(np.float64).reshape(-1, F)

    grad = np.zeros((og.n_params // F, F))
    mag_p = np.zeros_like(grad)
    cancel_p = np.zeros_like(grad)
    hits = np.zeros(og.n_params // F, dtype=np.int64)
    dx = np.zeros((n, D))
    mag_x = np.zeros((n, D))

    dLddy = mag_y = None
    if dy_dx is not None:
        j = np.asarray(dy_dx)
        assert j.dtype == np.float32 and j.shape == (n, L * F, D)
        j = j.astype(np.float64)
        j[feature_mask(off, F)] = 0.0
        dLddy = (j * dd[:, None, :]).sum(axis=2)
        mag_y = (np.abs(j) * np.abs(dd)[:, None, :]).sum(axis=2)

    if og.interpolation == O.INTERP_NEAREST:
        return Result(grad.reshape(-1), dLddy, dx, mag_p.reshape(-1), mag_y, mag_x, np.repeat(hits, F), mag_p.reshape(-1).copy())

    smooth = og.interpolation == O.INTERP_SMOOTHSTEP
    idx = O.grid_indices(og, positions).astype(np.int64)  # [n, L, C]
    t_all = fractions(og, positions).astype(np.float64)
    bits = (np.arange(C)[:, None] >> np.arange(D)[None, :]) & 1  # [C, D]
    sign = np.where(bits == 1, 1.0, -1.0)
    for level in range(L):
        on = ~off[:, level]
        scale = np.float64(np.float32(og.scale[level]))
        t = t_all[:, level, :]
        if smooth:
            s, d1, d2 = t * t * (3.0 - 2.0 * t), 6.0 * t * (1.0 - t), 6.0 - 12.0 * t
        else:
            s, d1, d2 = t, np.ones_like(t), np.zeros_like(t)
        w = np.where(bits[None, :, :] == 1, s[:, None, :], 1.0 - s[:, None, :])  # [n, C, D]: w_d of corner c (>= 0)
        w_mag, d2_mag = w, np.abs(d2)  # (w >= 0)
        w_off = w + np.where(bits[None, :, :] == 0, lower_weight_abs_error, 0.0) if smooth else w  # cancel_p only

        def prod_except(skip, of=None):
            of = w if of is None else of
            keep = [e for e in range(D) if e not in skip]
            return np.prod(of[:, :, keep], axis=2) if keep else np.ones((n, C))

        dy = np.where(on[:, None], dL_dy[:, level * F:(level + 1) * F].astype(np.float64), 0.0)  # [n, F]
        entry = og.offsets[level] + idx[:, level, :]  # [n, C]
        values = table[entry]  # [n, C, F]
        v = (values * dy[:, None, :]).sum(axis=2)
        v_abs = (np.abs(values) * np.abs(dy)[:, None, :]).sum(axis=2)

        # parameters: one contribution per (sample, corner, feature)
        weight = np.zeros((n, C))
        weight_abs = np.zeros((n, C))
        weight_off = np.zeros((n, C))
        for d in range(D):
            factor = scale * dd[:, d, None] * d1[:, d, None]
            weight += sign[None, :, d] * factor * prod_except((d,))
            weight_abs += np.abs(factor) * prod_except((d,), w_mag)
            weight_off += np.abs(factor) * (prod_except((d,), w_off) - prod_except((d,), w_mag))
        np.add.at(grad, entry[on], weight[on][:, :, None] * dy[on][:, None, :])
        np.add.at(mag_p, entry[on], weight_abs[on][:, :, None] * np.abs(dy[on])[:, None, :])
        np.add.at(cancel_p, entry[on], weight_off[on][:, :, None] * np.abs(dy[on])[:, None, :])
        np.add.at(hits, entry[on], 1)

        # positions
        for a in range(D):
            acc = np.zeros(n)
            acc_abs = np.zeros(n)
            if smooth:
                factor = scale * scale * dd[:, a, None]
                acc += (sign[None, :, a] * factor * d2[:, a, None] * prod_except((a,)) * v).sum(axis=1)
                acc_abs += (np.abs(factor) * d2_mag[:, a, None] * prod_except((a,), w_mag) * v_abs).sum(axis=1)
            for b in range(D):
                if b == a:
                    continue
                factor = scale * scale * dd[:, b, None] * d1[:, b, None] * d1[:, a, None]
                acc += (sign[None, :, a] * sign[None, :, b] * factor * prod_except((a, b)) * v).sum(axis=1)
                acc_abs += (np.abs(factor) * prod_except((a, b), w_mag) * v_abs).sum(axis=1)
            dx[:, a] += acc
            mag_x[:, a] += acc_abs
    return Result(grad.reshape(-1), dLddy, dx, mag_p.reshape(-1), mag_y, mag_x, np.repeat(hits, F), cancel_p.reshape(-1))

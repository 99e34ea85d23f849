"""Expected values of the grid encoding under max_level (MultiLevelEncoding::set_max_level / set_max_level_gpu), from the oracle, which has
no max_level of its own: per level, the encoding of a sample does not depend on the other levels, so the expected output is the oracle's
with the off (sample, level) blocks zeroed, and the expected gradients are the oracle's on a dL_dy whose off blocks are zeroed (adding
zeros is exact in every accumulation the oracle makes).  The off levels of a sample are always its upper ones (a monotone mask), so the
second-order position kernel's break at the first off level is the same mask.

The mask is the reference's fp32 expression (grid.h:70-75): t = (m * (L * F)) / F, level l off when l >= t + 1e-3f in the forward pass and
when l > t + 1e-3f in the backward passes.  MARGIN: both comparisons, and any rounding of the fp32 expression (under 1e-6 for L <= 32), give
the same answer while t + 1e-3 stays away from every integer l.  The values the tests use are m = k / L with small integers k and L, for
which t is the integer k exactly and the distance is 1e-3 -- the largest such values can have; a margin of 1e-2 would rule all of them
out, m = 0.5 and m = 1.0 included.  off_mask() therefore asserts half of that, 5e-4 (500 times the rounding), for them, and the full 1e-2
for the one case whose t is no integer (m = 0.3: t = 2.4 with 8 levels, 1.2 with 4): a violation fails the test."""
import numpy as np

from oracle import oracle as O

MARGIN = 5e-4


def off_mask(max_level, n, n_levels, n_feat, margin=MARGIN):
    """[n, L] bool: level l is off for sample i.  max_level: a scalar or one value per sample.  margin: the least distance of t + 1e-3 from
    every level that is asserted -- 1e-2 for the cases whose t is no integer (m = 0.3)."""
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(max_level, dtype=np.float32), (n,)))
    t = (m * np.float32(n_levels * n_feat)) / np.float32(n_feat)
    assert t.dtype == np.float32
    threshold = t + np.float32(1e-3)
    levels = np.arange(n_levels, dtype=np.float32)
    assert np.all(np.abs(levels[None, :].astype(np.float64) - threshold[:, None].astype(np.float64)) >= margin), "max_level too close to a level's threshold"
    forward = levels[None, :] >= threshold[:, None]
    backward = levels[None, :] > threshold[:, None]
    assert np.array_equal(forward, backward)
    assert np.all(forward[:, 1:] >= forward[:, :-1])  # monotone: once off, off for every finer level
    return forward


def feature_mask(off, n_feat, width=None):
    """[n, width] bool from the [n, L] level mask: the features of off levels; columns beyond L * F (padding) are never off."""
    f = np.repeat(off, n_feat, axis=1)
    if width is not None and width > f.shape[1]:
        f = np.concatenate([f, np.zeros((f.shape[0], width - f.shape[1]), dtype=bool)], axis=1)
    return f


def masked(values, fmask):
    """a copy of `values` [n, width] (any dtype, bit patterns included: zero is all bits clear) with the off features zeroed"""
    out = np.array(values, copy=True)
    out[fmask[:, : out.shape[1]]] = 0
    return out


def forward(og, params_h, positions, off, out_stride=None):
    """-> (features [n, stride] bit patterns, dy_dx [n, L*F, D]) of the 16-bit encoding with the off blocks zeroed"""
    y, dy_dx = O.grid_forward(og, params_h, positions, out_stride=out_stride, want_dy_dx=True)
    f = feature_mask(off, og.n_features_per_level)
    y = masked(y, f)
    dy_dx = dy_dx.copy()
    dy_dx[f] = 0.0
    return y, dy_dx


def forward_f32(og, params, positions, off):
    y, dy_dx = O.grid_forward_f32(og, params, positions, want_dy_dx=True)
    f = feature_mask(off, og.n_features_per_level)
    y = masked(y, f)
    dy_dx = dy_dx.copy()
    dy_dx[f] = 0.0
    return y, dy_dx


def backward(og, positions, dL_dy_h, off):
    """-> (grid gradient float64, the same scatter of |dL_dy|: the magnitude the tolerances of tests/test_gpu_parity.py scale with)"""
    dy = masked(dL_dy_h, feature_mask(off, og.n_features_per_level, dL_dy_h.shape[1]))
    return O.grid_backward(og, positions, dy), O.grid_backward(og, positions, O.f2h(np.abs(O.h2f(dy))))


def backward_f32(og, positions, dL_dy, off):
    dy = masked(np.asarray(dL_dy, dtype=np.float32), feature_mask(off, og.n_features_per_level, dL_dy.shape[1]))
    return O.grid_backward_f32(og, positions, dy), O.grid_backward_f32(og, positions, np.abs(dy))


def backward_backward(og, params_h, positions, ddx, dL_dy_h, off, dy_dx=None):
    """Second order on masked inputs -> (grid gradient float64, its magnitude, dL_ddLdy bit patterns or None, dL_dx [n, D]).
    The mask is monotone, so zeroing dL_dy's off blocks is the position kernel's break at the first off level."""
    dy = masked(dL_dy_h, feature_mask(off, og.n_features_per_level, dL_dy_h.shape[1]))
    grad, dLddy, dx = O.grid_backward_backward_input(og, params_h, positions, ddx, dy, dy_dx=dy_dx)
    mag = np.abs(O.grid_backward_backward_input(og, params_h, positions, np.abs(ddx), O.f2h(np.abs(O.h2f(dy))))[0]) + np.abs(grad)
    return grad, mag, dLddy, dx

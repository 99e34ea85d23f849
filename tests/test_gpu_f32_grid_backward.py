"""The owner pass of fp32 grid encodings (csrc/grid_backward_f32.hip) against the oracle's float64 sums of the fp32 terms.

Grids, per (D, F), with the slices of at most 8192 / F entries the plan cuts (csrc/grid_backward_plan.h make_f32_backward_plan):
  (2, 1) base 64, 3 levels, T = 2^15: 4096 dense entries (1 slice), 16384 dense (2 slices), 32768 hashed (4 slices)
  (3, 2) base 4, 4 levels, T = 2^14:  64, 512, 4096 dense (1 slice each), 16384 hashed (4 slices)
  (3, 4) the same grid:               64, 512 (1 slice each), 4096 dense (2 slices), 16384 hashed (8 slices)
  (4, 8) base 4, 3 levels, T = 2^14:  256 dense (1 slice), 4096 dense (4 slices), 16384 hashed (16 slices)
Batches 256 and 768 (half a scatter tile / one and a half at D = 3) leave every level at the largest slice; 4352 is the first batch past
4096, where the 8 * n records of a level at D = 3 pass 32768 and the plan cuts every table finer, into twice the slices (also level 0's 64
entries).

The bar per entry: (hits + 30) * 2^-24 * sum|terms| -- DESIGN.md section 5's bar for the fp32 scatter -- plus hits * q_l, the quantisation:
the kernel's quantum of a value is never coarser than q_l = 2^(e_l + ceil(log2 n) + D - 62), 2^(e_l - 1) <= max |dL_dy| < 2^e_l over the
level, computed here from the rule."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu
GRIDS = {(2, 1): (3, 15, 64), (3, 2): (4, 14, 4), (3, 4): (4, 14, 4), (4, 8): (3, 14, 4)}  # (D, F) -> levels, log2_hashmap_size, base
INTERP = {"Linear": O.INTERP_LINEAR, "Smoothstep": O.INTERP_SMOOTHSTEP}


def _C():
    import tinycudann
    return tinycudann._C


def make(d, f, interpolation="Linear"):
    levels, log2, base = GRIDS[(d, f)]
    cfg = {"otype": "HashGrid", "n_levels": levels, "n_features_per_level": f, "log2_hashmap_size": log2, "base_resolution": base, "per_level_scale": 2.0,
           "interpolation": interpolation}
    return _C().create_encoding(d, cfg, _C().Precision.Fp32), O.grid_init(d, levels, f, log2, base, 2.0, O.GRID_HASH, INTERP[interpolation])


def data(og, n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, og.n_dims), dtype=np.float32), rng.standard_normal((n, og.n_levels * og.n_features_per_level)).astype(np.float32)


def gradient(m, x_np, dy_np, into=None):
    """Overwrite, or Accumulate into a copy of `into` -> dL_dparams on the host"""
    x, dy = torch.from_numpy(x_np).cuda(), torch.from_numpy(dy_np).cuda()
    p = torch.zeros(m.n_params(), device="cuda").requires_grad_(True)
    ctx, y = m.fwd(x, p)
    if into is None:
        return m.bwd(ctx, x, p, y, dy)[1].cpu().numpy()
    dp = torch.from_numpy(into).cuda()
    m.bwd_into(ctx, x, p, y, dy, dp, gradient_mode=_C().GradientMode.Accumulate, want_dL_dinput=False)
    return dp.cpu().numpy()


def reference(og, x, dy, on=None):
    """float64 sums, the bar's two terms per value; `on` [n][L]: the (sample, level) pairs that max_level leaves on"""
    n, L, F, D = x.shape[0], og.n_levels, og.n_features_per_level, og.n_dims
    on = np.ones((n, L), bool) if on is None else on
    live = dy * np.repeat(on, F, axis=1)
    ref, mag = O.grid_backward_f32(og, x, live), O.grid_backward_f32(og, x, np.abs(live))
    idx = O.grid_indices(og, x)
    hits, q = np.zeros(og.n_params // F), np.zeros(og.n_params // F)
    for l in range(L):
        np.add.at(hits, og.offsets[l] + idx[on[:, l], l, :].reshape(-1), 1)
        level_max = np.abs(dy[:, l * F:(l + 1) * F]).max()  # over every sample of the batch
        if level_max > 0:
            q[og.offsets[l]:og.offsets[l + 1]] = 2.0 ** (math.frexp(level_max)[1] + math.ceil(math.log2(n)) + D - 62)
    hits, q = np.repeat(hits, F), np.repeat(q, F)
    return ref, (hits + 30) * 2.0 ** -24 * mag, hits * q


@pytest.mark.parametrize("n", [256, 768, 4352])
@pytest.mark.parametrize("interpolation", list(INTERP))
@pytest.mark.parametrize("d,f", list(GRIDS))
def test_parity(d, f, interpolation, n):
    m, og = make(d, f, interpolation)
    assert m.fp32_grid_backward(n) == 1
    x, dy = data(og, n, seed=n + d + f)
    ref, rounding, quantum = reference(og, x, dy)
    got = gradient(m, x, dy)
    assert np.all(np.abs(got - ref) <= rounding + quantum), np.abs(got - ref).max()
    assert np.count_nonzero(got) > og.n_params // 50
    try:  # the control: the atomic kernel on the same inputs
        _C().set_fp32_grid_backward(False)
        assert m.fp32_grid_backward(n) == 0
        assert np.all(np.abs(gradient(m, x, dy) - ref) <= rounding + quantum)
    finally:
        _C().set_fp32_grid_backward(True)


@pytest.mark.parametrize("n", [768, 4352])
@pytest.mark.parametrize("d,f", [(3, 2), (4, 8)])
def test_the_order_of_the_samples_does_not_matter(d, f, n):
    m, og = make(d, f)
    x, dy = data(og, n, seed=n)
    got = gradient(m, x, dy)
    assert np.array_equal(got, gradient(m, x[::-1].copy(), dy[::-1].copy())) and np.array_equal(got, gradient(m, x, dy)) and got.any()
    stored = np.random.default_rng(1).standard_normal(og.n_params).astype(np.float32)
    for xs, dys in ((x, dy), (x[::-1].copy(), dy[::-1].copy())):
        assert np.array_equal(gradient(m, xs, dys, into=stored), stored + got)  # added once, in fp32


@pytest.mark.parametrize("power", [13, -20])
def test_the_quantum_follows_the_magnitude(power):
    m, og = make(3, 2)
    x, dy = data(og, 768, seed=5)
    assert np.array_equal(gradient(m, x, dy * np.float32(2.0 ** power)), gradient(m, x, dy) * np.float32(2.0 ** power))


def test_mixed_magnitudes():
    m, og = make(3, 2)
    x, dy = data(og, 768, seed=9)
    small = np.arange(768) % 2 == 1
    dy[small] *= np.float32(2.0 ** -30)
    ref, rounding, quantum = reference(og, x, dy)
    reached = O.grid_backward_f32(og, x, np.abs(dy) * ~small[:, None]) > 0  # by a large sample
    assert reached.any() and np.all(quantum[reached] < rounding[reached])
    assert np.all(np.abs(gradient(m, x, dy) - ref) <= rounding + quantum)


@pytest.mark.parametrize("per_sample", [False, True], ids=["scalar", "array"])
def test_max_level(per_sample):
    m, og = make(3, 2)
    n, L = 768, og.n_levels
    x, dy = data(og, n, seed=3)
    values = np.where(np.arange(n) % 3 == 0, 0.25, 0.5).astype(np.float32) if per_sample else np.full(n, 0.5, np.float32)  # level 3 off, level 2 for a third
    on = ~(np.arange(L, dtype=np.float32)[None, :] > (values[:, None] * np.float32(L * og.n_features_per_level)) / np.float32(og.n_features_per_level) + np.float32(1e-3))
    array = torch.from_numpy(values).cuda()
    try:
        m.set_max_level_gpu(array) if per_sample else m.set_max_level(0.5)
        got = gradient(m, x, dy)
    finally:
        m.set_max_level_gpu(None)
    ref, rounding, quantum = reference(og, x, dy, on)
    off_levels = [l for l in range(L) if not on[:, l].any()]
    assert off_levels and all(not got[og.offsets[l] * 2:og.offsets[l + 1] * 2].any() for l in off_levels)
    assert np.all(np.abs(got - ref) <= rounding + quantum) and got.any()

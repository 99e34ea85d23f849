"""The tiled forward gather of fp32 grid encodings (csrc/grid_forward_f32.hip), with and without dy_dx, bit for bit against the oracle's
fp32 restatement -- the bar tests/test_emu_kernels.py::test_grid_fp32_kernels holds the one-thread-per-(sample, level) kernel to.

The grids are tests/test_gpu_f32_grid_backward.py's (dense and hashed levels, tables of 64 to 32768 entries).  A workgroup's tile is 512
samples where a thread owns two -- (2, 1), (3, 2), (3, 4) -- and 256 at (4, 8): the batches 256, 768 and 1280 are half a tile, one and a
half and two and a half, or 1, 3 and 5 tiles, and with 3 or 4 levels the eight runs of the plan are cut inside levels.  The module surface
returns dL_dinput, not dy_dx: it is compared with the oracle's grid_backward_input_f32 of the oracle's dy_dx and a random dL_dy."""
import functools

import numpy as np
import pytest
import torch

import max_level_reference as R
from oracle import oracle as O
from test_gpu_f32_grid_backward import GRIDS

pytestmark = pytest.mark.gpu
INTERP = {"Linear": O.INTERP_LINEAR, "Smoothstep": O.INTERP_SMOOTHSTEP}
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def _C():
    import tinycudann
    return tinycudann._C


def make(d, f, interpolation="Linear", otype="HashGrid", levels=None, base=None, scale=2.0):
    n_levels, log2, base_resolution = GRIDS[(d, f)]
    levels, base = levels or n_levels, base or base_resolution
    cfg = {"otype": otype, "n_levels": levels, "n_features_per_level": f, "log2_hashmap_size": log2, "base_resolution": base, "per_level_scale": scale,
           "interpolation": interpolation}
    og = O.grid_init(d, levels, f, log2, base, scale, O.GRID_HASH if otype == "HashGrid" else O.GRID_DENSE, INTERP[interpolation])
    return cfg, _C().create_encoding(d, cfg, _C().Precision.Fp32), og


@functools.lru_cache(maxsize=None)
def case(d, f, interpolation, n, **grid):
    """-> module, oracle grid, positions (rows 0 and 1: exactly 0.0 and 1.0), parameters, dL_dy, the oracle's features and dy_dx"""
    _, m, og = make(d, f, interpolation, **grid)
    rng = np.random.default_rng(1000 * d + 100 * f + n)
    x = rng.random((n, d), dtype=np.float32)
    x[0], x[1] = 0.0, 1.0
    p = (rng.standard_normal(og.n_params) * 0.3).astype(np.float32)
    dy = rng.standard_normal((n, og.n_levels * f)).astype(np.float32)
    return (m, og, x, p, dy) + tuple(O.grid_forward_f32(og, p, x, want_dy_dx=True))


def run(m, x, p, dy=None):
    """features, and with a dL_dy the forward call that prepares dy_dx and the dL_dinput computed from it"""
    xt, pt = torch.from_numpy(x).cuda().requires_grad_(dy is not None), torch.from_numpy(p).cuda()
    ctx, y = m.fwd(xt, pt)
    return y.cpu().numpy(), None if dy is None else m.bwd(ctx, xt, pt, y, torch.from_numpy(dy).cuda())[0].cpu().numpy()


@pytest.mark.parametrize("with_dy_dx", [False, True], ids=["features", "dy_dx"])
@pytest.mark.parametrize("n", [256, 768, 1280])
@pytest.mark.parametrize("interpolation", list(INTERP))
@pytest.mark.parametrize("d,f", list(GRIDS))
def test_bits_against_the_oracle(d, f, interpolation, n, with_dy_dx):
    m, og, x, p, dy, want, dy_dx = case(d, f, interpolation, n)
    assert m.fp32_grid_forward(n) == 1
    y, gx = run(m, x, p, dy if with_dy_dx else None)
    assert np.array_equal(bits(y), bits(want)) and y.any()
    if with_dy_dx:
        assert np.array_equal(bits(gx), bits(O.grid_backward_input_f32(og, dy, dy_dx))) and gx.any()


@pytest.mark.parametrize("d,f", [(2, 1), (3, 4), (4, 8)])
def test_the_switch_off_gives_the_same_bits(d, f):
    m, og, x, p, dy, _, _ = case(d, f, "Smoothstep", 768)
    on = run(m, x, p, dy)
    try:
        _C().set_fp32_grid_forward(False)
        assert m.fp32_grid_forward(768) == 0
        off = run(m, x, p, dy)
    finally:
        _C().set_fp32_grid_forward(True)
    assert np.array_equal(bits(on[0]), bits(off[0])) and np.array_equal(bits(on[1]), bits(off[1]))


@pytest.mark.parametrize("per_sample", [False, True], ids=["scalar", "array"])
def test_max_level(per_sample):
    """scalar: the tiled kernel, whose workgroups of the off level load nothing and store zeros; a per-sample array: the probe says 0 and the
    one-thread-per-(sample, level) kernel runs"""
    n = 768
    m, og, x, p, dy, _, _ = case(3, 2, "Linear", n)
    values = np.where(np.arange(n) % 3 == 0, 0.25, 0.5).astype(np.float32) if per_sample else np.float32(0.5)
    off = R.off_mask(values, n, og.n_levels, 2)
    fmask = R.feature_mask(off, 2)
    want, dy_dx = R.forward_f32(og, p, x, off)
    array = torch.from_numpy(np.broadcast_to(values, n).copy()).cuda()  # (the library keeps the pointer only)
    try:
        m.set_max_level_gpu(array) if per_sample else m.set_max_level(0.5)
        assert m.fp32_grid_forward(n) == (0 if per_sample else 1)
        y, gx = run(m, x, p, dy)
        gx_off = run(m, x, p, dy * fmask)[1]  # dL_dy on the off blocks alone: it meets zero rows of dy_dx only
    finally:
        m.set_max_level_gpu(None)
        m.set_max_level(1.0)
    assert off.all(axis=0).any() and not y[fmask].any() and not gx_off.any()
    assert np.array_equal(bits(y), bits(want))
    assert np.array_equal(bits(gx), bits(O.grid_backward_input_f32(og, R.masked(dy, fmask), dy_dx))) and gx.any()


def test_more_segments_than_one_round_of_loads():
    """48 small dense levels, one tile each, of equal cost: six segments per run, two past the four a workgroup searches in registers
    (csrc/grid_forward_plan.h FWD_SEGMENTS_AT_ONCE)"""
    m, og, x, p, dy, want, dy_dx = case(2, 1, "Linear", 256, otype="DenseGrid", levels=48, base=2, scale=1.05)
    assert m.fp32_grid_forward(256) == 1
    y, gx = run(m, x, p, dy)
    assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(gx), bits(O.grid_backward_input_f32(og, dy, dy_dx)))
    assert y[:, 40:].any()


def test_behind_an_fp32_network():
    """the layout the network reads: the same output with the tiled gather and without"""
    n = 768
    cfg, _, _ = make(3, 2)
    C = _C()
    m = C.create_network_with_input_encoding_precision(3, 4, cfg, {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64,
                                                                   "n_hidden_layers": 2}, C.Precision.Fp32)
    rng = np.random.default_rng(7)
    x, p = rng.random((n, 3), dtype=np.float32), (rng.standard_normal(m.n_params()) * 0.3).astype(np.float32)
    assert m.fp32_grid_forward(n) == 1
    on = run(m, x, p)[0]
    try:
        C.set_fp32_grid_forward(False)
        off = run(m, x, p)[0]
    finally:
        C.set_fp32_grid_forward(True)
    assert np.array_equal(bits(on), bits(off)) and on.any()

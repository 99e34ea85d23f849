"""The grid kernels with a per-sample max_level array (GridIO::max_level) and with a scalar below one, on the host SIMT emulator (no GPU),
against the oracle with the off (sample, level) blocks masked (tests/max_level_reference.py): features and dy_dx bit for bit, gradients within
the bars tests/test_gpu_parity.py states for the same passes (restated at each assert).  n = 768: three granules, more than one workgroup of
the tiled gather (512 samples per tile) with a partly filled last tile; the patterns put waves that are wholly off, wholly on and mixed into
one workgroup."""
import numpy as np
import pytest

import emu
import emu_max_level as E
import max_level_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not E.available(), reason="no host compiler for the emulator")

N = 768
# D = 3, F = 2, 8 levels, T = 2^12: dense levels (<= 16^3 entries) and hashed ones; D = 2, F = 4 dense with Smoothstep
GRIDS = {
    "hash3d": (O.grid_init(3, 8, 2, 12, 4, 1.5, O.GRID_HASH, O.INTERP_LINEAR), 8),
    "dense2d": (O.grid_init(2, 4, 4, 19, 8, 2.0, O.GRID_DENSE, O.INTERP_SMOOTHSTEP), 4),
}

MARGINS = {"fractional": 1e-2}  # t = 2.4 / 1.2: no integer, the full margin holds (tests/max_level_reference.py)


def patterns(n, L):
    """name -> (scalar, array or None): every value is k / L"""
    coarse = np.where(np.arange(n) < n // 2, 2.0 / L, 1.0).astype(np.float32)  # whole waves off for the upper levels
    lanes = np.array([2.0 / L, (L - 3.0) / L, 1.0], np.float32)[np.arange(n) % 3]  # neighbouring lanes differ
    return {"scalar": (0.5, None), "fractional": (0.3, None), "constant": (1.0, np.full(n, 0.5, np.float32)), "half-coarse": (1.0, coarse), "interleaved": (0.25, lanes)}


def _inputs(og, n, seed):
    rng = O.pcg32(seed)
    pos = O.generate_random_uniform(rng, n * og.n_dims, 0.0, 1.0).reshape(n, og.n_dims)
    r = np.random.default_rng(seed)
    params = O.f2h((r.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    dy = O.f2h(r.standard_normal((n, og.n_levels * og.n_features_per_level)).astype(np.float32))
    return pos, params, dy


@pytest.fixture(scope="module", params=list(GRIDS))
def case(request):
    og, L = GRIDS[request.param]
    pos, params, dy = _inputs(og, N, 17)
    return og, L, pos, params, dy


@pytest.mark.parametrize("pattern", ["scalar", "fractional", "constant", "half-coarse", "interleaved"])
def test_forward_and_dy_dx_bit_for_bit(case, pattern):
    og, L, pos, params, _ = case
    scalar, array = patterns(N, L)[pattern]
    off = R.off_mask(array if array is not None else scalar, N, L, og.n_features_per_level, margin=MARGINS.get(pattern, R.MARGIN))
    assert off.any() and not off.all()
    want, want_dy_dx = R.forward(og, params, pos, off)
    g = E.Grid(og, max_level=scalar)
    for soa in (True, False):  # the tiled gather in the network's and the bare encoding's layout
        assert np.array_equal(E.grid_forward(g, array, params, pos, soa=soa), want), soa
    got, dy_dx = E.grid_forward(g, array, params, pos, soa=False, want_dy_dx=True)  # the reference-form kernel
    assert np.array_equal(got, want)
    assert np.array_equal(np.transpose(dy_dx, (1, 0, 2)).view(np.uint32), want_dy_dx.view(np.uint32))


def test_nothing_set_changes_nothing(case):
    og, L, pos, params, dy = case
    g = E.Grid(og)
    assert np.array_equal(E.grid_forward(g, None, params, pos), O.grid_forward(og, params, pos))
    ones = np.ones(N, np.float32)
    assert np.array_equal(E.grid_forward(g, ones, params, pos), O.grid_forward(og, params, pos))
    assert np.array_equal(E.grid_backward(g, ones, pos, dy), E.grid_backward(g, None, pos, dy))


@pytest.mark.parametrize("mode", [E.ATOMIC, E.BUCKETED, E.SLICED_F32], ids=["atomic", "bucketed", "sliced"])
@pytest.mark.parametrize("pattern", ["scalar", "fractional", "constant", "half-coarse", "interleaved"])
def test_backward(case, pattern, mode):
    og, L, pos, params, dy = case
    scalar, array = patterns(N, L)[pattern]
    off = R.off_mask(array if array is not None else scalar, N, L, og.n_features_per_level, margin=MARGINS.get(pattern, R.MARGIN))
    ref, absacc = R.backward(og, pos, dy, off)
    got = O.h2f(E.grid_backward(E.Grid(og, max_level=scalar), array, pos, dy, mode=mode)).astype(np.float64)
    # tests/test_gpu_parity.py::test_grid_backward_and_input_gradient: 2^-9 of the magnitude for the fp32 slices, 2^-8 for the modes that add in fp16
    assert np.all(np.abs(got - ref) <= absacc * 2.0 ** (-9 if mode == E.SLICED_F32 else -8) + 2e-3)
    assert not got[absacc == 0].any()  # entries only off pairs touch stay exactly zero
    assert np.abs(ref).max() > 0


def test_constant_array_equals_the_scalar_bit_for_bit(case):
    """(the bucketed backward accumulates exactly, in any order; the atomic form adds in fp16 in the order of arrival and is held to its bar above)"""
    og, L, pos, params, dy = case
    const = np.full(N, 0.5, np.float32)
    assert np.array_equal(E.grid_forward(E.Grid(og, max_level=0.5), None, params, pos), E.grid_forward(E.Grid(og), const, params, pos))
    a = E.grid_backward(E.Grid(og, max_level=0.5), None, pos, dy, mode=E.BUCKETED)
    assert np.array_equal(a, E.grid_backward(E.Grid(og), const, pos, dy, mode=E.BUCKETED))


@pytest.mark.parametrize("pattern", ["scalar", "fractional", "half-coarse", "interleaved"])
def test_second_order(case, pattern):
    """the position kernel (break at the first off level, per sample) and the bucketed parameter scatter with the second-order weight"""
    og, L, pos, params, dy = case
    scalar, array = patterns(N, L)[pattern]
    off = R.off_mask(array if array is not None else scalar, N, L, og.n_features_per_level, margin=MARGINS.get(pattern, R.MARGIN))
    ddx = (np.random.default_rng(3).standard_normal((N, og.n_dims)) * 1e-2).astype(np.float32)
    gp_ref, mag, _, dx_ref = R.backward_backward(og, params, pos, ddx, dy, off)
    grad, dx = E.grid_backward_backward(E.Grid(og, max_level=scalar), array, pos, ddx, dy, params)
    # tests/test_gpu_parity.py::test_grid_second_order_through_c_abi_and_double_backward (every level of these grids is in the bucket plan)
    assert np.all(emu.grid_backward_plan(E.Grid(og), N, mode=E.BUCKETED)[:, 0] == emu.PLAN_BUCKET)
    assert np.allclose(dx, dx_ref, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(dx_ref).max()))
    got = O.h2f(grad).astype(np.float64)
    assert np.all(np.abs(got - gp_ref) <= 2.0 ** -8 * mag + 1e-3 * max(1.0, np.abs(gp_ref).max()))
    assert not got[mag == 0].any()
    assert np.abs(gp_ref).max() > 0 and np.abs(dx_ref).max() > 0


@pytest.mark.parametrize("pattern", ["scalar", "interleaved"])
def test_fp32_encoding(case, pattern):
    og, L, pos, params, dy = case
    scalar, array = patterns(N, L)[pattern]
    off = R.off_mask(array if array is not None else scalar, N, L, og.n_features_per_level, margin=MARGINS.get(pattern, R.MARGIN))
    p32 = (np.random.default_rng(4).standard_normal(og.n_params) * 0.3).astype(np.float32)
    want, want_dy_dx = R.forward_f32(og, p32, pos, off)
    g = E.Grid(og, max_level=scalar)
    got, dy_dx = E.grid_forward_f32(g, array, p32, pos, want_dy_dx=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.transpose(dy_dx, (1, 0, 2)).view(np.uint32), want_dy_dx.view(np.uint32))
    w = O.h2f(dy)
    ref, mag = R.backward_f32(og, pos, w, off)
    grad = E.grid_backward_f32(g, array, pos, w)
    # tests/test_gpu_parity.py::test_fp32_encoding_module: the rounding of a running fp32 sum, hits x 2^-24 x the sum of the magnitudes
    F = og.n_features_per_level
    idx = O.grid_indices(og, pos)
    hits = np.zeros(og.n_params // F, np.int64)
    for l in range(L):
        np.add.at(hits, og.offsets[l] + idx[~off[:, l], l, :].reshape(-1), 1)
    hits = np.repeat(hits, F)
    assert np.all(np.abs(grad - ref) <= np.maximum(hits, 1) * 2.0 ** -24 * mag * 1.001)
    assert not grad[mag == 0].any()


def test_bf16_forward_bit_for_bit():
    og, L = GRIDS["hash3d"]
    O.set_half_format(True)
    try:
        pos, params, _ = _inputs(og, N, 23)
        _, array = patterns(N, L)["interleaved"]
        off = R.off_mask(array, N, L, og.n_features_per_level)
        want, _ = R.forward(og, params, pos, off)
        assert np.array_equal(E.grid_forward(E.Grid(og), array, params, pos, bf16=True), want)
    finally:
        O.set_half_format(False)

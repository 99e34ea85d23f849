"""The grid kernel SOURCES on the host SIMT emulator at positions OUTSIDE the unit cube and ON cell boundaries (tests/grid_domain_positions.py):
cells that wrap modulo 2^32 as the reference's pos_fract defines them (common_device.h:1016-1043).  The oracle is pinned to the reference's own
kernels on the same positions in tests/test_oracle_ref.py; here the kernels are held to the oracle with the bars tests/test_emu_kernels.py and
tests/test_emu_max_level.py state for the same passes (restated at each assert).  No GPU.

What runs here for the first time outside [0, 1): `hhi = hlo + prime` of make_cell, the pair tag of the record scatter and pair_second_index,
the dense form `i1 = i0 + 1` with its `pair_second_index(...) != i1` escape, the second-order, fp32, stochastic and per-sample max_level forms.

Which backward case is which (make_backward_plan, grid_backward_plan.h; asserted in test_plans_hold_the_cases_the_pair_encoding_needs):
  * GRID_CASES[2] (D 3, F 4, T 2^12, Smoothstep), BUCKETED, default LDS budget: a slice holds 128 KiB / (4 x 8 B) = 4096 entries, so the
    hashed levels 2-7 (power-of-two tables of 4096 entries: the `fast` form) run bucketed with ONE bucket.  fast_together holds for every
    sample there, whatever its carry: the pair of a cell -1 (x ^ (x + 1) = 0xFFFFFFFF) stays together with tag 31, the pair of cell
    -(2^17) - 1 with tag 17.  GRID_CASES[3] (F 1, T 2^12) and [4] (F 8, T 2^10) are single-bucket too.
  * GRID_CASES[5] (DenseGrid, D 3, F 2, resolutions 4, 6, 8, 11, 16), BUCKETED: dense levels in one bucket each.  The rows with cell
    (-1, 0, 0) have the dense index 0xFFFFFFFF at the first corner and 0 at its dimension-0 neighbour: the 32-bit index wraps between the
    two, and on the levels whose size does not divide 2^32 (216 and 1336 entries) 0xFFFFFFFF % size + 1 is NOT the second index -- only the
    `pair_second_index(...) != i1` test keeps such a pair out of the queue.
  * lds_budget 1024 (4096 with 16 levels): every level in many buckets, pairs that straddle two of them, the overflow list."""
import numpy as np
import pytest

from oracle import oracle as O

emu = pytest.importorskip("emu")
if not emu.available():
    pytest.skip("ROCm clang++ not available to build the host emulator", allow_module_level=True)

import emu_max_level as EM  # noqa: E402
import grid_domain_positions as GD  # noqa: E402
import max_level_reference as MR  # noqa: E402
from test_emu_kernels import GRID_CASES  # noqa: E402

N = 777  # ragged: no multiple of a wave, a workgroup or a tile; above the generator's 188 mandatory rows for 16 levels
_cache = {}


def setup(case, n=N, seed=41):
    """(oracle grid, positions): one draw per (case, n), shared and never written to"""
    key = (case, n, seed)
    if key not in _cache:
        D, L, F, T, base, scale, gtype, interp = case
        og = O.grid_init(D, L, F, T, base, scale, gtype, interp)
        pos = GD.for_grid(og, n, seed)
        pos.setflags(write=False)
        _cache[key] = (og, pos)
    return _cache[key]


def test_plans_hold_the_cases_the_pair_encoding_needs():
    """the two situations the module's docstring names exist in the plans, and the positions reach them"""
    og, pos = setup(GRID_CASES[2])
    plan = emu.grid_backward_plan(emu.Grid(og), N, mode=emu.BUCKETED)
    sizes = np.array([og.offsets[l + 1] - og.offsets[l] for l in range(og.n_levels)])
    fast = [l for l in range(og.n_levels) if sizes[l] == 4096 and int(og.resolution[l]) ** 3 > 4096]
    assert fast and all(plan[l, 0] == emu.PLAN_BUCKET and plan[l, 1] == 1 for l in fast)
    cells = GD.cells(pos, [og.scale[l] for l in range(og.n_levels)])
    assert all(np.any(cells[:, l, 0] == -1) and GD.has_long_carry(og, pos, l) for l in fast)
    og, pos = setup(GRID_CASES[5])
    plan = emu.grid_backward_plan(emu.Grid(og), N, mode=emu.BUCKETED)
    assert np.all(plan[:, 0] == emu.PLAN_BUCKET) and np.all(plan[:, 1] == 1)
    cells = GD.cells(pos, [og.scale[l] for l in range(og.n_levels)])
    wrapping = 0
    for l in range(og.n_levels):
        size = int(og.offsets[l + 1] - og.offsets[l])
        if (1 << 32) % size and np.any((cells[:, l, 0] == -1) & np.all(cells[:, l, 1:] == 0, axis=1)):
            wrapping += 1  # index 0xFFFFFFFF % size, neighbour 0
    assert wrapping >= 2


@pytest.mark.parametrize("case", GRID_CASES)
def test_grid_forward_bit_exact(case):
    og, pos = setup(case)
    D, L, F = og.n_dims, og.n_levels, og.n_features_per_level
    g = emu.Grid(og)
    params = O.f2h((np.random.default_rng(0).random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    assert np.array_equal(emu.grid_indices(g, pos), O.grid_indices(og, pos))
    ref, ref_dydx = O.grid_forward(og, params, pos, want_dy_dx=True)
    out, dydx = emu.grid_forward(g, params, pos, soa=True, want_dy_dx=True)
    assert np.array_equal(out.T, ref)
    assert np.array_equal(np.transpose(dydx, (1, 0, 2)), ref_dydx)
    assert np.array_equal(emu.grid_forward(g, params, pos, soa=True).T, ref)  # the tiled gather, feature-major ...
    assert np.array_equal(emu.grid_forward(g, params, pos, soa=False, out_stride=L * F + 8)[:, :L * F], ref)  # ... and sample-major


@pytest.mark.parametrize("case", GRID_CASES)
def test_grid_fp32_kernels(case):
    """bars of tests/test_emu_kernels.py::test_grid_fp32_kernels"""
    og, pos = setup(case)
    L, F = og.n_levels, og.n_features_per_level
    n = pos.shape[0]
    g = emu.Grid(og)
    rng = np.random.default_rng(4)
    params = (rng.standard_normal(og.n_params) * 0.3).astype(np.float32)
    ref, ref_dydx = O.grid_forward_f32(og, params, pos, want_dy_dx=True)
    out, dydx = emu.grid_forward_f32(g, params, pos, out_stride=L * F + 8, want_dy_dx=True)
    assert np.array_equal(out[:, :L * F].view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(np.transpose(dydx, (1, 0, 2)), ref_dydx)
    dy = (rng.standard_normal((n, L * F)) * 1.0e4).astype(np.float32)
    want, mag = O.grid_backward_f32(og, pos, dy), O.grid_backward_f32(og, pos, np.abs(dy))
    got = emu.grid_backward_f32(g, pos, dy)
    assert np.all(np.abs(got - want) <= 8 * n * 2.0 ** -24 * np.maximum(mag, 1e-30)) and not got[mag == 0].any()
    if og.interpolation != O.INTERP_NEAREST:
        assert np.array_equal(emu.grid_backward_input_f32(g, dy, dydx), O.grid_backward_input_f32(og, dy, ref_dydx))


@pytest.mark.parametrize("case", GRID_CASES + [(3, 4, 2, 16, 16, 2.0, O.GRID_HASH, O.INTERP_LINEAR)])  # last: > 1 slice per level
@pytest.mark.parametrize("mode,lds_budget", [(emu.SLICED_F32, 0), (emu.SLICED_F16, 0), (emu.ATOMIC, 0), (emu.ATOMIC, 48 * 1024),
                                             (emu.BUCKETED, 0), (emu.BUCKETED, 1024)])
def test_grid_backward(case, mode, lds_budget):
    """modes, budgets and bars of tests/test_emu_kernels.py::test_grid_backward"""
    if mode == emu.ATOMIC and case[2] == 1:
        pytest.skip("the atomic A/B mode needs F >= 2")
    # (small slices: the emulator walks hundreds of tiny workgroups per level; fewer samples, still above the generator's mandatory rows)
    og, pos = setup(case, n=N if lds_budget == 0 else 333)
    L, F = og.n_levels, og.n_features_per_level
    n = pos.shape[0]
    g = emu.Grid(og)
    if lds_budget == 1024 and L > 8:
        lds_budget = 4096  # (as there: sixteen levels of 1 KiB slices are a minute of emulation for the same code paths)
    dy = O.f2h(np.random.default_rng(1).standard_normal((n, L * F)).astype(np.float32))
    ref = O.grid_backward(og, pos, dy)
    dys = np.ascontiguousarray(dy.T)
    got = emu.grid_backward(g, pos, dys, soa=True, mode=mode, lds_budget=lds_budget)  # Overwrite into a garbage-filled buffer
    gotf = O.h2f(got).astype(np.float64)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))))
    tol = absacc * 2.0 ** -9 + 2e-3
    assert np.all(np.abs(gotf - ref) <= tol)
    if mode == emu.SLICED_F32:
        assert np.all(np.abs(gotf - ref) <= np.abs(ref) * 2.0 ** -10 + absacc * 2.0 ** -11 + 1e-6)
    if mode == emu.BUCKETED and F > 1 and lds_budget == 0:
        # one owner per slice, exact sums, ONE rounding: a record sent to a wrong entry shows as two wrong halves
        assert np.mean(got == O.f2h(ref.astype(np.float32))) > 0.999
    assert not gotf[absacc == 0].any()  # entries nothing was sent to stay exactly zero
    acc = emu.grid_backward(g, pos, dys, soa=True, mode=mode, lds_budget=lds_budget, grad_init=got)
    assert np.all(np.abs(O.h2f(acc).astype(np.float64) - 2 * ref) <= 2 * tol + np.abs(ref) * 2.0 ** -9)


@pytest.mark.parametrize("case", [GRID_CASES[2], GRID_CASES[4], GRID_CASES[5]])
def test_grid_backward_bucket_once_is_one_rounding_of_the_exact_sum(case):
    """The bucket-once form sums a slice's records in exact fixed point and rounds once, and the oracle sums the same records in float64: on
    the single-bucket cases (no pair straddles two buckets, nothing travels through fp16 atomics) EVERY entry is the rounded exact sum, bit
    for bit -- a pair whose second record is derived to the wrong entry (tag 31 or 17 on the hashed levels, the wrapped dense index) cannot
    hide inside a tolerance.  (Sums of up to ~200 halves of magnitude <= 8: exact in float64.)"""
    og, pos = setup(case)
    L, F = og.n_levels, og.n_features_per_level
    plan = emu.grid_backward_plan(emu.Grid(og), N, mode=emu.BUCKETED)
    assert np.all(plan[:, 0] == emu.PLAN_BUCKET) and np.all(plan[:, 1] == 1) and np.all(plan[:, 2] == 1)
    dy = O.f2h(np.random.default_rng(2).standard_normal((N, L * F)).astype(np.float32))
    ref = O.grid_backward(og, pos, dy)
    got = emu.grid_backward(emu.Grid(og), pos, np.ascontiguousarray(dy.T), soa=True, mode=emu.BUCKETED)
    assert np.array_equal(O.h2f(got), O.h2f(O.f2h(ref.astype(np.float32))))  # (values: +0 and -0 are the same sum)


@pytest.mark.parametrize("case", [GRID_CASES[0], GRID_CASES[1], GRID_CASES[2], GRID_CASES[4], GRID_CASES[5], GRID_CASES[6]])
def test_grid_second_order(case):
    """bars of tests/test_emu_kernels.py::test_grid_second_order"""
    og, pos = setup(case)
    D, L, F = og.n_dims, og.n_levels, og.n_features_per_level
    n = pos.shape[0]
    rng = np.random.default_rng(8)
    params = O.f2h(((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5))
    dy = O.f2h(rng.standard_normal((n, L * F)).astype(np.float32))
    # The records are dy * ddx * scale (the finest scale of these grids is 7e3) and the positions fold four times the unit cube's area onto each
    # table: with ddx of order one a single entry's exact sum reached 66384, beyond the largest half (65504), where there is nothing to be
    # equal to.  A quarter of that keeps every sum inside the format (asserted); every bar below is relative to the sums, so none widens.
    ddx = (rng.standard_normal((n, D)) * 0.25).astype(np.float32)
    _, dydx = O.grid_forward(og, params, pos, want_dy_dx=True)
    gp_ref, dLddy_ref, dx_ref = O.grid_backward_backward_input(og, params, pos, ddx, dy, dy_dx=dydx)
    assert np.abs(gp_ref).max() < 32752.0  # half of the format's range
    grad, dLddy, dx = emu.grid_backward_backward(emu.Grid(og), pos, ddx, np.ascontiguousarray(dy.T), params, np.ascontiguousarray(np.transpose(dydx, (1, 0, 2))))
    assert np.array_equal(dLddy.T, dLddy_ref)
    assert np.allclose(dx, dx_ref, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(dx_ref).max()))
    mag = np.abs(O.grid_backward_backward_input(og, params, pos, np.abs(ddx), O.f2h(np.abs(O.h2f(dy))))[0]) + np.abs(gp_ref)
    assert np.all(np.abs(O.h2f(grad).astype(np.float64) - gp_ref) <= 2.0 ** -8 * mag + 2e-3 * max(1.0, np.abs(gp_ref).max()) * 2.0 ** -4)
    if og.interpolation != O.INTERP_NEAREST:
        assert np.abs(gp_ref).max() > 0 and np.abs(dx_ref).max() > 0


def test_grid_stochastic_interpolation_backward():
    """as tests/test_emu_kernels.py::test_grid_stochastic_interpolation_backward: the single corner of every (sample, level) is the oracle's;
    unit gradients, so the sums are small integers, exact in fp16"""
    case = (3, 6, 2, 12, 8, 1.6, O.GRID_HASH, O.INTERP_LINEAR)
    og, pos = setup(case, n=512 + 5)
    g = emu.Grid(og, stochastic_interpolation=True)
    dy = O.f2h(np.ones((pos.shape[0], 12), dtype=np.float32))
    ref = O.grid_backward(og, pos, dy, stochastic_interpolation=True)
    for mode in (emu.SLICED_F32, emu.BUCKETED):
        got = O.h2f(emu.grid_backward(g, pos, np.ascontiguousarray(dy.T), mode=mode)).astype(np.float64)
        assert np.array_equal(got, ref)
    assert not np.array_equal(ref, O.grid_backward(og, pos, dy))


# ---- per-sample max_level (tests/test_emu_max_level.py: its grids, patterns and bars)
MAX_LEVEL_GRIDS = {"hash3d": (3, 8, 2, 12, 4, 1.5, O.GRID_HASH, O.INTERP_LINEAR), "dense2d": (2, 4, 4, 19, 8, 2.0, O.GRID_DENSE, O.INTERP_SMOOTHSTEP)}
N_ML = 768 + 5


def _max_level_case(name, pattern):
    from test_emu_max_level import MARGINS, patterns
    og, pos = setup(MAX_LEVEL_GRIDS[name], n=N_ML, seed=17)
    L = og.n_levels
    scalar, array = patterns(N_ML, L)[pattern]
    off = MR.off_mask(array if array is not None else scalar, N_ML, L, og.n_features_per_level, margin=MARGINS.get(pattern, MR.MARGIN))
    assert off.any() and not off.all()
    r = np.random.default_rng(17)
    params = O.f2h((r.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    dy = O.f2h(r.standard_normal((N_ML, L * og.n_features_per_level)).astype(np.float32))
    return og, pos, params, dy, scalar, array, off


@pytest.mark.parametrize("pattern", ["scalar", "half-coarse", "interleaved"])
@pytest.mark.parametrize("name", list(MAX_LEVEL_GRIDS))
def test_max_level_forward_and_dy_dx_bit_for_bit(name, pattern):
    og, pos, params, _, scalar, array, off = _max_level_case(name, pattern)
    want, want_dy_dx = MR.forward(og, params, pos, off)
    g = EM.Grid(og, max_level=scalar)
    for soa in (True, False):
        assert np.array_equal(EM.grid_forward(g, array, params, pos, soa=soa), want), soa
    got, dy_dx = EM.grid_forward(g, array, params, pos, soa=False, want_dy_dx=True)
    assert np.array_equal(got, want)
    assert np.array_equal(np.transpose(dy_dx, (1, 0, 2)), want_dy_dx)


@pytest.mark.parametrize("mode", [EM.ATOMIC, EM.BUCKETED, EM.SLICED_F32], ids=["atomic", "bucketed", "sliced"])
@pytest.mark.parametrize("pattern", ["scalar", "half-coarse", "interleaved"])
@pytest.mark.parametrize("name", list(MAX_LEVEL_GRIDS))
def test_max_level_backward(name, pattern, mode):
    og, pos, _, dy, scalar, array, off = _max_level_case(name, pattern)
    ref, absacc = MR.backward(og, pos, dy, off)
    got = O.h2f(EM.grid_backward(EM.Grid(og, max_level=scalar), array, pos, dy, mode=mode)).astype(np.float64)
    assert np.all(np.abs(got - ref) <= absacc * 2.0 ** (-9 if mode == EM.SLICED_F32 else -8) + 2e-3)
    assert not got[absacc == 0].any()
    assert np.abs(ref).max() > 0

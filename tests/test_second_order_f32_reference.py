"""tests/grid_second_order_f32_reference.py (the numpy restatement of the fp32 second-order pass) pinned to the oracle, on the CPU.  The
oracle's second-order pass takes 16-bit parameters and a 16-bit dL_dy, so both are 16-bit-valued here and the restatement gets the same
numbers as fp32; ddx is fp32.  D in {2, 3}, Linear and Smoothstep, a hash grid whose coarse levels are dense and whose fine ones are hashed
(T = 2^8 at D = 2, 2^10 at D = 3: collisions) and a DenseGrid, positions inside the unit cube and the hard ones of tests/grid_domain_positions.py.

 * dL_dinput against oracle.grid_backward_backward_input, which sums in fp32: within 2^-20 * mag_x.
 * dL_dparams against the oracle's float64 sums: within 2^-20 * mag_p at F = 1, where the oracle's contributions are fp32 products
   (grad_t is float for F = 1, grid.h:665), and within 2^-9 * mag_p at F = 2, where it rounds the corner weight to 16 bits first as the
   reference's T = __half instance does ((GRAD_T)weight * grad).  For Smoothstep a separately named term, cancel_p, is added to either bar:
   the oracle's 1 - S(t) subtracts a rounded S(t) (see the assert).
 * dL_ddLdoutput, rounded to half, equal to the oracle's.  The oracle sums in fp32 and rounds that to half; a float64 sum of the same terms
   can land on the other side of a half-way point between two halves (seen: one element in a thousand).  This result depends on dy_dx and
   ddx only, so it gets a ddx of its own for which the oracle's fp32 sum is the correctly rounded exact sum: signed powers of two (exact
   products) with, at D = 3, one zero component per sample (a single fp32 addition).  The other two results use a ddx of standard_normal * 1e-2, on which
   dL_ddLdoutput is also held to the oracle's within one half ulp."""
import numpy as np
import pytest

import grid_domain_positions as P
import grid_second_order_f32_reference as S
from oracle import oracle as O

N = 128
LOG2_T = {2: 8, 3: 10}  # the finest levels (resolution 32) are hashed: 32^D entries would not fit
INTERPS = {"linear": O.INTERP_LINEAR, "smoothstep": O.INTERP_SMOOTHSTEP}


def _grid(d, f, kind, interp):
    if kind == "hash":
        return O.grid_init(d, 4, f, LOG2_T[d], 4, 2.0, O.GRID_HASH, INTERPS[interp])
    return O.grid_init(d, 4, f, 19, 4 if d == 3 else 8, 2.0 if d == 2 else 1.5, O.GRID_DENSE, INTERPS[interp])


@pytest.mark.parametrize("where", ["inside", "outside"])
@pytest.mark.parametrize("interp", ["linear", "smoothstep"])
@pytest.mark.parametrize("kind", ["hash", "dense"])
@pytest.mark.parametrize("f", [1, 2])
@pytest.mark.parametrize("d", [2, 3])
def test_restatement_against_the_oracle(d, f, kind, interp, where):
    og = _grid(d, f, kind, interp)
    L, K = og.n_levels, og.n_levels * f
    if kind == "hash":  # dense and hashed levels both
        sizes = [og.offsets[l + 1] - og.offsets[l] for l in range(L)]
        assert sizes[0] < 1 << LOG2_T[d] and sizes[-1] == 1 << LOG2_T[d] and og.resolution[L - 1] ** d > 1 << LOG2_T[d]
    seed = 100 * d + 10 * f + (kind == "hash") + 2 * (interp == "linear")
    r = np.random.default_rng(seed)
    pos = O.generate_random_uniform(O.pcg32(seed), N * d, 0.0, 1.0).reshape(N, d) if where == "inside" else P.for_grid(og, N, seed)
    params_h = O.f2h(r.standard_normal(og.n_params).astype(np.float32) * 0.3)
    dy_h = O.f2h(r.standard_normal((N, K)).astype(np.float32))
    ddx = (r.standard_normal((N, d)) * 1e-2).astype(np.float32)
    # for dL_ddLdoutput alone (it depends on dy_dx and ddx only): signed powers of two, and at D = 3 one zero component per sample
    ddx_y = (r.choice([-1.0, 1.0], (N, d)) * 2.0 ** -r.integers(5, 9, (N, d))).astype(np.float32)
    if d == 3:
        ddx_y[np.arange(N), r.integers(0, 3, N)] = 0.0
    _, dy_dx = O.grid_forward(og, params_h, pos, want_dy_dx=True)

    want_p, _, want_x = O.grid_backward_backward_input(og, params_h, pos, ddx, dy_h)
    got = S.second_order(og, O.h2f(params_h), pos, ddx, O.h2f(dy_h))

    assert np.abs(want_x).max() > 0 and np.all(got.mag_x >= np.abs(got.dL_dinput) * (1 - 1e-12))
    ratio_x = np.max(np.abs(got.dL_dinput - want_x) / np.maximum(2.0 ** -20 * got.mag_x, 1e-300))
    print(f"dL_dinput: max |restatement - oracle| / (2^-20 mag_x) = {ratio_x:.4f}")
    assert np.all(np.abs(got.dL_dinput - want_x) <= 2.0 ** -20 * got.mag_x)
    # The oracle forms Smoothstep's lower weight as 1 - S(t) from an fp32 S(t) (three roundings, <= 3 * 2^-24 absolute since S <= 1; a fourth
    # for the subtraction): an ABSOLUTE error of that weight, which no multiple of mag_p covers where the weight is small.  It is a term of
    # its own, cancel_p, zero for Linear -- not part of mag_p.  Without it the Smoothstep F = 1 cases miss 2^-20 mag_p by up to 115 times.
    got_c = S.second_order(og, O.h2f(params_h), pos, ddx, O.h2f(dy_h), lower_weight_abs_error=4 * 2.0 ** -24)
    assert np.array_equal(got_c.dL_dparams, got.dL_dparams) and np.array_equal(got_c.mag_p, got.mag_p)
    assert (interp == "smoothstep") == bool(got_c.cancel_p.any())
    assert np.abs(want_p).max() > 0
    # F = 1: the oracle's contributions are fp32 products.  F > 1: it rounds each dimension's weight to 16 bits and multiplies in 16 bits,
    # two roundings of 2^-11 per term -- 2^-10 mag_p, held to 2^-9: loose, but an indexing or sign error of the F > 1 path is of order mag_p.
    rel = 2.0 ** -20 if f == 1 else 2.0 ** -9
    # (F > 1 also: the 16-bit weight and product round to the format's subnormal spacing when small, 2^-25 absolute each, per dimension's term)
    underflow = 0.0 if f == 1 else got.hits * d * 2.0 ** -25 * (1.0 + np.abs(O.h2f(dy_h)).max())
    bar_p = rel * got.mag_p + got_c.cancel_p + underflow
    ratio_p = np.max(np.abs(got.dL_dparams - want_p) / np.maximum(bar_p, 1e-300))
    print(f"dL_dparams: max |restatement - oracle| / ({rel:g} mag_p + cancel_p) = {ratio_p:.4f}")
    assert np.all(np.abs(got.dL_dparams - want_p) <= bar_p)
    assert not want_p[got.hits == 0].any() and not got.dL_dparams[got.hits == 0].any()
    # dL_ddLdoutput on the ordinary ddx: within one half ulp of the oracle's (equal except across a half-way point)
    _, want_y0, _ = O.grid_backward_backward_input(og, params_h, pos, ddx, dy_h, dy_dx=dy_dx)
    got_y0 = S.second_order(og, O.h2f(params_h), pos, ddx, O.h2f(dy_h), dy_dx=dy_dx).dL_ddLdoutput
    a, b = O.h2f(O.f2h(got_y0.astype(np.float32))).astype(np.float64), O.h2f(want_y0).astype(np.float64)
    half_ulp = 2.0 ** np.maximum(np.floor(np.log2(np.maximum(np.maximum(np.abs(a), np.abs(b)), 2.0 ** -14))) - 10, -24)
    assert np.all(np.abs(a - b) <= half_ulp) and np.mean(a != b) < 0.01
    _, want_y, _ = O.grid_backward_backward_input(og, params_h, pos, ddx_y, dy_h, dy_dx=dy_dx)
    got_y = S.second_order(og, O.h2f(params_h), pos, ddx_y, O.h2f(dy_h), dy_dx=dy_dx).dL_ddLdoutput
    assert np.any(O.h2f(want_y) != 0) and np.array_equal(O.f2h(got_y.astype(np.float32)), want_y)


def test_hits_count_every_contribution_and_the_mask_removes_its_share():
    og = _grid(3, 2, "hash", "linear")
    r = np.random.default_rng(5)
    pos = r.random((N, 3), dtype=np.float32)
    params = (r.standard_normal(og.n_params) * 0.3).astype(np.float32)
    dy = r.standard_normal((N, 8)).astype(np.float32)
    ddx = (r.standard_normal((N, 3)) * 1e-2).astype(np.float32)
    full = S.second_order(og, params, pos, ddx, dy)
    assert full.hits.sum() == N * 4 * 8 * 2
    off = S.off_mask(0.5, N, 4, 2)
    half = S.second_order(og, params, pos, ddx, dy, off=off)
    assert half.hits.sum() == N * 3 * 8 * 2  # t = 2: levels 0 to 2 stay on (l > t + 1e-3 is off)
    dy0 = dy.copy()
    dy0[:, 6:] = 0
    zeroed = S.second_order(og, params, pos, ddx, dy0)
    assert np.array_equal(half.dL_dparams, zeroed.dL_dparams) and np.array_equal(half.dL_dinput, zeroed.dL_dinput)
    nearest = S.second_order(O.grid_init(3, 4, 2, 10, 4, 2.0, O.GRID_HASH, O.INTERP_NEAREST), params, pos, ddx, dy)
    assert not nearest.dL_dparams.any() and not nearest.dL_dinput.any() and not nearest.hits.any()

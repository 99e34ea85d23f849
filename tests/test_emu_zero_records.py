"""The record scatter drops pair records whose payloads are all +-0 (csrc/grid_backward_scatter.hip).  On the host SIMT emulator (no GPU) the
scatter and the owners are compiled twice -- as shipped, and with the drop compiled out (-DTCNN_TEST_KEEP_ZERO_RECORDS, tests/emu only) -- and
must give the SAME BITS in every entry of the grid gradient, leave every counter zeroed (the driver fails otherwise), and the shipped build
must queue strictly fewer pairs wherever the pattern has an all-zero pair.

Shapes: N = 1000 (ragged against the 512-sample tile), D = 2 and 3, F = 1, 2 and 4, 4 levels of base 4, scale 2, T = 2^12 (dense coarse levels
and hashed ones), linear and nearest interpolation, first and second order, fp16 and bf16, Overwrite and Accumulate (into a table with -0
entries).  The planner splits a level's samples over several owners ("chunked") only beyond 65536 records per table slice, which N = 1000 does
not reach: the chunked path -- the one place where zero records are KEPT, in Accumulate mode -- has cases of its own at N = 9000, D = 3.

Which patterns must queue strictly fewer pairs (reasoned, not read off the result):
  * dL/dy zero for a whole sample (all zero, all but one sample, alternate samples, +0 / -0 mixed): every pair of that sample is all zero;
  * one feature zero: F = 1 makes that every record; with F >= 2 the other half of the packed word is non-zero and NOTHING may be dropped
    (equal counts: a test that a half-zero word is not taken for zero);
  * 1-4 subnormal units: (GRAD_T)weight * g rounds to zero where weight * units <= 1/2 -- with trilinear / bilinear weights (mean 2^-D) that is
    most corners, but only for 16-bit payloads (F >= 2: F = 1 carries an fp32 product), weights below one (linear) and the first-order weight;
  * ordinary values: the control, nothing to drop but the odd corner weight that rounds to zero (fewer or equal)."""
import numpy as np
import pytest

import emu_zero_records as E
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not E.available(), reason="no host compiler for the emulator")

N = 1000
N_CHUNKED = 9000  # 72000 records per level and slice: three sample chunks
PATTERNS = ["all_zero", "one_sample", "alternate", "one_feature_zero", "signed_zeros", "subnormal", "ordinary"]


def make_grid(D, F, interp):
    return O.grid_init(D, 4, F, 12, 4, 2.0, O.GRID_HASH, interp)


def make_dy(pattern, n, K, F, seed):
    """[n][K] bit patterns of the 16-bit type (the same bits serve fp16 and bf16: zeros, subnormal units, and values whose high bits are an
    ordinary number in either format)"""
    r = np.random.default_rng(seed)
    sign = (r.integers(0, 2, (n, K)) << 15).astype(np.uint16)
    ordinary = (r.integers(0x2C00, 0x3C00, (n, K)).astype(np.uint16) | sign)  # fp16: 2^-4 .. 1; bf16: 2^-39 .. 2^-7
    if pattern == "ordinary":
        return ordinary
    if pattern == "all_zero":
        return np.zeros((n, K), np.uint16)
    if pattern == "one_sample":
        dy = np.zeros((n, K), np.uint16)
        dy[n // 3] = ordinary[n // 3]
        return dy
    if pattern == "alternate":
        dy = ordinary.copy()
        dy[::2] = 0
        return dy
    if pattern == "one_feature_zero":
        dy = ordinary.copy()
        dy[:, ::F] = 0  # feature 0 of every level
        return dy
    if pattern == "signed_zeros":
        return sign
    if pattern == "subnormal":
        return r.integers(1, 5, (n, K)).astype(np.uint16) | sign
    raise KeyError(pattern)


def must_be_fewer(pattern, F, linear, second_order):
    if pattern in ("all_zero", "one_sample", "alternate", "signed_zeros"):
        return True
    if pattern == "one_feature_zero":
        return F == 1
    if pattern == "subnormal":
        return F >= 2 and linear and not second_order
    return False


def grad_with_negative_zeros(n_params, seed):
    """a table to accumulate into: ordinary values, +0 and -0 entries"""
    r = np.random.default_rng(seed)
    g = r.integers(0x2C00, 0x3C00, n_params).astype(np.uint16) | (r.integers(0, 2, n_params) << 15).astype(np.uint16)
    kind = r.integers(0, 4, n_params)
    g[kind == 0] = 0x8000
    g[kind == 1] = 0x0000
    return g


def run_case(og, n, pattern, second_order, bf16, accumulate, seed):
    D, F, K = og.n_dims, og.n_features_per_level, og.n_levels * og.n_features_per_level
    pos = O.generate_random_uniform(O.pcg32(seed), n * D, 0.0, 1.0).reshape(n, D)
    dy = make_dy(pattern, n, K, F, seed)
    ddx = (np.random.default_rng(seed + 1).standard_normal((n, D)) * 1e-2).astype(np.float32) if second_order else None
    init = grad_with_negative_zeros(og.n_params, seed + 2) if accumulate else None
    g = E.Grid(og)
    got, pairs, over = E.grid_backward(g, pos, dy, ddx=ddx, grad_init=init, keep=False, bf16=bf16)
    want, pairs_keep, over_keep = E.grid_backward(g, pos, dy, ddx=ddx, grad_init=init, keep=True, bf16=bf16)
    return got, want, init, (pairs, over), (pairs_keep, over_keep)


# (second order with nearest interpolation is no case: d(dy/dx)/d(grid) is zero without interpolation, grid.h:422-425 -- grid_backward() clears
# the gradient and runs no scatter)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("interp,second_order", [("linear", False), ("nearest", False), ("linear", True)], ids=["linear-first", "nearest-first", "linear-second"])
@pytest.mark.parametrize("F", [1, 2, 4])
@pytest.mark.parametrize("D", [2, 3])
def test_dropping_zero_records_changes_no_bit(D, F, interp, second_order, bf16):
    linear = interp == "linear"
    og = make_grid(D, F, O.INTERP_LINEAR if linear else O.INTERP_NEAREST)
    assert not (E.level_chunks(E.Grid(og), N) != 1).any()  # every level bucketed, one owner per slice
    for pattern in PATTERNS:
        for accumulate in (False, True):
            got, want, init, (pairs, over), (pairs_keep, over_keep) = run_case(og, N, pattern, second_order, bf16, accumulate, seed=11 + D + F)
            where = (pattern, accumulate)
            assert np.array_equal(got, want), where
            assert pairs_keep > 0, where
            assert pairs + over <= pairs_keep + over_keep and pairs <= pairs_keep and over <= over_keep, where
            if must_be_fewer(pattern, F, linear, second_order):
                assert pairs < pairs_keep, where
            if pattern == "one_feature_zero" and F >= 2 and not second_order:
                assert (pairs, over) == (pairs_keep, over_keep), where  # a word with one non-zero half is not zero
            if pattern in ("all_zero", "signed_zeros"):
                # every queue is empty: the owners still clear and store their slices (Overwrite), or add +0 (Accumulate: -0 + +0 = +0)
                assert (pairs, over) == (0, 0), where
                expect = np.zeros_like(got) if not accumulate else np.where(init == 0x8000, 0, init).astype(np.uint16)
                assert np.array_equal(got, expect), where
            if pattern == "ordinary":
                assert got.any() and (accumulate or np.count_nonzero(got) > got.size // 8), where


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("pattern", ["all_zero", "alternate", "subnormal", "ordinary"])
def test_chunked_levels(pattern, bf16):
    """Several owners per slice: the scatter zeroes the level (Overwrite) and the owners add their non-zero sums with atomics.  In Accumulate
    mode nothing clears or stores such a level, an entry may keep the caller's -0, and the scatter keeps every record of it."""
    og = make_grid(3, 2, O.INTERP_LINEAR)
    chunks = E.level_chunks(E.Grid(og), N_CHUNKED)
    assert (chunks > 1).all()
    for accumulate in (False, True):
        got, want, init, (pairs, over), (pairs_keep, over_keep) = run_case(og, N_CHUNKED, pattern, False, bf16, accumulate, seed=5)
        assert np.array_equal(got, want), accumulate
        if accumulate:
            assert (pairs, over) == (pairs_keep, over_keep)  # every level is chunked: nothing is dropped
            if pattern == "all_zero":
                assert np.array_equal(got, init)  # -0 entries included: no owner touched them
        else:
            assert pairs <= pairs_keep and over <= over_keep
            if pattern != "ordinary":
                assert pairs < pairs_keep
            if pattern == "all_zero":
                assert (pairs, over) == (0, 0) and not got.any()


N_LEVEL3_BUCKETS = 4  # T = 2^16: the finest level (32^3 entries, dense) is cut into four slices of 2^13 entries


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("pattern", ["alternate", "one_feature_zero", "subnormal", "ordinary"])
def test_records_on_the_overflow_list(pattern, bf16):
    """Both routes onto the overflow list, bit for bit.  T = 2^16 and every sample inside the one cell of the finest level whose x-neighbour
    pair (entries 8191, 8192) straddles two slices: that pair's second record travels through the list alone (1000 records), and the other
    three pairs of every sample land in one slice's queue, 3000 pairs against a capacity of 2 * 1000 + 512 rounded up to 2560 -- the rest
    spills, both records of a pair each on its own.  Asserted below from the oracle's indices.  (The owners pick their records out of the list
    themselves up to 2^18 of them: exact sums, so the two builds must agree in every bit whichever pairs spilled.)"""
    og = O.grid_init(3, 4, 2, 16, 4, 2.0, O.GRID_HASH, O.INTERP_LINEAR)
    n, K = N, og.n_levels * og.n_features_per_level
    pos = (np.array([0.992, 0.992, 0.225], np.float32) + (O.generate_random_uniform(O.pcg32(3), n * 3, 0.0, 1.0).reshape(n, 3) - 0.5) * 0.008).astype(np.float32)
    idx = O.grid_indices(og, pos)[:, 3, :]
    assert og.offsets[4] - og.offsets[3] == N_LEVEL3_BUCKETS << 13
    crossing = (idx[:, 0::2] >> 13) != (idx[:, 1::2] >> 13)
    per_bucket = np.bincount((idx[:, 0::2] >> 13).reshape(-1), minlength=N_LEVEL3_BUCKETS)
    capacity = (2 * (n * 4 // N_LEVEL3_BUCKETS) + 512 + 63) // 64 * 64
    assert crossing.sum() == n and per_bucket.max() - capacity >= 400
    g = E.Grid(og)
    assert (E.level_chunks(g, n) == 1).all()
    dy = make_dy(pattern, n, K, 2, seed=13)
    for accumulate in (False, True):
        init = grad_with_negative_zeros(og.n_params, 17) if accumulate else None
        got, pairs, over = E.grid_backward(g, pos, dy, grad_init=init, keep=False, bf16=bf16)
        want, pairs_keep, over_keep = E.grid_backward(g, pos, dy, grad_init=init, keep=True, bf16=bf16)
        assert np.array_equal(got, want), accumulate
        # kept: one list record per crossing pair, two per spilled pair
        assert over_keep == n + 2 * (per_bucket.max() - capacity), accumulate
        assert 0 < over <= over_keep and pairs <= pairs_keep
        assert got.any() or pattern == "subnormal"  # (bf16: sums of 2^-133 units lie below the owners' finest fixed-point unit, 2^-40)
        if pattern == "alternate":  # half the samples send nothing: half the crossing records, and the queue no longer spills (1500 pairs)
            assert over == n // 2, accumulate
        if pattern == "one_feature_zero":  # a word with one non-zero half is no zero: nothing may be dropped
            assert (pairs, over) == (pairs_keep, over_keep), accumulate
        if pattern == "subnormal":  # zero records next to non-zero ones in the crossing pairs and in the spilled ones
            assert over < over_keep and pairs < pairs_keep, accumulate

"""The bucketed grid backward on the host SIMT emulator, BIT FOR BIT against the 64-bit-per-value owners (grid_owner_mode 1, the
SLICE_FIXED64 accumulators of k_grid_backward_sliced) and the packed kernel's own wide redo (mode 2).  All three are exact integer sums of
the records the scatter queued, rounded once, so no entry of the gradient may differ in any bit -- the way
tests/test_emu_kernels.py::test_grid_bucket_owner_forms_agree compares them, over the shapes at which the scatter's tile loop and the owners'
stream loop change path (tests/scatter_owner_cases.py): a partial tile, a tile edge from both sides, several tiles, several tiles per
persistent workgroup; dense-only and hashed tables; uniform samples and all samples in one cell, which fills a queue past its capacity and
sends the rest through the overflow list (asserted from the plan's arithmetic, not assumed).

The owners share the scatter, so equal bits among them do not pin the records themselves: every case is also held against the CPU oracle
with the bar of test_grid_bucket_owner_forms_agree (2^-9 of the accumulated magnitude + 2e-3 of the gradient scale)."""
import numpy as np
import pytest

import emu
import scatter_owner_cases as K
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not emu.available(), reason="no host compiler for the emulator")

MAGNITUDE = 0.05  # scatter_owner_cases.make_dy


def run_case(D, table, kind, n, lds_budget, slice_entries):
    og = K.oracle_grid(D, table)
    g = emu.Grid(og)
    pos = K.make_positions(kind, n, D)
    dy = K.make_dy(n, og.n_levels * K.F)
    dys = np.ascontiguousarray(dy.T)
    spilled = K.spilled_pairs(og, pos, slice_entries)
    if K.must_overflow(og, kind, n, slice_entries):
        assert spilled > 0, "the case does not fill a queue: it does not test the overflow list"
    emu.grid_owner_stats()
    got = {o: emu.grid_backward(g, pos, dys, soa=True, mode=emu.BUCKETED, lds_budget=lds_budget, owner=o) for o in (emu.OWNER_PACKED, emu.OWNER_FIXED64, emu.OWNER_WIDE)}
    n_packed, n_wide = emu.grid_owner_stats()
    assert n_packed > 0
    for o in (emu.OWNER_FIXED64, emu.OWNER_WIDE):
        differing = int(np.count_nonzero(got[emu.OWNER_PACKED].view(np.int16) != got[o].view(np.int16)))
        assert differing == 0, (o, differing)
    ref = O.grid_backward(og, pos, dy)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))))
    assert np.all(np.abs(O.h2f(got[emu.OWNER_PACKED]).astype(np.float64) - ref) <= absacc * 2.0 ** -9 + 2e-3 * MAGNITUDE)
    if n > 1:
        assert np.count_nonzero(got[emu.OWNER_PACKED]) > 0
    return spilled


@pytest.mark.parametrize("kind", K.POSITIONS)
@pytest.mark.parametrize("table", list(K.TABLES))
@pytest.mark.parametrize("n", K.BATCHES)
@pytest.mark.parametrize("D", K.DIMS)
def test_bucketed_backward_bits(D, n, table, kind):
    run_case(D, table, kind, n, lds_budget=0, slice_entries=K.DEFAULT_SLICE_ENTRIES)


@pytest.mark.parametrize("D", K.DIMS)
def test_hashed_table_overflows_with_small_slices(D):
    """The hashed table has two queues per level at the default slice size and cannot fill one; with 2 KiB slices (128 entries, 128 queues a
    level) the one-cell batch of 4096 does."""
    assert K.must_overflow(K.oracle_grid(D, "hashed"), "one_cell", 4096, 128)
    spilled = run_case(D, "hashed", "one_cell", 4096, lds_budget=2048, slice_entries=128)
    assert spilled > 4096


def test_the_list_has_a_case_that_fills_a_queue():
    assert K.must_overflow(K.oracle_grid(3, "dense"), "one_cell", 4096)

"""The bucketed grid backward on the GPU, BIT FOR BIT against the library's own wide owner form (grid_owner_mode 2: every slice through the
packed kernel's 64-bit-per-value redo, exact sums of the same queued records, rounded once), over the cases of
tests/test_emu_scatter_owner_bits.py (tests/scatter_owner_cases.py).  The packed owners' stream loop -- loads, conversion and bound written as
inline assembly -- is compiled out of the host emulator: this is where its bits are pinned, subnormal payloads included.  Every sample chunk
has a sole owner at these sizes and the overflow list stays short enough for the owners to scan it themselves, so no entry may differ.
The records themselves are held against the CPU oracle with the bar of test_gpu_parity.py::test_bucketed_grid_backward_full_size.

Batches reach the kernels padded to the batch granularity (256) with rows whose dL/dy is zero, as a ragged batch does in use."""
import numpy as np
import pytest
import torch

import scatter_owner_cases as K
from oracle import oracle as O
from test_gpu_parity import h_t, tcnn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def encodings():
    C = tcnn()._C
    return C, {(D, table): (C.create_encoding(D, K.encoding_config(table)), K.oracle_grid(D, table)) for D in K.DIMS for table in K.TABLES}


@pytest.mark.parametrize("kind", K.POSITIONS)
@pytest.mark.parametrize("table", list(K.TABLES))
@pytest.mark.parametrize("n", K.BATCHES)
@pytest.mark.parametrize("D", K.DIMS)
def test_bucketed_backward_bits(encodings, D, n, table, kind):
    C, enc = encodings
    m, og = enc[(D, table)]
    padded = (n + 255) // 256 * 256
    pos = np.zeros((padded, D), np.float32)
    pos[:n] = K.make_positions(kind, n, D)
    if kind == "one_cell":
        pos[n:] = pos[0]  # (the padding rows queue nothing: their dL/dy is zero)
    dy = np.zeros((padded, m.n_output_dims()), np.uint16)
    dy[:n] = K.make_dy(n, m.n_output_dims())
    spilled = K.spilled_pairs(og, pos[:n])
    if K.must_overflow(og, kind, n):
        assert spilled > 0, "the case does not fill a queue: it does not test the overflow list"
    x = torch.from_numpy(pos).cuda()
    p = torch.zeros(og.n_params, dtype=torch.half, device="cuda").requires_grad_(True)
    ctx, y = m.fwd(x, p)
    out = {}
    default_owner, default_mode = C.get_grid_owner_mode(), C.get_grid_backward_mode()
    try:
        C.set_grid_backward_mode(3)
        for owner in (0, 2):
            C.set_grid_owner_mode(owner)
            _, dp = m.bwd(ctx, x, p, y, h_t(dy))
            torch.cuda.synchronize()
            out[owner] = dp.cpu().view(torch.int16).numpy().copy()
    finally:
        C.set_grid_owner_mode(default_owner)
        C.set_grid_backward_mode(default_mode)
    differing = int(np.count_nonzero(out[0] != out[2]))
    per_level = [int(np.count_nonzero(out[0][og.offsets[l] * K.F:og.offsets[l + 1] * K.F] != out[2][og.offsets[l] * K.F:og.offsets[l + 1] * K.F])) for l in range(og.n_levels)]
    print(f"D {D} n {n} {table} {kind}: {differing} differing entries of {out[0].size} (per level {per_level}), {spilled} pairs past their queue's capacity")
    assert differing == 0
    got = O.h2f(out[0].view(np.uint16)).astype(np.float64)
    ref = O.grid_backward(og, pos[:n], dy[:n])
    absacc = O.grid_backward(og, pos[:n], O.f2h(np.abs(O.h2f(dy[:n]))))
    assert np.all(np.abs(got - ref) <= absacc * 2.0 ** -8 + 1e-3)
    if n > 1:
        assert got.any()

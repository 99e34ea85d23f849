"""Positions for the grid encodings OUTSIDE the unit cube and ON cell boundaries -- the one generator every leg of the suite draws them from
(tests/test_oracle_ref.py, tests/test_emu_grid_domain.py, tests/test_gpu_grid_domain.py, tests/golden/make_ref_golden.py).  Plain numpy.

The reference defines what happens there (pos_fract, common_device.h:1016-1043): cell = (uint32_t)(int)floorf(fmaf(scale, x, 0.5f)), so cell
coordinates wrap modulo 2^32, are hashed or taken modulo the table size, and the weights come from the fraction.

hard_positions(n, d, scales, resolutions, seed) -> float32 [n, d], deterministic:
  * a bulk uniform in [-1.5, 2.5);
  * SPECIALS, each once in all dimensions at once and once in one dimension of an otherwise random row;
  * per level l and j in {-3, -1, 0, 1, res_l - 1, res_l, res_l + 2}: float32((j - 0.5) / scale_l) in dimension l % d -- the fma lands on or
    beside the integer j, a cell boundary;
  * per level, two rows whose dimension-0 cell is -1 (grid[0] == 0xFFFFFFFF) and whose other dimensions stay inside the cube: random there,
    and in cell 0 (the dense index of (-1, 0, ...) is 0xFFFFFFFF, that of its dimension-0 neighbour (0, 0, ...) is 0: the 32-bit index wraps
    between the two corners of a pair);
  * per level where the bound below allows it, one row whose dimension-0 cell is -(2^17) - 1: 17 trailing one bits.  The record scatter stores
    that count in five bits (grid_backward_plan.h); cell -1 is the count 31, but every table that keeps such a pair together is smaller than
    2^15 entries, where any count >= 14 gives the same second index -- a cell with 16 to 30 trailing ones is what tells a narrower field.
The rows are shuffled, so the special ones land in different lanes, waves and tiles.

Two bounds, the only exclusions: |x| * max(scale) + 0.5 < 2^31 for every value (beyond it the reference's float -> int conversion is
undefined and x86 and gfx950 differ), and no NaN or Inf.  Both are asserted, and so is what keeps a test on these positions from being
vacuous: at least half of all coordinates outside [0, 1), and per level a sample with dimension-0 cell 0xFFFFFFFF and a sample with a
(positive) cell >= the level's resolution.  for_grid() adds the check on the oracle's own indices: each below its level's table size."""
import numpy as np

SPECIALS = np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, -1.0, 2.0, -2.0 ** -24, -1e-30, -1e-40,  # (-1e-40: a negative subnormal)
                     1000.0, -1000.0, 2047.5, -2047.25], dtype=np.float32)
BOUNDARY_CELLS = (-3, -1, 0, 1)        # and res - 1, res, res + 2 of the level
LONG_CARRY_CELL = -(1 << 17) - 1       # 0xFFFDFFFF: 17 trailing ones


def cells(x, scales):
    """[n, L, d] int64: floor(fma(scale, x, 0.5)) as the reference's pos_fract finds it -- the product is exact in float64, the sum is rounded
    to float32 once more than the fma rounds (used for the coverage statistics below, not as a reference)."""
    p = (np.asarray(scales, np.float32).astype(np.float64)[None, :, None] * x.astype(np.float64)[:, None, :] + 0.5).astype(np.float32)
    return np.floor(p).astype(np.int64)


def n_required(n_levels, d):
    return 2 * SPECIALS.size + n_levels * (len(BOUNDARY_CELLS) + 3 + 3)


def hard_positions(n, d, scales, resolutions, seed):
    scales = np.asarray(scales, np.float32)
    resolutions = np.asarray(resolutions, np.int64)
    L = scales.size
    assert resolutions.size == L and n >= n_required(L, d), (n, n_required(L, d))
    rng = np.random.default_rng(seed)
    x = (rng.random((n, d), dtype=np.float32) * np.float32(4.0) - np.float32(1.5)).astype(np.float32)  # the bulk: [-1.5, 2.5)
    limit = (2.0 ** 31 - 1.0) / float(scales.max())
    row = 0
    for v in SPECIALS:
        x[row] = v
        x[row + 1, rng.integers(d)] = v
        row += 2
    for l in range(L):
        s = np.float64(scales[l])
        for j in BOUNDARY_CELLS + (int(resolutions[l]) - 1, int(resolutions[l]), int(resolutions[l]) + 2):
            x[row, l % d] = np.float32((j - 0.5) / s)
            row += 1
        x[row] = rng.random(d, dtype=np.float32)             # inside the cube ...
        x[row, 0] = np.float32(-1.0 / s)                     # ... but for dimension 0: the middle of cell -1
        x[row + 1] = np.float32(0.25 / s)                    # cell 0, inside the cube
        x[row + 1, 0] = np.float32(-1.0 / s)
        row += 2
        if abs(LONG_CARRY_CELL) / s < 0.99 * limit:
            x[row] = rng.random(d, dtype=np.float32)
            x[row, 0] = np.float32(LONG_CARRY_CELL / s)      # fma = cell + 0.5: its middle
            row += 1
    assert row <= n_required(L, d)
    x = x[rng.permutation(n)]

    # the two bounds
    assert np.isfinite(x).all()
    assert np.all(np.abs(x.astype(np.float64)) * float(scales.max()) + 0.5 < 2.0 ** 31)
    # not vacuous
    assert np.mean((x < 0) | (x >= 1)) >= 0.5
    c = cells(x, scales)
    for l in range(L):
        assert np.any(c[:, l, 0] == -1), l
        assert np.any(c[:, l, :] >= resolutions[l]), l
    return x


def for_grid(og, n, seed):
    """hard_positions for an oracle grid (oracle.Grid), with the checks on the oracle's own indices."""
    from oracle import oracle as O
    L = og.n_levels
    x = hard_positions(n, og.n_dims, [og.scale[l] for l in range(L)], [og.resolution[l] for l in range(L)], seed)
    idx = O.grid_indices(og, x)
    corners = 1 if og.interpolation == O.INTERP_NEAREST else idx.shape[2]
    for l in range(L):
        assert np.all(idx[:, l, :corners] < og.offsets[l + 1] - og.offsets[l]), l
    return x


def has_long_carry(og, x, level):
    """does a sample's dimension-0 cell at `level` carry 16 to 30 trailing one bits?"""
    c = cells(x, [og.scale[l] for l in range(og.n_levels)])[:, level, 0] & 0xFFFFFFFF
    t = np.array([((int(v) ^ (int(v) + 1)) & 0xFFFFFFFF).bit_length() - 1 for v in c])
    return bool(np.any((t >= 16) & (t <= 30)))

"""Cases of the bit-for-bit tests of the bucketed grid backward (tests/test_emu_scatter_owner_bits.py on the host emulator,
tests/test_gpu_scatter_owner_bits.py on the GPU): tables, batch sizes, positions, dL/dy, and the arithmetic that says whether a case
sends pairs through the overflow list because a queue is full.

Tables (F = 2, hash grid type, base 16, per_level_scale 2):
  dense   3 levels, T = 2^19: resolutions 16, 32, 64 -- every level smaller than its table, indexed densely;
  hashed  8 levels, T = 2^14: resolutions 16 .. 2048 -- the fine levels hashed into a power-of-two table.
Batch sizes: one partial tile (1), an edge of 256 samples from both sides (255, 257), one sample past 512 -- a whole tile at D = 3 -- (513),
and many tiles per level (4096), which also fills queues past the owners' first round of loads.
Positions: uniform in the unit cube, and every sample in ONE cell of every level."""
import numpy as np

from oracle import oracle as O

DIMS = [2, 3]
BATCHES = [1, 255, 257, 513, 4096]
TABLES = {"dense": dict(n_levels=3, log2_hashmap_size=19), "hashed": dict(n_levels=8, log2_hashmap_size=14)}
POSITIONS = ["uniform", "one_cell"]
F, BASE, SCALE = 2, 16, 2.0
DEFAULT_SLICE_ENTRIES = 8192  # make_backward_plan: 128 KiB of 64-bit accumulators per slice, F = 2


def oracle_grid(D, table):
    t = TABLES[table]
    return O.grid_init(D, t["n_levels"], F, t["log2_hashmap_size"], BASE, SCALE, O.GRID_HASH, O.INTERP_LINEAR)


def encoding_config(table):
    t = TABLES[table]
    return {"otype": "HashGrid", "n_levels": t["n_levels"], "n_features_per_level": F, "log2_hashmap_size": t["log2_hashmap_size"],
            "base_resolution": BASE, "per_level_scale": SCALE}


def make_positions(kind, n, D, seed=3):
    r = np.random.default_rng(seed)
    u = r.random((n, D), dtype=np.float32)
    if kind == "uniform":
        return u
    # 0.37 * resolution + 0.5 has a fraction between 0.18 and 0.94 at every resolution used here: 1e-5 of spread stays inside the cell
    return (0.37 + u * 1e-5).astype(np.float32)


def make_dy(n, K, seed=4):
    """half bit patterns [n][K]: ordinary values, and every other row small enough that the products with the corner weights are
    subnormal halves (the owners' fixed-point conversion must carry those exactly)"""
    r = np.random.default_rng(seed)
    dy = (r.standard_normal((n, K)) * 0.05).astype(np.float32)
    dy[1::2] *= 1e-3
    return O.f2h(dy)


def spilled_pairs(og, pos, slice_entries=DEFAULT_SLICE_ENTRIES):
    """Pairs that cannot fit their queue, by make_backward_plan's rule: a level of `entries` entries has ceil(entries / slice_entries) queues
    (one sample chunk: at most 4096 * 8 records per level here, below the 65536 per slice beyond which samples are split) of capacity
    2 * (n * pairs per sample / queues) + 512 pairs, rounded up to a multiple of 64.  A pair goes to the queue of its first entry."""
    n, D = pos.shape
    idx = O.grid_indices(og, pos)
    pairs_per_sample = (1 << D) // 2
    spilled = 0
    for l in range(og.n_levels):
        entries = og.offsets[l + 1] - og.offsets[l]
        queues = -(-entries // slice_entries)
        capacity = -(-(2 * (n * pairs_per_sample // queues) + 512) // 64) * 64
        per_queue = np.bincount((idx[:, l, 0::2] // slice_entries).reshape(-1), minlength=queues)
        spilled += int(np.maximum(per_queue - capacity, 0).sum())
    return spilled


def must_overflow(og, kind, n, slice_entries=DEFAULT_SLICE_ENTRIES):
    """Cases in which a full queue is certain, reasoned from the plan alone: all samples in one cell put the n * P pairs of a level (P pairs
    per sample) into at most P queues, so one queue is offered at least n pairs -- against a capacity of twice the UNIFORM share + 512.  That
    is certain to overflow where n exceeds the capacity: here at n = 4096 on a level with more than two queues (the 64^3 level of the dense
    table at D = 3; the hashed table only with slices smaller than the default, which the emulator's test adds).  The 512 pairs of slack
    keep every smaller batch of the list inside its queues, and a level with one or two queues has room for everything by construction."""
    if kind != "one_cell":
        return False
    pairs_per_sample = (1 << og.n_dims) // 2
    for l in range(og.n_levels):
        queues = -(-(og.offsets[l + 1] - og.offsets[l]) // slice_entries)
        capacity = -(-(2 * (n * pairs_per_sample // queues) + 512) // 64) * 64
        if n > capacity:
            return True
    return False

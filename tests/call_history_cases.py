"""Shapes, inputs and CPU-side arithmetic of tests/test_gpu_call_history.py: a call's result must not depend on the calls before it.

A PROBE is one fixed call on fixed inputs; a HISTORY is a short fixed list of other calls that dirty the state the host layer keeps
between calls (the scratch cache's recycled blocks, the zeroed queue / overflow counters, forward contexts that own blocks, the
process-wide switches).  This module is a helper, not a test: it holds what can be stated without a GPU, and
tests/test_call_history_cases.py checks on the CPU that the inputs have the properties the GPU test relies on.

Grid probes (G16, G32, G2) use the "hashed" table of tests/scatter_owner_cases.py at D = 3 (8 levels, T = 2^14, F = 2: level 0 is dense,
the others hashed into two queues each), n = 513 padded to 768 rows whose dL/dy is zero:
  * G16: uniform positions, make_dy (every other row small enough for subnormal products), random 16-bit parameters;
  * G32 / G2: positions on multiples of 1/4 and dL/dy (and dL/d(dL/dinput)) in {-1, -1/2, 0, 1/2, 1}.  With scales 15, 31, .., 2047 and the
    half-cell shift, x * scale + 1/2 has a fraction in {0, 1/4, 1/2, 3/4}: every weight is a multiple of 1/64, every first-order term
    weight * dL/dy a multiple of 2^-7, every second-order term scale * ddx * (a product of two weights) * dL/dy a multiple of 2^-6.  An entry's
    sum of |terms| divided by that unit stays below 2^24 (exact_grid_sums / exact_second_order_sums compute it from the data), so every
    partial sum in any order is an fp32 number and the fp32 atomics give the same bits in every order.
Network probes (W, L16, L32) take the dyadic inputs of tests/exact_network_cases.py and tests/exact_f32_network_cases.py: their clean result
is the float64 restatement's bits, no tolerance involved.  The calls of a history (another batch size, another seed) are not audited: only
the probe's result is compared.

The plans the histories rely on, from tests/scatter_owner_cases.py's restatement of make_backward_plan:
  * OTHER_PLAN: the "dense" table at D = 2 -- 3 levels of 17^2, 33^2, 65^2 entries, one queue each, overflow counter at index 3 -- against the
    probe's 8 levels with 1 + 7 * 2 queues, overflow counter at index 15: the two plans lay their counters out differently in ONE buffer.
    Both need far fewer than the 4096 counters a counter buffer holds at least, so these two share one buffer and never regrow it.
  * GROW_PLAN: what does regrow it -- ZeroedCounters::get's free-and-reallocate branch.  A plan's counters are its queues, the overflow
    counter and the finished-blocks counter, rounded up to an even index, then 2 * LEVEL_SUM_PARTS * MAX_BUCKET_LEVELS = 512 level-sum
    words (n_counters below).  8 levels at base resolution 256 with T = 2^22 and F = 2 are all hashed, 2^22 / 8192 = 512 queues each:
    4096 queues, 4610 counters > 4096, 128 MiB of 16-bit parameters, one sample chunk per queue at n = 1024.
  * OVERFLOW: one_cell, n = 4096, D = 3, "dense": K.must_overflow is true (the 65^3 level has 34 queues of capacity 1536 < 4096 pairs offered
    to one of them) and K.spilled_pairs counts the pairs that go through the overflow list."""
from dataclasses import replace

import numpy as np

import exact_f32_network_cases as F
import exact_mlp_second_order_cases as X
import exact_network_cases as E
import grid_second_order_f32_reference as S
import scatter_owner_cases as K
from oracle import oracle as O

BIG = 4096                      # the largest batch of any call
GRID_D, GRID_TABLE = 3, "hashed"
GRID_N, GRID_PADDED = 513, 768
GRID_NEAR = 1000              # padded to 1024: blocks of at most twice the probe's, which the scratch cache hands to the probe
OTHER_PLAN = dict(D=2, table="dense", n=513, padded=768)
OVERFLOW = dict(D=3, table="dense", n=4096, kind="one_cell")
GROW_PLAN = dict(D=3, n=1024, n_levels=8, log2_hashmap_size=22, base_resolution=256)
COUNTER_BUFFER_FLOOR = 4096     # ZeroedCounters::get: the smallest buffer, in counters
LEVEL_SUM_PARTS, MAX_BUCKET_LEVELS = 8, 32  # csrc/grid_backward_plan.h
TRAINER_N = 1024
LADDER = [256, BIG, TRAINER_N, BIG, TRAINER_N]
NE_N = 768


# ---- grids -----------------------------------------------------------------------------------------------------------------------------
def padded(n):
    return (n + 255) // 256 * 256


def grid_half_data(n, D=GRID_D, table=GRID_TABLE, kind="uniform", seed=3):
    """-> og, positions [padded][D] f32, dL/dy bits [padded][L*F] (rows >= n zero), parameter bits"""
    og = K.oracle_grid(D, table)
    width = og.n_levels * K.F
    pos = np.zeros((padded(n), D), np.float32)
    pos[:n] = K.make_positions(kind, n, D, seed=seed)
    if kind == "one_cell":
        pos[n:] = pos[0]
    dy = np.zeros((padded(n), width), np.uint16)
    dy[:n] = K.make_dy(n, width, seed=seed + 1)
    params = O.f2h((np.random.default_rng(seed + 2).random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    return og, pos, dy, params


def grid_exact_data(n, seed=5):
    """-> og, positions on multiples of 1/4, dL/dy and ddx in {-1, -1/2, 0, 1/2, 1} (rows >= n of dL/dy zero), fp32 parameters"""
    og = K.oracle_grid(GRID_D, GRID_TABLE)
    width = og.n_levels * K.F
    r = np.random.default_rng(seed)
    pos = (r.integers(0, 4, size=(padded(n), GRID_D)).astype(np.float32) * np.float32(0.25)).astype(np.float32)
    dy = np.zeros((padded(n), width), np.float32)
    dy[:n] = r.integers(-2, 3, size=(n, width)).astype(np.float32) * np.float32(0.5)
    ddx = (r.integers(-2, 3, size=(padded(n), GRID_D)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    params = r.uniform(-0.5, 0.5, og.n_params).astype(np.float32)
    return og, pos, dy, ddx, params


def exact_grid_sums(og, pos, dy):
    """first-order fp32 parameter gradient: (log2 of the unit every term is a multiple of, largest sum|terms| / unit) -- the sums are
    order-independent in fp32 when the second figure is below 2^24"""
    _, w = O.grid_indices(og, pos, with_weights=True)
    terms = w.astype(np.float64)[:, :, :, None] * dy.astype(np.float64).reshape(pos.shape[0], og.n_levels, 1, og.n_features_per_level)
    assert np.array_equal(terms.astype(np.float32).astype(np.float64), terms)
    lsb = next(k for k in range(64) if np.array_equal(np.rint(terms * 2.0 ** k), terms * 2.0 ** k))
    abs_sums = O.grid_backward_f32(og, pos, np.abs(dy))
    return -lsb, float(abs_sums.max() * 2.0 ** lsb), w


def exact_second_order_sums(og, ref, unit_log2=-6):
    """second-order fp32 parameter gradient of the restatement `ref` (grid_second_order_f32_reference.second_order): every entry a multiple
    of 2^unit_log2 (checked on the sums), largest sum|terms| / unit"""
    scaled = ref.dL_dparams * 2.0 ** -unit_log2
    assert np.array_equal(np.rint(scaled), scaled), "a second-order sum is no multiple of the unit"
    return float(ref.mag_p.max() * 2.0 ** -unit_log2)


def second_order_reference(og, pos, dy, ddx, params):
    _, dy_dx = O.grid_forward_f32(og, params, pos, want_dy_dx=True)
    return S.second_order(og, params, pos, ddx, dy, dy_dx=dy_dx)


def k_x(og):
    """the dL_dinput constant of tests/second_order_f32_cases.py's docstring, K_x = n_levels * 2^D * D + 40, at THIS grid's level count"""
    return og.n_levels * (1 << og.n_dims) * og.n_dims + 40


def overflow_case():
    """the history that provably touches the overflow counter: asserts the plan arithmetic BEFORE anything is launched"""
    c = OVERFLOW
    og, pos, dy, params = grid_half_data(c["n"], c["D"], c["table"], c["kind"])
    assert K.must_overflow(og, c["kind"], c["n"]), "the overflow history does not fill a queue"
    spilled = K.spilled_pairs(og, pos[:c["n"]])
    assert spilled > 0, "the overflow history spills no pair"
    return og, pos, dy, params, spilled


def queue_layout(og, n):
    """(queues per level, index of the overflow counter) by make_backward_plan's rule at these sizes (one sample chunk per queue)"""
    queues = [-(-(og.offsets[l + 1] - og.offsets[l]) // K.DEFAULT_SLICE_ENTRIES) for l in range(og.n_levels)]
    return queues, int(sum(queues))


def n_counters(og):
    """make_backward_plan's n_counters: queues, overflow counter, finished-blocks counter, up to an even index, then the level-sum words"""
    _, overflow = queue_layout(og, 0)
    return ((overflow + 2 + 1) & ~1) + 2 * LEVEL_SUM_PARTS * MAX_BUCKET_LEVELS


def grow_plan_config():
    c = GROW_PLAN
    return {"otype": "HashGrid", "n_levels": c["n_levels"], "n_features_per_level": K.F, "log2_hashmap_size": c["log2_hashmap_size"],
            "base_resolution": c["base_resolution"], "per_level_scale": K.SCALE}


def grow_plan_grid():
    c = GROW_PLAN
    return O.grid_init(c["D"], c["n_levels"], K.F, c["log2_hashmap_size"], c["base_resolution"], K.SCALE, O.GRID_HASH, O.INTERP_LINEAR)


# ---- networks --------------------------------------------------------------------------------------------------------------------------
W_CASE = E.by_name("fused-128x4").at(512)          # FullyFusedMLP 128 x 4: the LDS-resident-weights kernel
L16_CASE = E.by_name("general-256x2-n768")         # CutlassMLP 32 -> 256 x 2 -> 4: slabs + finalize
L32_CASE = E.Case("f32-48x1", 16, 48, 3, 1, seed=45, **F._F, **F.FINE).at(256)  # fp32 network 16 -> 48 x 1 -> 3


def other(case, n=None):
    """the case of a history call: another batch size and / or other values (not audited, never compared with a restatement)"""
    return replace(case, n=n or case.n, seed=case.seed + 100, name=f"{case.name}-other{n or ''}")


def network_probe_audits():
    """{probe: (description, passes)} of the dyadic probes, by their case files' own audits"""
    out = {}
    for name, case in (("W", W_CASE), ("L16", L16_CASE)):
        fig = E.audit(case, E.generate(case))
        out[name] = (E.describe(case, fig), E.audit_passes(fig))
    data = X.generate(L32_CASE)
    fig = F.audit(L32_CASE, data)
    out["L32"] = (F.describe(L32_CASE, fig), F.audit_passes(fig))
    fig = X.audit(L32_CASE, data)
    out["L32 second order"] = (X.describe(L32_CASE, fig), X.audit_passes(fig))
    return out


# ---- trainer ---------------------------------------------------------------------------------------------------------------------------
def positions(n, d, seed):
    return O.generate_random_uniform(O.pcg32(seed), n * d, 0.0, 1.0).reshape(n, d)


def targets_for(pos, out):
    return np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c + 1) * pos[:, 0]) * np.cos(2 * np.pi * pos[:, 1]) for c in range(out)], 1).astype(np.float32)


def trainer_batch(n):
    """the probe's batch at n == TRAINER_N (seed 21, as test_training_step_matches_oracle), another one at every other size"""
    pos = positions(n, 3, seed=21 if n == TRAINER_N else 21 + n)
    return pos, targets_for(pos, 4)


# ---- reporting -------------------------------------------------------------------------------------------------------------------------
def difference(history, probe, name, got, want, level_offsets=None):
    """'' if the two bit arrays are equal; else history, probe, tensor, the count of differing entries, for grid parameters the count per
    level (level_offsets: first VALUE of every level, n_levels + 1 numbers), and the first few (index, got, want)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"history {history}, probe {probe}, {name}: shape {got.shape} != {want.shape}"
    if np.array_equal(got, want):
        return ""
    bad = got != want
    text = f"history {history}, probe {probe}, {name}: {int(bad.sum())} of {got.size} entries differ"
    if level_offsets is not None:
        flat = bad.reshape(-1)
        text += f" (per level {[int(flat[level_offsets[l]:level_offsets[l + 1]].sum()) for l in range(len(level_offsets) - 1)]})"
    idx = np.argwhere(bad)[:6]
    return text + "; first: " + "; ".join(f"{tuple(int(j) for j in i)}: got 0x{int(got[tuple(i)]):x} want 0x{int(want[tuple(i)]):x}" for i in idx)

"""The bfloat16 build of the kernel sources (-DTCNN_BF16, what libtcnn_hip_bf16.so is compiled from) on the host SIMT emulator
(tests/emu/libtcnn_emu_bf16.so) against the oracle's bfloat16 mode.  The case tables are those of tests/test_emu_kernels.py.

Every bar below is derived from the number formats and the arithmetic the path performs, or measured oracle-vs-float64; none
comes from the kernels' own output.  Notation: u = 2^-9, the unit the bars are written in; bfloat16 has 8 significant bits, so ONE
rounding to nearest moves a value by up to half a unit in the last place = 2^-8 of its magnitude = 2 u (f2h(ref) itself is that far
from ref at a tie).  `absacc` is the oracle's backward of |dL/dy| (the sum of the magnitudes an entry accumulated), N_e the number of
records of an entry.

The fixed-point rule the bucketed backward documents (grid_backward_plan.h, OwnerScale): a record v enters a slice's sum as
round(v * 2^k), k = 30 - ceil(log2(8 * share)) clamped to 20..40, share = (level's sum of min(|record magnitude per sample|, 4096))
/ (slices x chunks of the level).  `owner_k` restates that rule from the test's inputs and the host plan's slice counts; at most
half a unit 2^-k is lost per record: floor_e = N_e * 2^-(k+1).
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O

emu = pytest.importorskip("emu")
if not emu.available():
    pytest.skip("ROCm clang++ not available to build the host emulator", allow_module_level=True)

import test_emu_kernels as K  # noqa: E402  (the case tables and the type-independent tests)

from bf16_bars import ONE_ROUNDING, TINY, absf, level_k, max_abs_per_level, owner_k, record_counts, second_order_magnitudes, spread  # noqa: E402


@pytest.fixture(autouse=True, scope="module")
def _bf16_everywhere():
    """The oracle's 16-bit format is a process-wide switch and emu.py calls one library at a time: both to bfloat16 for this module."""
    O.set_half_format(True)
    previous = emu.set_bf16(True)
    yield
    emu.set_bf16(previous)
    O.set_half_format(False)


def floors(g, og, pos, per_sample_magnitude, lds_budget=0, mode=None, accumulate=False):
    """(floor_e, N_e, k per level, plan) for a backward call.  per_sample_magnitude [n, L]: what a sample contributes to its level's
    sum.  The plan -- kind, table slices and sample chunks per level -- is the library's host plan for the same call (mode, Accumulate or
    Overwrite, LDS budget), read through the driver.  Levels that are not bucketed use IEEE-style fixed point at k = 24 or floating
    point: 2^-25 per record there."""
    mode = emu.BUCKETED if mode is None else mode
    plan = emu.grid_backward_plan(g, pos.shape[0], mode=mode, accumulate=accumulate, lds_budget=lds_budget) if mode != emu.ATOMIC else np.zeros((og.n_levels, 3), np.uint32)
    counts = record_counts(og, pos)
    ks = [level_k(per_sample_magnitude[:, l], int(plan[l, 1]) * int(plan[l, 2])) if mode == emu.BUCKETED and plan[l, 0] == emu.PLAN_BUCKET else 24
          for l in range(og.n_levels)]
    return counts * spread(og, [2.0 ** -(k + 1) for k in ks]), counts, ks, plan


# ---------------------------------------------------------------------------------------------------------------------
# single device functions
# ---------------------------------------------------------------------------------------------------------------------
def bf_value(bits):
    return O.h2f(np.array([bits], dtype=np.uint16)).astype(np.float64)[0]


def rne_bf16_exact(q):
    """Fraction -> bfloat16 bits with ONE round-to-nearest-even, in rational arithmetic."""
    if q == 0:
        return 0
    sign = 0x8000 if q < 0 else 0
    q = abs(q)
    e = max(math.floor(math.log2(q)) if q >= Fraction(2) ** -126 else -126, -126)
    while Fraction(2) ** (e + 1) <= q:
        e += 1
    while e > -126 and Fraction(2) ** e > q:
        e -= 1
    unit = Fraction(2) ** (e - 7)
    m = q / unit
    lo = m.numerator // m.denominator
    rest = m - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    value = lo * unit
    if value >= Fraction(2) ** 128:
        return sign | 0x7F80
    if lo < 128:  # subnormal (e == -126)
        return sign | lo
    if lo == 256:
        e, lo = e + 1, 128
    return sign | ((e + 127) << 7) | (lo - 128)


def test_packed_atomic_add_rounds_once():
    """The emulator's packed bfloat16 atomic add is the exact sum rounded ONCE to nearest even -- ties, near-ties one fp32 / fp64 bit
    off a tie (where rounding through fp32 or fp64 first would land on the tie and go the other way), subnormals, overflow -- against
    rational arithmetic."""
    rng = np.random.default_rng(0)
    a = rng.integers(0, 0x7F80, 300).astype(np.uint16) | (rng.integers(0, 2, 300).astype(np.uint16) << 15)
    b = a ^ rng.integers(0, 0x0800, 300).astype(np.uint16) ^ (rng.integers(0, 2, 300).astype(np.uint16) << 15)  # exponents at most 16 apart: the sums do round
    b = np.where((b & 0x7F80) == 0x7F80, a, b).astype(np.uint16)  # (no Inf / NaN operands)
    # crafted: 1 + 2^-8 (tie -> 1), 1 + 2^-8 + 2^-8 * 2^-7 (just above), (1 + 2^-7) + 2^-8 (tie -> even: up), ties broken by a third far bit
    one, tie = 0x3F80, 0x3B80  # 1.0, 2^-8
    crafted = [(one, tie), (one, tie + 1), (one + 1, tie), (one, 0x3B7F), (0x7F7F, 0x7F7F), (0x7F7F, 0x7380), (0x0001, 0x0001), (0x0001, 0x8001),
               (0x007F, 0x0001), (one, 0x8000 | tie), (one + 1, 0x8000 | tie), (0x4780, 0x3B80 + 3)]
    # near-ties further apart than fp32's 24 bits: 2^e + (2^(e-8) +- 2^(e-8-30)) cannot be written as one bfloat16 operand, but
    # big + small where small sits just off the tie of big can: big = 2^20 (ulp 2^13, tie 2^12), small = 2^12 * (1 +- 2^-7)
    crafted += [(0x4980, 0x4580), (0x4980, 0x4581), (0x4980, 0x457F), (0x4981, 0x457F), (0x4981, 0x4580)]
    a = np.concatenate([a, np.array([c[0] for c in crafted], np.uint16)])
    b = np.concatenate([b, np.array([c[1] for c in crafted], np.uint16)])
    got = emu.atomic_add_h2(a, b)
    for i in range(a.size):
        want = rne_bf16_exact(Fraction(bf_value(a[i])) + Fraction(bf_value(b[i])))
        if want & 0x7FFF == 0:  # +-0: the sign of an exact zero sum is not at issue here
            assert got[i] & 0x7FFF == 0, (hex(a[i]), hex(b[i]))
        else:
            assert got[i] == want, (hex(a[i]), hex(b[i]), hex(got[i]), hex(want))


def test_fma_is_an_fp32_fma_rounded_to_bf16():
    """fma_h of the bfloat16 build: (bf16)fmaf(a, b, c) -- the product is exact in fp32 (8 x 8 bits), so fp32's rounding of a * b + c
    followed by the rounding to bfloat16 is what the device does; a product rounded to bfloat16 before the add differs."""
    rng = np.random.default_rng(1)
    a, b, c = (O.f2h(rng.standard_normal(20000).astype(np.float32)) for _ in range(3))
    fa, fb, fc = (O.h2f(v).astype(np.float64) for v in (a, b, c))
    want = O.f2h((fa * fb + fc).astype(np.float32))  # fp64 holds a * b + c of these exactly; fp32 rounding, then bfloat16
    got = emu.fma_h(a, b, c)
    assert np.array_equal(got, want)
    product_then_add = O.f2h(O.h2f(O.f2h((fa * fb).astype(np.float32))) + O.h2f(c))
    assert np.mean(product_then_add != want) > 0.05  # the comparison can tell the two apart


def test_level_sum_conversion_is_clamped_and_saturates():
    """level_sum_units: a workgroup's fp32 total -> 2^-32 units in 64 bits, clamped below 2^32 before the conversion; the sums saturate."""
    below = float(np.nextafter(np.float32(2.0 ** 32), np.float32(0)))
    top = int(below) << 32
    assert emu.level_sum_units(0.0) == 0
    assert emu.level_sum_units(float(np.float32(1e-45))) == 0  # one ulp above zero: below one unit
    assert emu.level_sum_units(2.0 ** -32) == 1 and emu.level_sum_units(1.0) == 1 << 32 and emu.level_sum_units(4096.0) == 4096 << 32
    assert emu.level_sum_units(below) == top
    assert emu.level_sum_units(2.0 ** 32) == top and emu.level_sum_units(float("inf")) == top and emu.level_sum_units(3.0e38) == top
    assert emu.level_sum_units(float("nan")) == 0 and emu.level_sum_units(-1.0) == 0
    m = (1 << 64) - 1
    assert emu.saturating_add_u64(top, top) == m and emu.saturating_add_u64(1 << 40, 3 << 40) == 4 << 40 and emu.saturating_add_u64(m - 5, 5) == m
    assert emu.saturating_add_u64(m - 5, 6) == m and emu.saturating_add_u64(m, m) == m and emu.saturating_add_u64(top << 0, m) == m


def test_level_sum_saturates_to_the_coarsest_exponent():
    """2^20 samples at the clamp would wrap a 64-bit sum of 2^-32 units to ZERO (k = 40: every record of 4096 and more beyond 64 bits,
    dropped).  Few samples cannot reach that through the kernel, so the pieces are chained as the kernel chains them: per-workgroup
    totals -> units -> saturating sum -> the rule."""
    units = emu.level_sum_units(4096.0 * 1024 * 1024)  # one workgroup's clamped total: 2^32 -> clamped
    total = 0
    for _ in range(8):
        total = emu.saturating_add_u64(total, units)
    total = emu.saturating_add_u64(total, units)
    assert total == (1 << 64) - 1
    assert owner_k(total / 2.0 ** 32, 64) == 20


# ---------------------------------------------------------------------------------------------------------------------
# grid: forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.GRID_CASES)
def test_grid_forward_bit_exact(case):
    """indices, features (both layouts) and dy_dx: the oracle's bits, including pos = 0 and pos = 1"""
    K.test_grid_forward_bit_exact(case)  # (asserts equality of bit patterns only: nothing in it depends on the type)


# ---------------------------------------------------------------------------------------------------------------------
# grid: backward
# ---------------------------------------------------------------------------------------------------------------------
def backward_bar(og, mode, plan, absacc, counts, floor):
    """|got - ref| <= c * u * (absacc + floor) + floor + TINY, c = 2 x the roundings to bfloat16 (2 u each) the path performs on a sum
    bounded by absacc, per level from the plan's kind and chunk count C; counted in roundings:
      bucketed level, one owner of the slice: exact integer sum, ONE rounding (int -> fp32 -> bf16)                      1
      bucketed level, C sample chunks: every chunk's partial sum rounded once (together <= u * absacc), then C packed
        atomics each rounding the running sum (<= absacc)                                                                1 + C
      fixed-point slices (small tables, every mode but ATOMIC) and SLICED_F32's fp32 slices: the product (16-bit weight) x dy is taken in fp32 WITHOUT
        the rounding to the 16-bit type that the reference's record has (1, of the records' magnitudes), the table adds
        exactly or with 2^-24 per add (N_e * 2^-15 roundings), one rounding at the flush, C more if chunks meet in atomics   2 + N_e 2^-15 (+ C)
      packed 16-bit slices (SLICED_F16), levels sent through global atomics, and mode ATOMIC: one rounding of the running
        sum per record, one for a flush                                                                                  N_e + 1 (+ C)"""
    per_level_const, per_record = [], []
    for l in range(og.n_levels):
        kind, chunks = int(plan[l, 0]), max(1, int(plan[l, 2]))
        more = chunks if chunks > 1 else 0
        if mode == emu.BUCKETED and kind == emu.PLAN_BUCKET:
            per_level_const.append(1.0 + more); per_record.append(0.0)
        elif mode != emu.ATOMIC and (kind == emu.PLAN_FIXED64 or (kind == emu.PLAN_FLOAT and mode == emu.SLICED_F32)):
            per_level_const.append(2.0 + more); per_record.append(2.0 ** -15)
        else:
            per_level_const.append(1.0 + more); per_record.append(1.0)
    c = spread(og, per_level_const) + spread(og, per_record) * counts
    return c * ONE_ROUNDING * (absacc + floor) + floor + TINY


def sole_owner(og, plan):
    return bool(np.all(plan[:, 2] <= 1))


BACKWARD_MODES = [(emu.SLICED_F32, 0), (emu.SLICED_F16, 0), (emu.ATOMIC, 0), (emu.ATOMIC, 48 * 1024), (emu.BUCKETED, 0), (emu.BUCKETED, 1024)]


# (the atomic A/B mode needs F >= 2: the fp16 module skips those two combinations, here they are not generated)
@pytest.mark.parametrize("case,mode,lds_budget", [(c, m, b) for m, b in BACKWARD_MODES for c in K.GRID_CASES + [(3, 4, 2, 16, 16, 2.0, O.GRID_HASH, O.INTERP_LINEAR)]
                                                  if not (m == emu.ATOMIC and c[2] == 1)])
def test_grid_backward(case, mode, lds_budget):
    """All four modes, Overwrite into a garbage-filled buffer and Accumulate, against the oracle with the scale-free bar of
    backward_bar().  (Sixteen levels of 1 KiB slices are run with 4 KiB slices, as in the fp16 module: a minute of emulation otherwise.)

    BUCKETED with one owner per slice is ONE rounding of the exact sum of the quantised records: got == f2h(ref) except where the
    quantisation (or the fp32 step of the int -> fp32 -> bf16 conversion) moves a sum across a rounding boundary.  Measured on the
    emulator against the oracle over the even-F cases of this test: 0 ... 1.8 % of the entries differ (worst: the F = 4 Smoothstep case,
    share equal 0.9821; the 16-level hash cases 0.9967 and 0.9995) -- N(0, 1) gradients put every level at the coarsest exponent, k = 20,
    and sums of many records collect their half-units.  The bar is ten times the worst measured share of mismatches: 82 % equal."""
    D, L, F, T, base, scale, gtype, interp = case
    rng = np.random.default_rng(1)
    og = O.grid_init(D, L, F, T, base, scale, gtype, interp)
    g = emu.Grid(og)
    n = 1500 if lds_budget == 0 else 700
    if lds_budget == 1024 and L > 8:
        lds_budget = 4096
    pos = rng.random((n, D), dtype=np.float32)
    dy = O.f2h(rng.standard_normal((n, L * F)).astype(np.float32))
    ref = O.grid_backward(og, pos, dy)
    absacc = O.grid_backward(og, pos, absf(dy))
    dys = np.ascontiguousarray(dy.T)
    floor, counts, ks, plan = floors(g, og, pos, max_abs_per_level(dy, L, F), lds_budget, mode=mode)
    bar = backward_bar(og, mode, plan, absacc, counts, floor)
    got = emu.grid_backward(g, pos, dys, soa=True, mode=mode, lds_budget=lds_budget)
    gotf = O.h2f(got).astype(np.float64)
    err = np.abs(gotf - ref)
    print("worst |err| / bar:", float((err / bar).max()), "k per level:", ks)
    assert np.all(err <= bar)
    assert not np.any((gotf == 0) & (np.abs(ref) > bar))  # no finite gradient comes back as zero unless inside the bar
    if mode == emu.BUCKETED and F > 1 and lds_budget == 0 and sole_owner(og, plan):
        share_equal = np.mean(got == O.f2h(ref.astype(np.float32)))
        print("share of entries equal to f2h(ref):", share_equal)
        assert share_equal > 1 - 10 * 0.0179
    acc = emu.grid_backward(g, pos, dys, soa=True, mode=mode, lds_budget=lds_budget, grad_init=got)
    # Accumulate (its own plan: chunked levels are not zeroed first): the first pass's error, the second one's, and one rounding of the
    # sum of the two (<= 2 absacc) where a sole owner adds old + new; where atomics add into the old value its bar holds for a running
    # sum of up to 2 absacc instead of absacc: twice it
    floor2, _, _, plan2 = floors(g, og, pos, max_abs_per_level(dy, L, F), lds_budget, mode=mode, accumulate=True)
    bar2 = backward_bar(og, mode, plan2, absacc, counts, floor2)
    assert np.all(np.abs(O.h2f(acc).astype(np.float64) - 2 * ref) <= bar + 2 * bar2 + 2 * ONE_ROUNDING * (absacc + floor))


SWEEP = [2.0 ** -100, 2.0 ** -40, 3e-3, 2.0, 300.0, 2.0 ** 12, 2.0 ** 20, "mixed"]


@pytest.mark.parametrize("case,lds_budget", [((3, 4, 2, 14, 8, 1.7, O.GRID_HASH, O.INTERP_LINEAR), 0), ((3, 4, 4, 12, 8, 1.7, O.GRID_HASH, O.INTERP_LINEAR), 2048),
                                             ((2, 4, 8, 11, 4, 1.5, O.GRID_HASH, O.INTERP_SMOOTHSTEP), 0), ((3, 3, 2, 19, 4, 1.4, O.GRID_DENSE, O.INTERP_LINEAR), 2048)])
@pytest.mark.parametrize("magnitude", SWEEP, ids=[str(m) for m in SWEEP])
def test_grid_bucket_owner_forms_agree_over_the_range(case, magnitude, lds_budget):
    """The cases of test_grid_bucket_owner_forms_agree across bfloat16's range: dL/dy ~ N(0, 1) times 2^-100 ... 2^20 (2^12 is the
    per-sample clamp of the level sum), and a mixed batch -- 1 % of the samples at 2^10, the rest at 2^-20 -- in which slices exist that
    hold small records only.  The three owner forms give the same BITS; the result meets the one-rounding bar with the floor of the
    documented rule (so at 2^-100, where every record is below half a unit even at k = 40, zeros are inside the floor -- and nowhere
    else may a finite oracle gradient come back as zero)."""
    D, L, F, T, base, scale, gtype, interp = case
    rng = np.random.default_rng(11)
    og = O.grid_init(D, L, F, T, base, scale, gtype, interp)
    g = emu.Grid(og)
    n = 600
    pos = rng.random((n, D), dtype=np.float32)
    z = rng.standard_normal((n, L * F))
    if magnitude == "mixed":
        factor = np.where(np.arange(n) % 100 == 0, 2.0 ** 10, 2.0 ** -20)[:, None]
    else:
        factor = magnitude
    dy = O.f2h((z * factor).astype(np.float32))
    dys = np.ascontiguousarray(dy.T)
    got = [emu.grid_backward(g, pos, dys, soa=True, mode=emu.BUCKETED, lds_budget=lds_budget, owner=o) for o in (emu.OWNER_PACKED, emu.OWNER_FIXED64, emu.OWNER_WIDE)]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[1])
    ref = O.grid_backward(og, pos, dy)
    absacc = O.grid_backward(og, pos, absf(dy))
    floor, counts, ks, plan = floors(g, og, pos, max_abs_per_level(dy, L, F), lds_budget)
    assert sole_owner(og, plan)
    bar = backward_bar(og, emu.BUCKETED, plan, absacc, counts, floor)
    gotf = O.h2f(got[0]).astype(np.float64)
    print("k per level:", ks, "worst |err| / bar:", float((np.abs(gotf - ref) / bar).max()))
    assert np.all(np.isfinite(gotf)) and np.all(np.abs(gotf - ref) <= bar)
    assert not np.any((gotf == 0) & (np.abs(ref) > floor * (1 + ONE_ROUNDING) + TINY))
    acc = [emu.grid_backward(g, pos, dys, soa=True, mode=emu.BUCKETED, lds_budget=lds_budget, grad_init=got[0], owner=o) for o in (emu.OWNER_PACKED, emu.OWNER_FIXED64)]
    assert np.array_equal(acc[0], acc[1])


def test_grid_backward_record_range_edge():
    """The documented range of the bfloat16 bucketed backward (include/tcnn_hip.h, OwnerScale in grid_backward_plan.h): a record whose scaled
    value |v| * 2^k reaches 9e18 cannot enter a 64-bit sum and is dropped; k >= 20, so every record below 2^42 is carried.  One sample in
    the middle of a cell (all four corner weights 1/4, four distinct entries): dL/dy = 2^43 gives records of 2^41 -- carried exactly;
    dL/dy = 2^46 gives records of 2^44 = 2^64 units at k = 20 -- dropped: the entries read zero (not Inf, not garbage), in all three
    owner forms."""
    D, L, F = 2, 1, 2
    og = O.grid_init(D, L, F, 12, 8, 1.0, O.GRID_HASH, O.INTERP_LINEAR)
    g = emu.Grid(og)
    res = og.resolution[0]
    cell = (np.array([[2.5, 3.5]]) - 0.5) / float(og.scale[0])
    pos = cell.astype(np.float32)
    assert emu.grid_backward_plan(g, 1)[0, 0] == emu.PLAN_BUCKET and res >= 4
    for e, dropped in ((43, False), (46, True)):
        dy = O.f2h(np.array([[2.0 ** e, -(2.0 ** e)]], dtype=np.float32))
        ref = O.grid_backward(og, pos, dy)
        assert np.count_nonzero(ref) == 8 and np.allclose(np.abs(ref[ref != 0]), 2.0 ** (e - 2), rtol=2.0 ** -6)
        k = owner_k(4096.0, int(np.prod(emu.grid_backward_plan(g, 1)[0, 1:])))
        assert k == 20 and (2.0 ** (e - 2 + k) >= 9.0e18) == dropped
        for o in (emu.OWNER_PACKED, emu.OWNER_FIXED64, emu.OWNER_WIDE):
            got = O.h2f(emu.grid_backward(g, pos, np.ascontiguousarray(dy.T), soa=True, mode=emu.BUCKETED, owner=o)).astype(np.float64)
            if dropped:
                assert not got.any()
            else:
                assert np.all(np.abs(got - ref) <= ONE_ROUNDING * np.abs(ref))


@pytest.mark.parametrize("ddx_scale", [1.0, 1e-4, 1e3])
@pytest.mark.parametrize("case", [K.GRID_CASES[i] for i in (0, 1, 2, 4, 5, 6)])
def test_grid_second_order(case, ddx_scale):
    """d(dL_dx)/d(grid) in bfloat16 with ddx ~ N(0, 1) times 1, 1e-4 (eikonal-sized) and 1e3.  The records are dy * weight with
    weight = scale * sum_d +-ddx_d * pos'_d * prod_{e != d} w_e: their size follows ddx * scale, not dL/dy, and so must absacc and the
    floor (second_order_magnitudes: the level sum of the rule is taken from the records, max_f |dy| * sum over the corners of |weight|).
    Roundings, each at most 2 u of a magnitude bounded by absacc: the kernel rounds a corner's fp32 weight and then the product with dy
    (2); the oracle, like the reference, rounds each of the D terms and each term's product with dy (2, of the terms' magnitudes); one
    for the owner's sum: c = 2 x 5.  d(dL_dx)/d(dL_dy) bit-exact, d(dL_dx)/dx to fp32 rounding as in the fp16 module."""
    D, L, F, T, base, scale, gtype, interp = case
    rng = np.random.default_rng(8)
    og = O.grid_init(D, L, F, T, base, scale, gtype, interp)
    g = emu.Grid(og)
    n = 700
    pos = rng.random((n, D), dtype=np.float32)
    params = O.f2h(((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5))
    dy = O.f2h(rng.standard_normal((n, L * F)).astype(np.float32))
    ddx = (rng.standard_normal((n, D)) * ddx_scale).astype(np.float32)
    _, dydx = O.grid_forward(og, params, pos, want_dy_dx=True)
    gp_ref, dLddy_ref, dx_ref = O.grid_backward_backward_input(og, params, pos, ddx, dy, dy_dx=dydx)
    grad, dLddy, dx = emu.grid_backward_backward(g, pos, ddx, np.ascontiguousarray(dy.T), params, np.ascontiguousarray(np.transpose(dydx, (1, 0, 2))))
    assert np.array_equal(dLddy.T, dLddy_ref)
    assert np.allclose(dx, dx_ref, rtol=1e-4, atol=1e-4 * max(ddx_scale, np.abs(dx_ref).max()))
    gotf = O.h2f(grad).astype(np.float64)
    if interp == O.INTERP_NEAREST:
        assert not gotf.any() and not gp_ref.any()
        return
    absacc, per_sample = second_order_magnitudes(og, pos, ddx, dy)
    assert np.all(np.abs(gp_ref) <= absacc * (1 + 2.0 ** -6) + TINY)  # the helper's magnitudes do bound the oracle's sums
    floor, counts, ks, _ = floors(g, og, pos, per_sample)
    bar = 5 * ONE_ROUNDING * (absacc + floor) * (1 + 1e-5) + floor + TINY
    err = np.abs(gotf - gp_ref)
    print("k per level:", ks, "worst |err| / bar:", float((err / bar).max()))
    assert np.all(err <= bar)
    assert not np.any((gotf == 0) & (np.abs(gp_ref) > bar))


def test_grid_backward_bucket_overflow():
    """test_grid_backward_bucket_overflow's clustered batch: queues overflow, the overflow list (picked up by the owners, exact) keeps
    the sums right: the one-owner bar, c = 1."""
    D, L, F, T = 3, 3, 2, 14
    rng = np.random.default_rng(5)
    og = O.grid_init(D, L, F, T, 16, 2.0, O.GRID_HASH, O.INTERP_LINEAR)
    g = emu.Grid(og)
    n = 2048
    pos = np.tile(np.array([[0.3137, 0.6211, 0.1173]], np.float32), (n, 1))
    pos[: n // 8] = rng.random((n // 8, D), dtype=np.float32)
    dy = O.f2h((rng.standard_normal((n, L * F)) * 0.05).astype(np.float32))
    ref = O.grid_backward(og, pos, dy)
    absacc = O.grid_backward(og, pos, absf(dy))
    floor, counts, ks, plan = floors(g, og, pos, max_abs_per_level(dy, L, F), 512)
    bar = backward_bar(og, emu.BUCKETED, plan, absacc, counts, floor)
    got = O.h2f(emu.grid_backward(g, pos, np.ascontiguousarray(dy.T), soa=True, mode=emu.BUCKETED, lds_budget=512)).astype(np.float64)
    assert np.count_nonzero(ref) > 0 and np.all(np.abs(got - ref) <= bar)


def test_grid_backward_bucket_chunks():
    """test_grid_backward_bucket_chunks in bfloat16: several owners per slice meet in packed bfloat16 atomics, c = 1 + chunks."""
    D, L, F = 3, 2, 2
    rng = np.random.default_rng(6)
    og = O.grid_init(D, L, F, 12, 4, 2.0, O.GRID_HASH, O.INTERP_LINEAR)
    g = emu.Grid(og)
    n = 20000
    pos = rng.random((n, D), dtype=np.float32)
    dy = O.f2h((rng.standard_normal((n, L * F)) * 0.05).astype(np.float32))
    ref = O.grid_backward(og, pos, dy)
    absacc = O.grid_backward(og, pos, absf(dy))
    dys = np.ascontiguousarray(dy.T)
    floor, counts, ks, plan = floors(g, og, pos, max_abs_per_level(dy, L, F))
    assert plan[:, 2].max() > 1
    chunks = spread(og, plan[:, 2].astype(np.float64))
    bar = backward_bar(og, emu.BUCKETED, plan, absacc, counts, floor)
    got = emu.grid_backward(g, pos, dys, soa=True, mode=emu.BUCKETED)
    assert np.all(np.abs(O.h2f(got).astype(np.float64) - ref) <= bar)
    acc = emu.grid_backward(g, pos, dys, soa=True, mode=emu.BUCKETED, grad_init=got)
    assert np.all(np.abs(O.h2f(acc).astype(np.float64) - 2 * ref) <= 2 * bar + chunks * 2 * ONE_ROUNDING * (absacc + floor))


# ---------------------------------------------------------------------------------------------------------------------
# network kernels
# ---------------------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def same_weight_gradients(a, b):
    """as K.same_weight_gradients with bfloat16's spacing: equal up to the last bit (2^-7 relative) of a few entries"""
    fa, fb = O.h2f(a).astype(np.float64), O.h2f(b).astype(np.float64)
    return np.mean(a != b) < 0.05 and np.all(np.abs(fa - fb) <= 2.0 ** -7 * np.abs(fb) + 2.0 ** -7 * np.abs(fb).max() * 2.0 ** -10)


@pytest.mark.parametrize("case", K.MLP_CASES)
def test_mlp_forward_backward(case):
    """The bars tests/bf16_cases.py states for the same comparison on the GPU: outputs and activations RAE p99 < 3e-2, gradients
    relative L2 < 2e-2 (entry-wise RAE p99 < 3e-2 for up to two hidden layers); inference == forward bit for bit."""
    IN, W, OUT, H = case
    rng = np.random.default_rng(2)
    om = O.mlp_init(IN, W, OUT, H)
    ph = O.f2h(O.mlp_init_params(om, O.pcg32(1337)))
    n = 256
    x = O.f2h(rng.random((n, IN), dtype=np.float32))
    xs = np.ascontiguousarray(x.T)
    hid_ref, out_ref = O.mlp_forward(om, ph, x)
    hid, out = emu.mlp_forward(om, ph, xs)
    assert np.percentile(K.rae(O.h2f(out)[:, :OUT], O.h2f(out_ref)[:, :OUT]), 99) < 3e-2
    assert np.percentile(K.rae(O.h2f(hid), O.h2f(hid_ref)), 99) < 3e-2
    _, out_inf = emu.mlp_forward(om, ph, xs, save_hidden=False)
    assert np.array_equal(out_inf, out)
    dy = O.f2h((rng.standard_normal((n, om.padded_out)) * 0.01).astype(np.float32))
    dy[:, OUT:] = 0
    gref, dref = O.mlp_backward(om, ph, x, hid_ref, out_ref, dy)
    gh, dx = emu.mlp_backward(om, ph, xs, hid_ref, dy)
    assert rel_l2(O.h2f(gh), gref) < 2e-2
    if H <= 2:
        assert np.percentile(K.rae(O.h2f(gh), gref), 99) < 3e-2
    assert rel_l2(O.h2f(dx).T, O.h2f(dref)) < 2e-2
    gacc, _ = emu.mlp_backward(om, ph, xs, hid_ref, dy, grads_init=gh)
    assert rel_l2(O.h2f(gacc), 2 * gref) < 2e-2
    g_none, dx2 = emu.mlp_backward(om, ph, xs, hid_ref, dy, want_grads=False)
    assert g_none is None and np.array_equal(dx2, dx)


@pytest.mark.parametrize("act,out_act", K.ACTIVATION_CASES)
def test_mlp_activations(act, out_act):
    """test_mlp_activations in bfloat16: oracle bars of tests/bf16_cases.py; fused == unfused bit for bit."""
    IN, W, OUT, H = 32, 64, 4, 2
    rng = np.random.default_rng(11)
    om = O.mlp_init(IN, W, OUT, H, activation=act, output_activation=out_act)
    ph = O.f2h(O.mlp_init_params(om, O.pcg32(5)) * 0.5)
    n = 256
    x = O.f2h(rng.random((n, IN), dtype=np.float32) * 0.5)
    xs = np.ascontiguousarray(x.T)
    hid_ref, out_ref = O.mlp_forward(om, ph, x)
    hid, out = emu.mlp_forward(om, ph, xs)
    assert np.percentile(K.rae(O.h2f(out)[:, :OUT], O.h2f(out_ref)[:, :OUT]), 99) < 3e-2
    assert np.percentile(K.rae(O.h2f(hid), O.h2f(hid_ref)), 99) < 3e-2
    dy = O.f2h((rng.standard_normal((n, om.padded_out)) * 0.01).astype(np.float32))
    dy[:, OUT:] = 0
    gref, dref = O.mlp_backward(om, ph, x, hid_ref, out_ref, dy)
    gh, dx = emu.mlp_backward(om, ph, xs, hid_ref, dy, output=out_ref)
    assert rel_l2(O.h2f(gh), gref) < 2e-2 and rel_l2(O.h2f(dx).T, O.h2f(dref)) < 2e-2
    target = rng.random((n, OUT), dtype=np.float32)
    out_f, dy_f, dx_f, g_f, _ = emu.mlp_train(om, ph, xs, O.LOSS_L2, target, OUT)
    _, dyl, _ = emu.loss(O.LOSS_L2, out, target, OUT)
    g_u, dx_u = emu.mlp_backward(om, ph, xs, hid, dyl, output=out)
    assert np.array_equal(out_f, out) and np.array_equal(dy_f, dyl) and np.array_equal(dx_f, dx_u) and same_weight_gradients(g_f, g_u)


@pytest.mark.parametrize("case", K.MLP_CASES + K.WAVE_CASES + K.WIDE_CASES)
@pytest.mark.parametrize("loss_type", [O.LOSS_L2, O.LOSS_RELATIVE_L2])
def test_mlp_fused_training_pass_equals_the_unfused_kernels(case, loss_type):
    """The "same BITS fused vs unfused" assertions of the fp16 module, unchanged; where that module allows the last fp16 bit of a
    few weight gradients (fp32 partial sums grouped differently) this one allows the last bfloat16 bit."""
    IN, W, OUT, H = case
    rng = np.random.default_rng(7)
    om = O.mlp_init(IN, W, OUT, H)
    ph = O.f2h(O.mlp_init_params(om, O.pcg32(99)))
    n = 256 if W == 128 else 512
    xs = np.ascontiguousarray(O.f2h(rng.random((n, IN), dtype=np.float32)).T)
    target = rng.random((n, OUT), dtype=np.float32)
    pdf = (0.5 + rng.random((n, OUT), dtype=np.float32)) if loss_type == O.LOSS_L2 else None
    fused = emu.mlp_train(om, ph, xs, loss_type, target, OUT, data_pdf=pdf, n_total=2 * n * OUT)
    if H > 4 or OUT > 16 or (W == 128 and IN not in (32, 64)):
        assert fused is None
        return
    out_f, dy_f, dx_f, g_f, loss_f = fused
    hid, out = emu.mlp_forward(om, ph, xs)
    _, dy, loss_u = emu.loss(loss_type, out, target, OUT, data_pdf=pdf, n_total=2 * n * OUT)
    g, dx = emu.mlp_backward(om, ph, xs, hid, dy)
    assert np.array_equal(out_f, out) and np.array_equal(dy_f, dy)
    assert np.array_equal(dx_f, dx) and same_weight_gradients(g_f, g)
    assert abs(loss_f - loss_u) <= 1e-5 * abs(loss_u) + 1e-12
    out2 = emu.mlp_train(om, ph, xs, loss_type, target, OUT, data_pdf=pdf, n_total=2 * n * OUT, want_dinput=False)
    assert out2[2] is None and np.array_equal(out2[3], g_f)
    ext = O.f2h((rng.standard_normal((n, om.padded_out)) * 0.02).astype(np.float32))
    out_e, _, dx_e, g_e, _ = emu.mlp_train(om, ph, xs, loss_type, None, OUT, external_dL_doutput=ext)
    g_u, dx_u = emu.mlp_backward(om, ph, xs, hid, ext)
    assert np.array_equal(out_e, out)
    # (as in the fp16 module, in units of the largest entry: there 2^-10 = one fp16 step at the largest entry's binade, here 2^-7)
    close = lambda a, b: np.mean(a != b) < 0.05 and np.abs(O.h2f(a) - O.h2f(b)).max() <= 2.0 ** -7 * np.abs(O.h2f(b)).max()  # noqa: E731
    assert close(g_e, g_u) and close(dx_e, dx_u)


@pytest.mark.parametrize("case", K.WAVE_CASES + [(32, 64, 4, 2), (32, 64, 5, 3), (32, 32, 7, 4), (64, 64, 16, 2), (64, 64, 1, 3)])
@pytest.mark.parametrize("act", [O.ACT_RELU, O.ACT_NONE])
def test_mlp_register_resident_inference_equals_forward(case, act):
    K.test_mlp_register_resident_inference_equals_forward(case, act)  # bit equality of two kernels: nothing depends on the type


@pytest.mark.parametrize("hidden_layers", [2, 1])
@pytest.mark.parametrize("loss_type", [O.LOSS_L2, O.LOSS_RELATIVE_L2])
@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (0.75, -0.125)])
def test_network_kernel_loads_an_unpadded_identity_encoding_itself(loss_type, scale, offset, hidden_layers):
    K.test_network_kernel_loads_an_unpadded_identity_encoding_itself(loss_type, scale, offset, hidden_layers)


@pytest.mark.parametrize("shape", [(64, 64, 16, 2), (64, 64, 16, 1), (64, 64, 16, 3), (32, 64, 16, 2), (32, 32, 16, 4)])
def test_inference_kernel_loads_an_unpadded_identity_encoding_itself(shape):
    K.test_inference_kernel_loads_an_unpadded_identity_encoding_itself(shape)


# ---------------------------------------------------------------------------------------------------------------------
# loss, Adam, casts, encodings
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", range(len(O.LOSS_NAMES)))
def test_loss_bit_exact(loss_type):
    K.test_loss_bit_exact(loss_type)  # gradients: the oracle's (bfloat16) bits


def test_adam_matches_oracle_and_keeps_the_half_copy_in_step():
    """test_adam_matches_oracle in bfloat16, plus the invariant of the 16-bit copy: params16 == f2h(master) for every parameter the
    step touched (entries with a zero gradient are skipped and keep both)."""
    rng = np.random.default_rng(4)
    h = O.adam_defaults(learning_rate=1e-2, beta2=0.99, epsilon=1e-15, l2_reg=1e-6)
    n, nm = 4096 + 3, 1024
    w = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 20).astype(np.float32)
    g[2000:3000] = 0
    gh = O.f2h(g)
    a = [w.copy(), O.f2h(w), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)]
    b = [x.copy() for x in a]
    for step in (1, 2, 3):
        O.adam_step(h, nm, 128.0, step, a[0], a[1], gh, a[2], a[3], a[4])
        emu.adam_step(h, nm, 128.0, step, b[0], b[1], gh, b[2], b[3], b[4])
        assert np.array_equal(b[1], O.f2h(b[0]))
    assert np.array_equal(a[4], b[4]) and np.all(a[4][2000:3000] == 0)
    assert np.allclose(a[0], b[0], rtol=1e-6, atol=1e-9) and np.allclose(a[2], b[2], rtol=1e-6) and np.allclose(a[3], b[3], rtol=1e-6)
    assert np.mean(a[1] != b[1]) < 1e-3


def test_casts_and_identity_over_the_bf16_range():
    """cast_f32_to_f16 and identity_forward in bfloat16, including inputs above 65504 and below 2^-24 -- legal here, not in fp16 --
    and the rounding edges: ties (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6), subnormals, the largest finite value, infinity."""
    x = np.random.default_rng(5).standard_normal(1003).astype(np.float32)
    x[:12] = [1.00390625, 1.01171875, 65504.0, 1.0e5, 3.0e38, 3.3961775e38, 2.0 ** -24, 2.0 ** -30, 1.0e-38, 2.0 ** -133, 2.0 ** -134, -2.0 ** -140]
    x[12:15] = [np.inf, -np.inf, 0.0]
    got = emu.cast_f32_to_f16(x)
    assert np.array_equal(got, O.f2h(x))
    assert got[0] == 0x3F80 and got[1] == 0x3F82 and got[2] == 0x4780 and got[6] == 0x3380 and got[9] == 0x0001 and got[10] == 0x0000 and got[12] == 0x7F80
    for i in range(15):  # the oracle's conversion itself against rational arithmetic
        if np.isfinite(x[i]):
            assert got[i] & 0x7FFF == rne_bf16_exact(Fraction(float(x[i]))) & 0x7FFF, i
    for n, n_dims, padded in ((768, 64, 64), (600, 12, 16), (256, 5, 16), (256, 3, 16)):
        xi = (np.random.default_rng(n).standard_normal((n, n_dims)) * 10.0 ** np.random.default_rng(n + 1).integers(-30, 30, (n, n_dims))).astype(np.float32)
        xi[0, :3] = [1.0e5, 2.0 ** -30, -7.0e4]
        want = O.identity_forward(xi, padded)
        assert np.array_equal(emu.identity_forward(xi, padded).T, want), (n, n_dims)
        assert np.all(np.isfinite(O.h2f(want))) and O.h2f(want)[0, 0] == 99840.0


@pytest.mark.parametrize("d,n_frequencies,padded", [(3, 12, 80), (2, 4, 16), (5, 10, 112)])
def test_frequency_encoding(d, n_frequencies, padded):
    K.test_frequency_encoding(d, n_frequencies, padded)


@pytest.mark.parametrize("d,n_bins,padded", [(2, 64, 128), (3, 16, 48), (1, 4, 16)])
def test_oneblob_encoding(d, n_bins, padded):
    K.test_oneblob_encoding(d, n_bins, padded)

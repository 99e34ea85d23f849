"""The CPU-side conditions tests/test_gpu_call_history.py relies on (tests/call_history_cases.py), from the case files' own arithmetic:
the overflow history provably fills a queue, the other-plan history lays its counters out differently from the probe's plan, every dyadic
network probe passes its case file's exactness audit, and the fp32 grid probes' sums are order-independent."""
import numpy as np

import call_history_cases as H
import scatter_owner_cases as K


def test_the_overflow_history_fills_a_queue():
    og, pos, dy, _, spilled = H.overflow_case()  # (asserts K.must_overflow and K.spilled_pairs > 0)
    print(f"overflow history: {spilled} pairs past their queue's capacity")
    assert pos.shape == (H.BIG, 3) and spilled > 0
    # and the probe's own calls stay inside their queues: what touches the overflow counter is the history alone
    og, pos, _, _ = H.grid_half_data(H.GRID_N)
    assert not K.must_overflow(og, "uniform", H.GRID_N) and K.spilled_pairs(og, pos[:H.GRID_N]) == 0


def test_the_other_plan_lays_its_counters_out_differently():
    probe, _ = H.grid_half_data(H.GRID_N)[:2]
    other, _ = H.grid_half_data(H.OTHER_PLAN["n"], H.OTHER_PLAN["D"], H.OTHER_PLAN["table"])[:2]
    (qa, overflow_a), (qb, overflow_b) = H.queue_layout(probe, H.GRID_PADDED), H.queue_layout(other, H.OTHER_PLAN["padded"])
    print(f"probe plan: queues {qa}, overflow counter {overflow_a}; other plan: queues {qb}, overflow counter {overflow_b}")
    assert len(qa) == 8 and len(qb) == 3 and overflow_a != overflow_b
    assert overflow_b < overflow_a  # the other plan's overflow counter is one of the probe plan's queue counters
    assert max(H.n_counters(probe), H.n_counters(other)) < H.COUNTER_BUFFER_FLOOR  # these two share one buffer and never regrow it


def test_the_grow_plan_needs_more_counters_than_the_smallest_buffer():
    """history 3's third plan makes ZeroedCounters::get free and reallocate the buffer the probe's plan allocated: from the plan arithmetic"""
    og = H.grow_plan_grid()
    queues, overflow = H.queue_layout(og, H.GROW_PLAN["n"])
    print(f"grow plan: queues {queues}, overflow counter {overflow}, {H.n_counters(og)} counters, {og.n_params * 2 / 2 ** 20:.0f} MiB of parameters")
    assert H.n_counters(og) > H.COUNTER_BUFFER_FLOOR
    assert max(queues) <= 4096 and max(og.offsets[l + 1] - og.offsets[l] for l in range(og.n_levels)) <= 1 << 25  # MAX_BUCKETS_PER_LEVEL, PAIR_INDEX_BITS
    n, pairs = H.GROW_PLAN["n"], (1 << H.GROW_PLAN["D"])
    assert all(n * pairs // q <= 65536 for q in queues)  # one sample chunk per queue: a sole owner per slice, exact sums
    assert H.GROW_PLAN["n"] <= H.BIG


def test_every_batch_is_at_most_4096():
    assert max(H.LADDER + [H.BIG, H.OVERFLOW["n"], H.GRID_PADDED, H.NE_N, H.TRAINER_N, H.W_CASE.n, H.L16_CASE.n, H.L32_CASE.n]) <= 4096


def test_dyadic_network_probes_pass_their_audits():
    for name, (text, passes) in H.network_probe_audits().items():
        print(name, text)
        assert passes, (name, text)


def test_fp32_grid_probe_sums_are_order_independent():
    og, pos, dy, ddx, params = H.grid_exact_data(H.GRID_N)
    unit, figure, w = H.exact_grid_sums(og, pos, dy)
    print(f"first order: unit 2^{unit}, largest sum|terms| / unit {figure:.0f}")
    assert unit >= -7 and figure < 2.0 ** 24
    assert np.any((w > 0) & (w < 1)) and np.any(w == 1)
    ref = H.second_order_reference(og, pos, dy, ddx, params)
    figure = H.exact_second_order_sums(og, ref)
    print(f"second order: unit 2^-6, largest sum|terms| / unit {figure:.0f}")
    assert figure < 2.0 ** 24
    assert np.abs(ref.dL_dparams).max() > 0 and np.abs(ref.dL_dinput).max() > 0 and np.abs(ref.dL_ddLdoutput).max() > 0

"""The record scatter drops pair records whose payloads are all +-0 (csrc/grid_backward_scatter.hip): the bucketed grid backward on the GPU with
dL/dy patterns that make such records -- whole samples of zeros, one feature zero, +0 / -0, subnormal values that underflow only in the product
with the corner weight -- against the oracle, with the comparison and the bars of tests/test_gpu_parity.py::test_bucketed_grid_backward_full_size
(restated at the asserts; the owners' sums are exact, so none is loosened).  N = 1000 reaches the kernels the way a ragged batch does in use:
padded to the batch granularity (1024) with rows whose dL/dy is zero; the oracle sees the 1000 rows.  1024 rows are two whole 512-sample
tiles of the scatter, so N = 1280 (a multiple of the granularity, two and a half tiles) is there for the partly filled last tile.
The patterns enter through the encoding's own backward (Module::bwd over the C ABI, as in test_bucketed_grid_backward_full_size): the
trainer's backward computes dL/dy itself and takes none from outside; the trainer is covered by the 30-step run at the end.
(Patterns: tests/test_emu_zero_records.py.)"""
import numpy as np
import pytest
import torch

from conftest import HASH_ENCODING_SMALL, config_hash
from oracle import oracle as O
from test_emu_zero_records import PATTERNS, make_dy
from test_gpu_parity import h_t, oracle_grid, positions, targets_for, tcnn

pytestmark = pytest.mark.gpu

ENC = dict(HASH_ENCODING_SMALL)  # 16 levels, F = 2, T = 2^15, 3-D: dense coarse levels and hashed ones


def backward_both(C, m, og, pos, dy_bits, n_real):
    """-> {mode: gradient as float64} for the fp32-slice formulation (0) and the bucketed one (3); rows >= n_real are padding (dL/dy zero)"""
    n = pos.shape[0]
    assert n % 256 == 0 and not dy_bits[n_real:].any()
    x = torch.from_numpy(pos).cuda()
    p = torch.zeros(og.n_params, dtype=torch.half, device="cuda").requires_grad_(True)
    ctx, y = m.fwd(x, p)
    out = {}
    default_mode = C.get_grid_backward_mode()
    try:
        for mode in (0, 3):
            C.set_grid_backward_mode(mode)
            _, dp = m.bwd(ctx, x, p, y, h_t(dy_bits))
            torch.cuda.synchronize()
            out[mode] = dp.float().cpu().numpy().astype(np.float64)
    finally:
        C.set_grid_backward_mode(default_mode)
    return out


def check(out, og, pos, dy_bits, exact):
    ref = O.grid_backward(og, pos, dy_bits)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy_bits))))
    err3, err03 = np.abs(out[3] - ref) - absacc * 2.0 ** -8, np.abs(out[3] - out[0]) - absacc * 2.0 ** -8
    print(f"max(|bucketed - oracle| - 2^-8 sum|.|) = {err3.max():.3e}, max(|bucketed - sliced| - 2^-8 sum|.|) = {err03.max():.3e} (bar 1e-3)")
    # test_bucketed_grid_backward_full_size: 2^-8 of the magnitude + 1e-3, against the oracle and against the fp32-slice formulation
    assert np.all(err3 <= 1e-3)
    assert np.all(err03 <= 1e-3)
    assert not out[3][absacc == 0].any()  # entries that only zeros reach (or nothing) are stored as zero
    if exact:
        # every slice has one owner here (<= 65536 records per slice) and the overflow list is scanned by the owners: the exact sum rounded
        # once, as test_bucketed_grid_backward_full_size asserts for its sole-owner levels (same fraction: the oracle's float64 sum is
        # itself rounded where the magnitudes differ widely)
        same = np.mean(out[3].astype(np.float32) == O.h2f(O.f2h(ref.astype(np.float32))))
        print(f"entries equal to the oracle's sum rounded once: {same:.6f} (bar 0.998)")
        assert same > 0.998


@pytest.fixture(scope="module")
def encoding():
    C = tcnn()._C
    return C, C.create_encoding(3, ENC), oracle_grid(ENC, 3)


@pytest.mark.parametrize("n", [1000, 1280, 4096])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_zero_record_patterns_against_the_oracle(encoding, pattern, n):
    C, m, og = encoding
    padded = (n + 255) // 256 * 256
    pos = np.zeros((padded, 3), np.float32)
    pos[:n] = positions(n, 3, seed=21)
    dy = np.zeros((padded, m.n_output_dims()), np.uint16)
    dy[:n] = make_dy(pattern, n, m.n_output_dims(), 2, seed=7)
    out = backward_both(C, m, og, pos, dy, n)
    check(out, og, pos[:n], dy[:n], exact=True)
    if pattern in ("all_zero", "signed_zeros"):
        assert not out[3].any()
    elif pattern != "subnormal":  # (sums of a few subnormal products may all round to zero)
        assert out[3].any()


def test_clustered_input_through_the_overflow_list():
    """Every sample inside one cell of the fine levels of a T = 2^17 table (16 slices): a hashed level's pairs land in two slices' queues and pass
    their capacity (asserted below from the oracle's indices and the planner's capacity rule); what does not fit travels through the overflow
    list.  One sample in eight has dL/dy zero (its pairs are never queued) and one in eight subnormal values, whose pairs hold zero records
    next to non-zero ones: among the spilled pairs are records that stay out of the list."""
    C = tcnn()._C
    enc = dict(ENC, log2_hashmap_size=17)
    m, og = C.create_encoding(3, enc), oracle_grid(enc, 3)
    n = 4096
    pos = (0.37 + positions(n, 3, seed=5) * 1e-5).astype(np.float32)
    K = m.n_output_dims()
    dy = make_dy("ordinary", n, K, 2, seed=9)
    dy[0::8] = 0
    dy[1::8] = make_dy("subnormal", n, K, 2, seed=10)[1::8]
    # make_backward_plan: slices of 2^13 entries, n * 8 / 16 records per slice (one chunk), capacity = 2 * (n * 4 / 16) + 512 pairs
    idx = O.grid_indices(og, pos)
    capacity = 2 * (n * 4 // 16) + 512
    ordinary = np.arange(n) % 8 >= 2
    spilled = 0
    for l in range(og.n_levels):
        if og.offsets[l + 1] - og.offsets[l] == 1 << 17:
            per_bucket = np.bincount((idx[ordinary, l, 0::2] >> 13).reshape(-1), minlength=16)  # first entry of each pair, rows whose records are not zero
            spilled += int(np.maximum(per_bucket - capacity, 0).sum())
    assert spilled > 1000, "the input does not overflow a queue: the case tests nothing"
    assert spilled * 2 < 1 << 18  # OVERFLOW_INLINE_MAX: the owners scan the list themselves (exact sums)
    out = backward_both(C, m, og, pos, dy, n)
    check(out, og, pos, dy, exact=False)  # (thousands of records per entry: the oracle's float64 sum is not the exact sum any more)
    assert out[3].any()


def test_thirty_training_steps_equal_the_fp32_slice_formulation():
    """A tiny model (T = 2^12, 64x2), 30 steps from the same parameters with the bucketed backward and with TCNN_GRID_BACKWARD=sliced_f32's
    formulation.  The suite asserts no bit-for-bit equality between the two for training (the fp32 slices round a running sum, the owners
    round the exact sum once), so the run is held to the bars tests/test_gpu_parity.py::test_training_step_matches_oracle holds the trainer to
    against the oracle: losses within 2e-2 relative, and fewer than 2e-3 of the parameters further than 1e-2 (one Adam step) apart."""
    T = tcnn()
    C = T._C
    cfg = config_hash(log2_hashmap_size=12, per_level_scale=1.5)
    n = 4096
    pos = positions(n, 3, seed=21)
    tgt = targets_for(pos, 4)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    default_mode = C.get_grid_backward_mode()
    runs = {}
    try:
        for mode in (3, 0):
            C.set_grid_backward_mode(mode)
            tm = T.create_from_config(3, 4, cfg, seed=1337)
            w = tm.params_full_precision.clone()
            w[tm.n_mlp_params:] *= 1.0e3
            tm.set_params_full_precision(w)
            losses = []
            for _ in range(30):
                ctx = tm.training_step(x, t)
                losses.append(tm.loss(ctx))
            runs[mode] = (np.array(losses), tm.params_full_precision.cpu().numpy().copy())
    finally:
        C.set_grid_backward_mode(default_mode)
    (l3, w3), (l0, w0) = runs[3], runs[0]
    far = np.mean(np.abs(w3 - w0) > 1e-2)
    print(f"max relative loss difference {np.max(np.abs(l3 - l0) / np.abs(l0)):.3e} (bar 2e-2), parameters further than 1e-2 apart: {far:.3e} (bar 2e-3), "
          f"bit-identical parameters: {np.mean(w3 == w0):.4f}")
    assert np.allclose(l3, l0, rtol=2e-2)
    assert far < 2e-3
    assert l3[-1] < l3[0]

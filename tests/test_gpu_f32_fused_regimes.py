"""The fused fp32 network kernels (csrc/mlp_f32_fused*.hip) on a real MI355X in the regimes the tests that came with them leave out, with
the data, the bars (FACTOR x the error of a numpy float32 restatement against float64 on the same inputs) and the helpers of
tests/test_gpu_f32_fused_network.py, test_gpu_f32_fused_backward.py and test_gpu_f32_fused_second_order.py, unchanged; every helper
restores the switch it sets.

  * Shapes: inputs 64, 80 and 112, padded outputs 48 and 64 from 40 and 33 outputs, one to three hidden layers, at every width and n = 768.
  * Staged weights through the persistent loop: 128 -> 64 x 6 -> 16 fits LDS neither in the forward pass nor in the backward chain with
    dL/dinput (tests/test_emu_f32_fused.py asserts the sizes); at n = 131328 there are 513 sample tiles for 512 workgroups, so workgroup 0
    stages every matrix a second time.  Per-sample results of the first, a middle and that last tile are, bit for bit, those of the same
    256 rows as a batch of their own; the parameter gradients are held to the bar.  At this batch size some ReLU pre-activation always
    lies within 2e-6 of zero whatever the seed (measured: a GPU dL/dinput 5e-3 off on such a sample, where fp32 rounding decides the
    branch), so the data is drawn away from the kinks row by row: the few such samples are replaced by copies of others.
  * Residency: without dL/dinput the same chain keeps its matrices resident; each result alone and both together are the same bits."""
import numpy as np
import pytest
import torch

import second_order_mlp_reference as R
from test_gpu_f32_fused_backward import grads
from test_gpu_f32_fused_network import FACTOR, bits, case, held, mlp, run
from test_gpu_f32_fused_second_order import NAMES, fp32, hold, second_order

pytestmark = pytest.mark.gpu

SHAPES = [(80, 2, 40), (112, 3, 33), (64, 1, 40)]  # (inputs, hidden layers, outputs)
STAGED = dict(IN=128, W=64, H=6, OUT=13)
BIG = 131328
TILES = (0, 65536, 131072)  # first rows of tile 0, of tile 256 and of tile 512: workgroup 0's second


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-x%d-%d" % s)
@pytest.mark.parametrize("W", [16, 32, 64])
def test_shapes_first_order(W, shape):
    IN, H, OUT = shape
    run(fp32(IN, OUT, W, H), case(IN, W, H, OUT, 768, away_from_kinks=True), 768, backward=True)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-x%d-%d" % s)
@pytest.mark.parametrize("W", [16, 32, 64])
def test_shapes_second_order(W, shape):
    IN, H, OUT = shape
    hold(IN, W, H, OUT, 768)  # (Softplus; fused and layer by layer)


def staged(hidden_act):
    s = STAGED
    return fp32(s["IN"], s["OUT"], s["W"], s["H"], hidden_act), (s["IN"], s["W"], s["H"], s["OUT"])


def test_staged_weights_through_the_persistent_loop():
    m, shape = staged("ReLU")
    mats, x, dy = case(*shape, BIG)[:3]
    # away from the kinks, row by row: a sample with a float64 pre-activation within 2e-6 of zero (the rule of tests/test_gpu_f32_network.py)
    # is replaced by one without; the weights of the seed stay
    near = np.zeros(BIG, bool)
    for pre in mlp(np.float64, mats, x, dy, "ReLU", "None")[3]:
        near |= np.abs(pre).min(axis=1) <= 2e-6
    assert near.sum() < 1000
    x = x.copy()
    x[near] = x[np.flatnonzero(~near)[:near.sum()]]
    data = case(*shape, BIG, given_x=x, away_from_kinks=True)
    assert all(np.array_equal(a, b) for a, b in zip(mats, data[0]))
    mats, x, dy = data[:3]
    y, dx, _ = run(m, data, BIG, backward=True)[True][:3]  # prediction, dL/dinput and parameter gradients under the bar, fused and layer by layer
    flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda()
    for lo in TILES:
        rows = slice(lo, lo + 256)
        xt = torch.from_numpy(x[rows]).cuda().requires_grad_(True)
        ctx, y_alone = m.fwd(xt, flat)
        dx_alone, none = m.bwd(ctx, xt, flat, y_alone, torch.from_numpy(dy[rows]).cuda())
        assert none is None
        assert np.array_equal(bits(y[rows]), bits(y_alone)), f"prediction of rows {lo} .."
        assert np.array_equal(bits(dx[rows]), bits(dx_alone)), f"dL/dinput of rows {lo} .."


def test_staged_weights_through_the_persistent_loop_second_order():
    m, shape = staged("Tanh")
    mats, x, dy = case(*shape, BIG, "Tanh")[:3]
    v = np.random.default_rng(99).uniform(-1, 1, size=x.shape).astype(np.float32)
    ref, cpu_error = R.errors(mats, x, dy, v, "Tanh", "None")
    full = second_order(m, mats, x, dy, v, True)
    held("fused " + NAMES[2], full[2], ref[2], FACTOR * cpu_error[2])
    held("layer by layer " + NAMES[2], second_order(m, mats, x, dy, v, False, want=(False, False, True))[2], ref[2], FACTOR * cpu_error[2])
    for lo in TILES:
        rows = slice(lo, lo + 256)
        alone = second_order(m, mats, x[rows], dy[rows], v[rows], True, want=(True, True, False))
        for k in (0, 1):
            assert np.array_equal(bits(full[k][rows]), bits(alone[k])), f"{NAMES[k]} of rows {lo} .."


def test_one_result_alone_is_the_same_bits_across_the_residency_change():
    n = 768
    m, shape = staged("ReLU")
    mats, x, dy = case(*shape, n, away_from_kinks=True)[:3]
    dx, dp = grads(m, mats, x, dy, True)
    dx_alone, none = grads(m, mats, x, dy, True, want_dp=False)
    assert none is None and np.array_equal(bits(dx_alone), bits(dx))
    none, dp_alone = grads(m, mats, x, dy, True, want_dx=False)  # (the chain with its matrices resident)
    assert none is None and np.array_equal(bits(dp_alone), bits(dp))
    m, _ = staged("Tanh")
    mats, x, dy = case(*shape, n, "Tanh")[:3]
    v = np.random.default_rng(99).uniform(-1, 1, size=x.shape).astype(np.float32)
    full = second_order(m, mats, x, dy, v, True)
    for k in range(3):
        alone = second_order(m, mats, x, dy, v, True, want=tuple(i == k for i in range(3)))
        assert [r is not None for r in alone] == [i == k for i in range(3)]
        assert np.array_equal(bits(alone[k]), bits(full[k])), NAMES[k]

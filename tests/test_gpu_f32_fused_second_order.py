"""The fused fp32 second-order pass (csrc/mlp_f32_fused_second_order.hip: the tangent chain, the dual reverse chain and the dual
weight-gradient kernel) on a real MI355X against the numpy float64 restatement of tests/second_order_mlp_reference.py, with the data of
tests/test_gpu_f32_fused_network.py and the bar of tests/test_gpu_f32_network.py unchanged: per result, FACTOR x the max error of the numpy
float32 restatement on the same inputs.  v ~ U(-1, 1) from a fixed seed.  Every case runs with tcnn_set_fp32_fused_second_order on and off
(the layer-by-layer launches, held to the same bar) and prints GPU error, CPU float32 error and bar (-s); every test restores the switch.

The exact cases follow test_gpu_f32_fused_backward.py: x and dL/doutput in {-1, 0, 1}, v in {-1, -1/2, 0, 1/2, 1}, input and output matrix
small integers over 4, hidden matrices {-1, 0, 1} over 2, ReLU -- every sum is an fp32 number in any order, so both paths and float64 must
agree in every bit."""
import numpy as np
import pytest
import torch

import second_order_mlp_reference as R
from test_gpu_f32_fused_network import C, HIDDEN, SHAPES, bits, case, held, network
from test_gpu_f32_network import FACTOR

pytestmark = pytest.mark.gpu
NAMES = ("dL/d(dL/doutput)", "dL/dinput", "parameter gradients")


def fp32(IN, OUT, W, H, hidden_act="ReLU", output_act="None"):
    return C().create_network_precision(IN, OUT, network(W, H, hidden_act, output_act), C().Precision.Fp32)


def second_order(m, mats, x, dy, v, fused, want=(True, True, True)):
    """fwd + bwd_bwd_input with the switch at `fused` -> (dL/d(dL/doutput), dL/dinput, parameter gradients), None where not wanted"""
    n = x.shape[0]
    C().set_fp32_fused_second_order(fused)
    try:
        assert m.fp32_fused_network(n) == 1 and m.fp32_fused_second_order(n) == int(fused)
        xt, pt = torch.from_numpy(x).cuda(), torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda()
        ctx, _ = m.fwd(xt.clone().requires_grad_(True), pt.clone().requires_grad_(True))
        ddy, dp, dx = m.bwd_bwd_input(ctx, xt.requires_grad_(want[1]), pt.requires_grad_(want[2]), torch.from_numpy(v).cuda(),
                                      torch.from_numpy(dy).cuda().requires_grad_(want[0]))
        return ddy, dx, dp
    finally:
        C().set_fp32_fused_second_order(True)


def hold(IN, W, H, OUT, n, hidden_act="Softplus", output_act="None"):
    mats, x, dy = case(IN, W, H, OUT, n, hidden_act, output_act, away_from_kinks=True)[:3]
    v = np.random.default_rng(99).uniform(-1, 1, size=x.shape).astype(np.float32)
    ref, cpu_error = R.errors(mats, x, dy, v, hidden_act, output_act)
    m = fp32(IN, OUT, W, H, hidden_act, output_act)
    for fused in (True, False):
        for name, got, r, e in zip(NAMES, second_order(m, mats, x, dy, v, fused), ref, cpu_error):
            held(("fused " if fused else "layer by layer ") + name, got, r, FACTOR * e)


@pytest.mark.parametrize("n", [256, 768])  # 768: three tiles over two slabs, the uneven slice
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-x%d-%d" % s)
@pytest.mark.parametrize("W", [16, 32, 64])
def test_widths_depths_and_batches(W, shape, n):
    IN, H, OUT = shape
    hold(IN, W, H, OUT, n)


@pytest.mark.parametrize("output_act", ["None", "Sigmoid"])
@pytest.mark.parametrize("hidden_act", HIDDEN)
def test_activations(hidden_act, output_act):
    """(SiLU / Sine: the derivatives are taken at the pre-activation block; None / ReLU / LeakyReLU with None: no curvature chain)"""
    hold(32, 32, 2, 4, 256, hidden_act, output_act)


def test_a_network_too_deep_for_resident_weights():
    hold(32, 64, 12, 4, 256, "Tanh")


@pytest.mark.parametrize("shape", [(48, 32, 3, 20), (128, 64, 2, 50)], ids=lambda s: "%d-%dx%d-%d" % s)
def test_one_result_alone_is_the_same_bits(shape):
    IN, W, H, OUT = shape
    m, (mats, x, dy) = fp32(IN, OUT, W, H, "Softplus"), case(IN, W, H, OUT, 768, "Softplus", away_from_kinks=True)[:3]
    v = np.random.default_rng(99).uniform(-1, 1, size=x.shape).astype(np.float32)
    full = second_order(m, mats, x, dy, v, True)
    for k in range(3):
        alone = second_order(m, mats, x, dy, v, True, want=tuple(i == k for i in range(3)))
        assert [r is not None for r in alone] == [i == k for i in range(3)]
        assert np.array_equal(bits(alone[k]), bits(full[k])), NAMES[k]


# (inputs, neurons, hidden layers, padded outputs, n); the last: 513 tiles, more than the chain kernels' 512 persistent workgroups
@pytest.mark.parametrize("shape", [(32, 64, 2, 16, 256), (48, 32, 3, 32, 768), (128, 64, 2, 64, 768), (16, 16, 2, 16, 131328)], ids=lambda s: "%d-%dx%d-%d-n%d" % s)
def test_exact_cases_agree_in_every_bit(shape):
    IN, W, H, OUTP, n = shape
    rng = np.random.default_rng(64)
    mats = [rng.integers(-2, 3, size=(W, IN)) / 4.0] + [rng.integers(-1, 2, size=(W, W)) / 2.0 for _ in range(H - 1)] + [rng.integers(-2, 3, size=(OUTP, W)) / 4.0]
    x, dy = rng.integers(-1, 2, size=(n, IN)).astype(np.float32), rng.integers(-1, 2, size=(n, OUTP)).astype(np.float32)
    v = (rng.integers(-2, 3, size=(n, IN)) / 2.0).astype(np.float32)
    mats = [a.astype(np.float32) for a in mats]
    ref = R.second_order(np.float64, mats, x, dy, v, "ReLU", "None")[:3]
    assert all(np.array_equal(r.astype(np.float32).astype(np.float64), r) for r in ref)  # (every result is an fp32 number)
    m = fp32(IN, OUTP, W, H)
    fused, plain = second_order(m, mats, x, dy, v, True), second_order(m, mats, x, dy, v, False)
    for k in (0, 2):
        assert np.array_equal(fused[k].cpu().numpy().astype(np.float64), ref[k]), NAMES[k]
        assert np.array_equal(bits(fused[k]), bits(plain[k])), NAMES[k]
    assert not fused[1].any() and not plain[1].any() and not ref[1].any()

"""The fused fp32 backward pass (csrc/mlp_f32_fused_backward.hip: the chain kernel and the one-launch weight-gradient kernel) on a real
MI355X against the numpy float64 MLP, with the data, the bars (FACTOR x the error of a numpy float32 restatement) and the helpers of
tests/test_gpu_f32_fused_network.py, unchanged.  The forward switch stays on; the backward switch is restored by every test.

The exact cases follow test_exact_case_agrees_in_every_bit there: x and dL/doutput in {-1, 0, 1}, input and output matrix small integers
over 4, hidden matrices {-1, 0, 1} over 2, ReLU -- every product and partial sum is an fp32 number in any order, so the fused kernels, the
layer-by-layer kernels and float64 must agree in every bit."""
import numpy as np
import pytest
import torch

from test_gpu_f32_fused_network import C, HIDDEN, SHAPES, bits, case, held, mlp, network

pytestmark = pytest.mark.gpu


def fp32(IN, OUT, W, H, hidden_act="ReLU", output_act="None"):
    return C().create_network_precision(IN, OUT, network(W, H, hidden_act, output_act), C().Precision.Fp32)


def grads(m, mats, x, dy, fused, want_dx=True, want_dp=True):
    """forward + backward with the backward switch at `fused` -> (dL/dinput, parameter gradients), None where not asked for"""
    n = x.shape[0]
    C().set_fp32_fused_backward(fused)
    try:
        assert m.fp32_fused_network(n) == 1 and m.fp32_fused_backward(n) == int(fused)
        xt = torch.from_numpy(x).cuda().requires_grad_(want_dx)
        pt = torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda().requires_grad_(want_dp)
        ctx, y = m.fwd(xt, pt)
        return m.bwd(ctx, xt, pt, y, torch.from_numpy(dy).cuda())
    finally:
        C().set_fp32_fused_backward(True)


def hold_both(m, data, fused):
    mats, x, dy, ref, bars = data
    dx, dp = grads(m, mats, x, dy, fused)
    tag = "fused" if fused else "layer by layer"
    held(f"{tag} dL/dinput", dx, ref[1], bars[1])
    held(f"{tag} parameter gradients", dp, ref[2], bars[2])


@pytest.mark.parametrize("n", [256, 768])  # 768: three tiles over two slabs, the uneven slice
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-x%d-%d" % s)
@pytest.mark.parametrize("W", [16, 32, 64])
def test_widths_depths_and_batches(W, shape, n):
    IN, H, OUT = shape
    m, data = fp32(IN, OUT, W, H), case(IN, W, H, OUT, n, away_from_kinks=True)
    hold_both(m, data, True)
    hold_both(m, data, False)


@pytest.mark.parametrize("output_act", ["None", "Sigmoid"])
@pytest.mark.parametrize("hidden_act", HIDDEN)
def test_activations(hidden_act, output_act):
    """(SiLU / Sine: the derivative is taken at the pre-activation block behind the post-activations)"""
    hold_both(fp32(32, 4, 32, 2, hidden_act, output_act), case(32, 32, 2, 4, 256, hidden_act, output_act, away_from_kinks=True), True)


def test_a_network_too_deep_for_resident_weights():
    hold_both(fp32(32, 4, 64, 12), case(32, 64, 12, 4, 256, away_from_kinks=True), True)


@pytest.mark.parametrize("shape", [(48, 32, 3, 20), (128, 64, 2, 50)], ids=lambda s: "%d-%dx%d-%d" % s)
def test_one_result_alone_is_the_same_bits(shape):
    IN, W, H, OUT = shape
    m, (mats, x, dy) = fp32(IN, OUT, W, H), case(IN, W, H, OUT, 768, away_from_kinks=True)[:3]
    dx, dp = grads(m, mats, x, dy, True)
    dx_alone, none = grads(m, mats, x, dy, True, want_dp=False)
    assert none is None and np.array_equal(bits(dx_alone), bits(dx))
    none, dp_alone = grads(m, mats, x, dy, True, want_dx=False)
    assert none is None and np.array_equal(bits(dp_alone), bits(dp))


# (inputs, neurons, hidden layers, padded outputs, n); the last: 513 tiles, more than the chain kernel's 512 persistent workgroups
@pytest.mark.parametrize("shape", [(32, 64, 2, 16, 256), (48, 32, 3, 32, 768), (128, 64, 2, 64, 768), (16, 16, 2, 16, 131328)], ids=lambda s: "%d-%dx%d-%d-n%d" % s)
def test_exact_cases_agree_in_every_bit(shape):
    IN, W, H, OUTP, n = shape
    rng = np.random.default_rng(64)
    mats = [rng.integers(-2, 3, size=(W, IN)) / 4.0] + [rng.integers(-1, 2, size=(W, W)) / 2.0 for _ in range(H - 1)] + [rng.integers(-2, 3, size=(OUTP, W)) / 4.0]
    x, dy = rng.integers(-1, 2, size=(n, IN)).astype(np.float32), rng.integers(-1, 2, size=(n, OUTP)).astype(np.float32)
    mats = [a.astype(np.float32) for a in mats]
    ref = mlp(np.float64, mats, x, dy, "ReLU", "None")[1:3]
    assert all(np.array_equal(r.astype(np.float32).astype(np.float64), r) for r in ref)  # (every result is an fp32 number)
    m = fp32(IN, OUTP, W, H)
    fused, plain = grads(m, mats, x, dy, True), grads(m, mats, x, dy, False)
    for name, f, p, r in zip(("dL/dinput", "parameter gradients"), fused, plain, ref):
        assert np.array_equal(f.cpu().numpy().astype(np.float64), r), name
        assert np.array_equal(bits(f), bits(p)), name

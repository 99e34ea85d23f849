"""csrc/optimizer_kernels_f32.hip -- the optimizers' and the loss's kernels with float as the value type -- on the host SIMT emulator (no
GPU), against the numpy restatement of the reference's kernels with T = float (tests/optimizer_f32_reference.py): the cases and bars of
tests/test_gpu_optimizers_f32.py.

n_weights = 4099 (16-byte vector body of four floats per lane, a ragged scalar tail of 3, a last partial workgroup; the Average ring's
slots 1 and 2 start at 4 * 4099 and 8 * 4099 bytes, no multiples of 16: the scalar form of the whole kernel), layers [(64, 32), (16, 64)] =
3072 matrix weights + 1027 others, 7 steps.

SGD, Lookahead, Average, Batched, Ema(ExponentialDecay(SGD)): every buffer BIT-EQUAL after every step (single-rounding fp32 operations,
-ffp-contract=off).  Novograd: the bars of tests/test_emu_optimizers.py.  Adam: moments and per-parameter counters bit-equal to the
oracle's adam_step fed the same (fp16-representable) gradients, weights within ulps.  Loss (n = 256, stride = 16, dims = 3, all nine, with
and without data_pdf): values bit-equal to the 16-bit kernel's on the same fp16-representable predictions, the 16-bit kernel's gradient =
the fp32 kernel's gradient rounded to fp16 (RNE) wherever that gradient is a normal fp16 value; the excluded share is printed and below 1 %."""
import numpy as np
import pytest

import emu_optimizers_f32 as E
import optimizer_f32_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not E.available(), reason="no host compiler for the emulator")

N, LAYERS, STEPS, LOSS_SCALE = R.N, R.LAYERS, R.STEPS, R.LOSS_SCALE
BEGINS = np.array(R.BEGINS, np.uint32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("which", ["SGD", "Lookahead", "Average", "Batched", "EmaDecay"])
def test_sgd_and_wrappers_bit_equal(which):
    _, ref, state = R.chains()[which]
    _, got, _ = R.chains(E.Kernels(), E.aligned_zeros)[which]
    w = R.weights(5)
    gw = E.aligned_copy(w)
    rng = np.random.default_rng(6)
    for k in range(STEPS):
        g = R.gradients(rng, N)
        ref.step(LOSS_SCALE, w, g)
        got.step(LOSS_SCALE, gw, E.aligned_copy(g))
        assert ref.step_count() == got.step_count()
        assert np.array_equal(_bits(gw), _bits(w)), k
        for attr in state.values():
            assert np.array_equal(_bits(R.state_arrays(got, attr)), _bits(R.state_arrays(ref, attr))), (k, attr)
    if which == "Batched":
        assert ref.step_count() == STEPS and ref.nested.step_count() == 2
    if which == "Average":
        assert ref.nested.step_count() // 3 == 2  # the ring wrapped twice
        assert got.samples[1].ctypes.data % 16 != 0 and got.samples[2].ctypes.data % 16 != 0  # the scalar form ran
    if which == "EmaDecay":
        assert np.isclose(float(ref.nested.nested.learning_rate), 1.25e-3, rtol=1e-6)


def test_sgd_steps_a_range_only():
    """[begin, end) as the 16-bit kernels take it (begin a multiple of 4): parameters outside keep their bits; two ranges tile one step"""
    w = R.weights(7)
    g = E.aligned_copy(R.gradients(np.random.default_rng(8), N))
    whole = E.aligned_copy(w)
    E.sgd_step(LOSS_SCALE, 1e-2, 1e-6, whole, g)
    part = E.aligned_copy(w)
    E.sgd_step(LOSS_SCALE, 1e-2, 1e-6, part, g, 0, 2052)
    assert np.array_equal(_bits(part[2052:]), _bits(w[2052:]))
    E.sgd_step(LOSS_SCALE, 1e-2, 1e-6, part, g, 2052, N)
    assert np.array_equal(_bits(part), _bits(whole))


def test_novograd():
    NOVOGRAD = R.NOVOGRAD
    w = R.weights(9)
    w_init = w.copy()
    gw, gm1 = E.aligned_copy(w), E.aligned_zeros(N, np.float32)
    m1 = np.zeros(N, np.float32)
    moments = np.zeros(len(LAYERS), np.float32)
    rng = np.random.default_rng(10)
    beta2 = float(np.float32(NOVOGRAD["beta2"]))
    for k in range(STEPS):
        g = R.gradients(rng, N)
        ga = E.aligned_copy(g)
        again = E.novograd_step(BEGINS, NOVOGRAD, LOSS_SCALE, k == 0, E.aligned_copy(gw), ga, E.aligned_copy(gm1), moments)  # determinism
        new = E.novograd_step(BEGINS, NOVOGRAD, LOSS_SCALE, k == 0, gw, ga, gm1, moments)
        assert np.array_equal(_bits(new), _bits(again)), k
        for l in range(len(LAYERS)):
            b, e = int(BEGINS[l]), int(BEGINS[l + 1])
            b2 = 0.0 if k == 0 else beta2
            want = b2 * float(moments[l]) + (1.0 - b2) * R.novograd_norm64(g, b, e) / LOSS_SCALE / LOSS_SCALE
            assert abs(float(new[l]) - want) <= ((e - b) + 2) * 2.0 ** -24 * want, (k, l)
            R.novograd_step_layer(NOVOGRAD, LOSS_SCALE, k == 0, new[l], w, g, m1, b, e)
        moments = new
        assert np.array_equal(_bits(gm1), _bits(m1)), k
        assert np.array_equal(_bits(gw), _bits(w)), k
    nm = int(BEGINS[-1])
    assert np.array_equal(_bits(gw[nm:]), _bits(w_init[nm:])) and not np.array_equal(gw[:nm], w_init[:nm])


def _within_ulps(w, w_ref, w_before, ulps=4):
    """tests/test_gpu_parity_full.py's helper: |w - w_ref| <= `ulps` units in the last place of the larger of the old weight, the new
    weight and the largest Adam update (~3 lr): the update is a difference, so a result close to zero carries the absolute error of its operands."""
    scale = np.maximum(np.maximum(np.abs(w_before), np.abs(w_ref)), np.float32(0.03))
    return bool((np.abs(w - w_ref) <= ulps * np.spacing(scale)).all())


def test_adam_against_the_oracle():
    """test_optimizer_object_on_its_own_bit_level's case: n = 40000 (tail of 0; a last partial workgroup), 4096 matrix weights, 40 % zero
    gradients behind them, 4 steps.  Gradients are fp16-representable: floats for the fp32 kernel, 16-bit patterns for O.adam_step."""
    O.set_half_format(False)
    n, nm = 40003, 4096  # (40003: a ragged tail of 3 as well)
    adam = O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=1e-6, non_matrix_learning_rate_factor=0.5)
    rng = np.random.default_rng(5)
    w32 = rng.standard_normal(n).astype(np.float32)
    w16 = O.f2h(w32)
    m1, m2, steps = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    gw, gm1, gm2, gsteps = E.aligned_copy(w32), E.aligned_zeros(n, np.float32), E.aligned_zeros(n, np.float32), E.aligned_zeros(n, np.uint32)
    for k in range(4):
        g = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 60.0], n)).astype(np.float16)
        g[nm:][rng.random(n - nm) < 0.4] = 0
        E.adam_step(adam, nm, 128.0, k + 1, gw, E.aligned_copy(g.astype(np.float32)), gm1, gm2, gsteps)
        w_before = w32.copy()
        O.adam_step(adam, nm, 128.0, k + 1, w32, w16, g.view(np.uint16), m1, m2, steps)
        assert np.array_equal(gsteps, steps) and np.array_equal(_bits(gm1), _bits(m1)) and np.array_equal(_bits(gm2), _bits(m2)), k
        assert _within_ulps(gw, w32, w_before), k
        w32[:] = gw
        w16[:] = O.f2h(gw)
    assert len(np.unique(steps)) > 2


@pytest.mark.parametrize("with_pdf", [False, True], ids=["no_pdf", "data_pdf"])
@pytest.mark.parametrize("loss_type", range(len(R.LOSSES)), ids=R.LOSSES)
def test_loss_f32_against_the_16_bit_kernel(loss_type, with_pdf):
    O.set_half_format(False)
    prediction, target, pdf = R.loss_case()
    n, stride = prediction.shape
    dims = target.shape[1]
    pdf = pdf if with_pdf else None
    prediction_h = O.f2h(prediction)
    assert np.array_equal(O.h2f(prediction_h), prediction)  # representable
    values, grads = E.loss(loss_type, prediction, target, dims, LOSS_SCALE, pdf)
    values_h, grads_h = E.loss_half(loss_type, prediction_h, target, dims, LOSS_SCALE, pdf)
    assert not np.isnan(values).any() and not np.isnan(grads).any()  # every element written
    assert not values[:, dims:].any() and not grads[:, dims:].any()  # padding rows carry no loss
    assert np.array_equal(_bits(values), _bits(values_h))
    g = grads[:, :dims]
    normal = (np.abs(g) >= 2.0 ** -14) & (np.abs(g) < 65520.0)
    excluded = 1.0 - normal.mean()
    print(f"{R.LOSSES[loss_type]}: {100 * excluded:.3f} % of the fp32 gradients are no normal fp16 value")
    assert excluded < 0.01
    assert np.array_equal(grads_h[:, :dims][normal], O.f2h(g)[normal])
    assert values.sum() > 0 or R.LOSSES[loss_type] in ("CrossEntropy", "Variance")

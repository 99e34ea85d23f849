"""The stand-alone fp32 optimizer object (tcnn_create_optimizer_precision(..., TCNN_PRECISION_FP32) / native.Optimizer(..., precision=Fp32))
and the fp32 loss (tcnn_loss_evaluate_precision) over buffers the caller owns, against the numpy restatement of the reference's kernels
with T = float (tests/optimizer_f32_reference.py).

n_weights = 4099 (16-byte vector body of four floats per lane, a ragged scalar tail of 3, a last partial workgroup; the Average ring's
slots 1 and 2 are not 16-byte aligned: the scalar form of the whole kernel), layers [(64, 32), (16, 64)] = 3072 matrix weights + 1027
others, gradients with magnitudes mixed over 1e-3, 1, 60, 7 steps: Lookahead(n_steps = 3) pulls at nested counts 0, 3, 6;
Average(n_samples = 3) wraps its ring twice; Batched(batch_size_multiplier = 3) runs the nested step twice and ends on a partly filled pool.

Bars: SGD, Lookahead, Average, Batched, Ema(ExponentialDecay(SGD)): the weights and every state buffer BIT-EQUAL after every step
(single-rounding fp32 operations under -ffp-contract=off; fp32 division and square root are correctly rounded in this build).  Novograd:
the per-layer second moment against a float64 sum of the squared fp32 gradients within (n_layer + 2) 2^-24 relative (a sum of n non-negative
fp32 terms in any order errs by at most n - 1 roundings, plus one per square and one for the moment's update); first moments and weights
bit-equal to the restatement fed with the second moment READ BACK from the library; two runs give the same bits; the 1027 non-matrix
weights stay bit-unchanged.  Adam: tests/test_gpu_parity_full.py::test_optimizer_object_on_its_own_bit_level's case and bars, the
gradients fp16-representable floats.  Loss: values bit-equal to the 16-bit tcnn_loss_evaluate on the same (16-bit representable)
predictions; its gradient = the fp32 kernel's gradient rounded to 16 bits (RNE) on the elements whose fp32 gradient is a normal value of
the 16-bit type (the excluded share is printed and below 1 %: 0.000 % for every loss on the emulator, tests/test_emu_optimizers_f32.py)."""
import numpy as np
import pytest
import torch

import optimizer_f32_reference as R
from oracle import oracle as O
from test_gpu_parity import h_np, h_t

pytestmark = pytest.mark.gpu

N, LAYERS, BEGINS, STEPS = R.N, R.LAYERS, R.BEGINS, R.STEPS


def _native():
    from tinycudann import native
    return native


def _optimizer(cfg, n=N, **kw):
    from tinycudann._C import Precision
    return _native().Optimizer(cfg, n, precision=Precision.Fp32, **({"layer_sizes": LAYERS} if not kw else kw))


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.ravel().view(np.uint32)


def _same(t, ref):
    return np.array_equal(_bits(t), _bits(ref))


@pytest.mark.parametrize("which", ["SGD", "Lookahead", "Average", "Batched", "EmaDecay"])
def test_sgd_and_wrappers_bit_equal(which):
    from tinycudann._C import Precision
    cfg, ref, state = R.chains()[which]
    opt = _optimizer(cfg)
    assert opt.precision == Precision.Fp32
    w = R.weights(5)
    wd = torch.from_numpy(w.copy()).cuda()
    rng = np.random.default_rng(6)
    for k in range(STEPS):
        g = R.gradients(rng, N)
        opt.step(wd, None, torch.from_numpy(g).cuda())
        ref.step(128.0, w, g)
        torch.cuda.synchronize()
        assert opt.step_count == ref.step_count()
        assert _same(wd, w), k
        for name, attr in state.items():
            got = opt.state_named(name)
            assert got.dtype == torch.float32 and got.element_size() == 4
            assert _same(got, R.state_arrays(ref, attr)), (k, name)
    custom = opt.custom_weights()
    if which == "SGD":
        assert custom is None
    elif which == "Batched":
        assert custom is None and opt.step_count == STEPS and ref.nested.step_count() == 2
    else:
        name = {"Lookahead": "weights_lookahead", "Average": "weights_average", "EmaDecay": "weights_ema"}[which]
        assert custom.dtype == torch.float32 and custom.data_ptr() == opt.state_named(name).data_ptr()
    if which == "Average":
        assert ref.nested.step_count() // 3 == 2  # the ring wrapped twice
    if which == "EmaDecay":
        assert np.float32(opt.hyperparams()["nested"]["nested"]["learning_rate"]) == ref.nested.nested.learning_rate


def test_weights_must_be_null_or_the_master_pointer():
    import ctypes as C
    from tinycudann._C import _lib, _ptr, _stream
    opt = _optimizer(R.SGD_CFG)
    w, other, g = (torch.zeros(N, device="cuda") for _ in range(3))
    assert _lib.tcnn_optimizer_step(opt._h, _stream(), 1.0, _ptr(w), _ptr(w), _ptr(g)) == 0
    assert _lib.tcnn_optimizer_step(opt._h, _stream(), 1.0, _ptr(w), _ptr(other), _ptr(g)) != 0
    assert b"must be NULL or equal" in _lib.tcnn_last_error()
    assert opt.step_count == 1
    with pytest.raises(RuntimeError, match="float32"):
        opt.step(w, None, g.half())
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step(w, None, g.cpu())
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step(w, None, torch.zeros(2 * N, device="cuda")[::2])
    del C


def test_novograd():
    NOVOGRAD = R.NOVOGRAD
    cfg = {"otype": "Novograd", **NOVOGRAD}
    opt, twin = _optimizer(cfg), _optimizer(cfg)
    w = R.weights(9)
    w_init = w.copy()
    wd = torch.from_numpy(w.copy()).cuda()
    wd2 = wd.clone()
    m1 = np.zeros(N, np.float32)
    moments = np.zeros(len(LAYERS), np.float32)
    rng = np.random.default_rng(10)
    beta2 = float(np.float32(NOVOGRAD["beta2"]))
    for k in range(STEPS):
        g = R.gradients(rng, N)
        gd = torch.from_numpy(g).cuda()
        opt.step(wd, None, gd)
        twin.step(wd2, None, gd)  # determinism: a second run from the same state
        torch.cuda.synchronize()
        new = opt.state_named("per_layer_second_moments").cpu().numpy()
        assert new.shape == (len(LAYERS),)
        assert np.array_equal(new.view(np.uint32), twin.state_named("per_layer_second_moments").cpu().numpy().view(np.uint32)), k
        for l in range(len(LAYERS)):
            b, e = BEGINS[l], BEGINS[l + 1]
            b2 = 0.0 if k == 0 else beta2
            want = b2 * float(moments[l]) + (1.0 - b2) * R.novograd_norm64(g, b, e) / 128.0 / 128.0
            print(f"novograd step {k} layer {l}: second moment {new[l]!r} vs float64 {want!r}, relative error {abs(float(new[l]) - want) / want:.3e}")
            assert abs(float(new[l]) - want) <= ((e - b) + 2) * 2.0 ** -24 * want, (k, l)
            R.novograd_step_layer(NOVOGRAD, 128.0, k == 0, new[l], w, g, m1, b, e)
        moments = new
        assert _same(opt.state_named("first_moments"), m1), k
        assert _same(wd, w), k
    assert _same(wd2, w)
    assert np.array_equal(_bits(wd)[3072:], _bits(w_init)[3072:])
    assert opt.step_count == STEPS and opt.custom_weights() is None


def _within_ulps(w, w_ref, w_before, ulps=4):
    """tests/test_gpu_parity_full.py's helper: |w - w_ref| <= `ulps` units in the last place of the larger of the old weight, the new
    weight and the largest Adam update (~3 lr): the update is a difference, so a result close to zero carries the absolute error of its operands."""
    scale = np.maximum(np.maximum(np.abs(w_before), np.abs(w_ref)), np.float32(0.03))
    return bool((np.abs(w - w_ref) <= ulps * np.spacing(scale)).all())


def test_adam_against_the_oracle():
    n, nm = 40000, 4096
    cfg = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6, "non_matrix_learning_rate_factor": 0.5}
    adam = O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=1e-6, non_matrix_learning_rate_factor=0.5)
    rng = np.random.default_rng(5)
    w32 = rng.standard_normal(n).astype(np.float32)
    w16 = O.f2h(w32)
    m1, m2, steps = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    opt = _optimizer(cfg, n, n_matrix_weights=nm)
    wd = torch.from_numpy(w32.copy()).cuda()
    for k in range(4):
        g = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 60.0], n)).astype(np.float16)
        g[nm:][rng.random(n - nm) < 0.4] = 0
        opt.step(wd, None, torch.from_numpy(g.astype(np.float32)).cuda())
        w_before = w32.copy()
        O.adam_step(adam, nm, 128.0, k + 1, w32, w16, g.view(np.uint16), m1, m2, steps)
        gm1, gm2, gsteps = opt.state()
        torch.cuda.synchronize()
        assert opt.step_count == k + 1
        assert np.array_equal(gsteps.cpu().numpy().view(np.uint32), steps) and _same(gm1, m1) and _same(gm2, m2), k
        w = wd.cpu().numpy()
        assert _within_ulps(w, w32, w_before), k
        w32[:] = w
        w16[:] = O.f2h(w)
    assert len(np.unique(steps)) > 2


@pytest.mark.parametrize("with_pdf", [False, True], ids=["no_pdf", "data_pdf"])
@pytest.mark.parametrize("otype", R.LOSSES)
def test_loss_f32_against_the_16_bit_kernel(otype, with_pdf):
    from tinycudann import _C
    prediction, target, pdf = R.loss_case()
    dims = target.shape[1]
    prediction_h = O.f2h(prediction)
    assert np.array_equal(O.h2f(prediction_h), prediction)  # representable in the library's 16-bit type
    t = torch.from_numpy(target).cuda()
    p = torch.from_numpy(pdf).cuda() if with_pdf else None
    values, grads = _C.loss_evaluate(otype, torch.from_numpy(prediction).cuda(), t, 128.0, p)
    values_h, grads_h = _C.loss_evaluate(otype, h_t(prediction_h), t, 128.0, p)
    torch.cuda.synchronize()
    assert grads.dtype == torch.float32
    values, grads, values_h, grads_h = values.cpu().numpy(), grads.cpu().numpy(), values_h.cpu().numpy(), h_np(grads_h)
    assert not values[:, dims:].any() and not grads[:, dims:].any()  # padding rows carry no loss
    assert np.array_equal(values.view(np.uint32), values_h.view(np.uint32))
    g = grads[:, :dims]
    smallest_normal, largest = (2.0 ** -126, 3.38e38) if _C.preferred_precision() == _C.Precision.Bf16 else (2.0 ** -14, 65520.0)
    normal = (np.abs(g) >= smallest_normal) & (np.abs(g) < largest)
    excluded = 1.0 - normal.mean()
    print(f"{otype}: {100 * excluded:.3f} % of the fp32 gradients are no normal value of the 16-bit type")
    assert excluded < 0.01
    assert np.array_equal(grads_h[:, :dims][normal], O.f2h(g)[normal])


def test_serialize_deserialize_step_equals_the_uninterrupted_run():
    import msgpack
    cfg = {"otype": "Batched", "batch_size_multiplier": 3, "nested": {"otype": "Average", "n_samples": 3, "nested": {"otype": "Lookahead", "nested": {"otype": "Novograd"}}}}
    opt = _optimizer(cfg)
    wd = torch.from_numpy(R.weights(13)).cuda()
    rng = np.random.default_rng(14)
    for _ in range(5):  # (the sixth step, after the snapshot, runs the nested chain: 6 % 3 == 0)
        opt.step(wd, None, torch.from_numpy(R.gradients(rng, N)).cuda())
    data = opt.serialize()
    doc = msgpack.unpackb(data, raw=False)
    assert set(doc) == {"averaged_gradients_binary", "averaged_gradients_half_binary", "current_step", "nested"} and doc["current_step"] == 5
    assert len(doc["averaged_gradients_half_binary"]) == 4 * N  # float where the 16-bit chain writes 16-bit values
    assert len(doc["nested"]["weights_samples_binary"]) == 3 * N * 4 and len(doc["nested"]["nested"]["weights_lookahead_binary"]) == 4 * N
    twin = _optimizer(cfg)
    twin.deserialize(data)
    wd2 = wd.clone()
    g = torch.from_numpy(R.gradients(rng, N)).cuda()
    opt.step(wd, None, g)
    twin.step(wd2, None, g)
    torch.cuda.synchronize()
    assert twin.step_count == opt.step_count == 6
    assert _same(wd, wd2)
    for name in ("weights_average", "weights_samples", "weights_lookahead", "first_moments", "per_layer_second_moments", "averaged_gradients", "averaged_gradients_half"):
        assert _same(opt.state_named(name), twin.state_named(name)), name

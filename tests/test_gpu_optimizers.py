"""The stand-alone optimizer object (tcnn_create_optimizer / native.Optimizer) over buffers the caller owns, against the numpy restatement
(tests/optimizer_reference.py).

n_weights = 4099 (16-byte vector body, a ragged scalar tail of 3, a last partial workgroup; the Average ring's slots 1 and 2 are not 16-byte
aligned: the scalar form of the whole kernel), layers [(64, 32), (16, 64)] = 3072 matrix weights + 1027 others, gradients with magnitudes
mixed over 1e-3, 1, 60, 7 steps: Lookahead(n_steps = 3) pulls at nested counts 0, 3, 6; Average(n_samples = 3) wraps its ring twice;
Batched(batch_size_multiplier = 3) runs the nested step twice and ends on a partly filled pool.

Bars: SGD, Lookahead, Average, Batched (and Ema(ExponentialDecay(SGD))): master weights, 16-bit weights and every state buffer BIT-EQUAL
after every step (single-rounding fp32 operations under -ffp-contract=off; fp32 division and square root are correctly rounded in this
build).  Novograd: the per-layer second moment against a float64 sum of the squared fp32 gradients within (n_layer + 2) 2^-24 relative (a
sum of n non-negative fp32 terms in any order errs by at most n - 1 roundings, plus one per square and one for the moment's update); first
moments and weights bit-equal to the restatement fed with the second moment READ BACK from the library; two runs give the same bits; the
1027 non-matrix weights stay bit-unchanged."""
import numpy as np
import pytest
import torch

import optimizer_reference as R
from oracle import oracle as O
from test_gpu_parity import h_np, h_t

pytestmark = pytest.mark.gpu

N = 4099
LAYERS = [(64, 32), (16, 64)]
BEGINS = [0, 2048, 3072]
STEPS = 7
SGD_CFG = {"otype": "SGD", "learning_rate": 1e-2, "l2_reg": 1e-6}


def _native():
    from tinycudann import native
    return native


def _weights(seed):
    w32 = np.random.default_rng(seed).standard_normal(N).astype(np.float32)
    return w32, O.f2h(w32)


def _ref_sgd():
    return R.SGD(learning_rate=1e-2, l2_reg=1e-6)


CHAINS = {
    "SGD": (SGD_CFG, lambda: _ref_sgd(), {}),
    "Lookahead": ({"otype": "Lookahead", "alpha": 0.5, "n_steps": 3, "nested": SGD_CFG}, lambda: R.Lookahead(_ref_sgd(), N, alpha=0.5, n_steps=3),
                  {"weights_lookahead": "slow16"}),
    "Average": ({"otype": "Average", "n_samples": 3, "nested": SGD_CFG}, lambda: R.Average(_ref_sgd(), N, n_samples=3),
                {"weights_samples": "samples16", "weights_average": "average16"}),
    "Batched": ({"otype": "Batched", "batch_size_multiplier": 3, "nested": SGD_CFG}, lambda: R.Batched(_ref_sgd(), N, batch_size_multiplier=3),
                {"averaged_gradients": "pool", "averaged_gradients_half": "pool16"}),
}


def _bits(t):
    a = t.cpu().numpy() if t.dtype == torch.float32 else h_np(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(t, ref):
    return np.array_equal(_bits(t), ref.ravel().view(np.uint32) if ref.dtype == np.float32 else ref.ravel())


@pytest.mark.parametrize("which", list(CHAINS))
def test_sgd_and_wrappers_bit_equal(which):
    cfg, make_ref, state = CHAINS[which]
    opt, ref = _native().Optimizer(cfg, N, layer_sizes=LAYERS), make_ref()
    w32, w16 = _weights(5)
    wfp, wh = torch.from_numpy(w32.copy()).cuda(), h_t(w16.copy())
    rng = np.random.default_rng(6)
    for k in range(STEPS):
        g = R.gradients(rng, N)
        opt.step(wfp, wh, h_t(g))
        ref.step(128.0, w32, w16, g)
        torch.cuda.synchronize()
        assert opt.step_count == ref.step_count()
        assert _same(wfp, w32), k
        assert _same(wh, w16), k
        for name, attr in state.items():
            assert _same(opt.state_named(name), getattr(ref, attr)), (k, name)
    custom = opt.custom_weights()
    if which == "SGD":
        assert custom is None
    elif which == "Lookahead":
        assert custom.data_ptr() == opt.state_named("weights_lookahead").data_ptr()
    elif which == "Average":
        assert custom.data_ptr() == opt.state_named("weights_average").data_ptr()
        assert ref.nested.step_count() // 3 == 2  # the ring wrapped twice
    else:
        assert custom is None and opt.step_count == STEPS and ref.nested.step_count() == 2  # Batched passes its nested one's through
    h = opt.hyperparams()
    assert h["otype"] == which and (which == "SGD" or h["nested"]["otype"] == "SGD")


def test_batched_passes_the_nested_custom_weights_through():
    opt = _native().Optimizer({"otype": "Batched", "nested": {"otype": "Average", "n_samples": 2, "nested": SGD_CFG}}, N, layer_sizes=LAYERS)
    assert opt.custom_weights().data_ptr() == opt.state_named("weights_average").data_ptr()


NOVOGRAD = {"learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8, "relative_decay": 1e-3, "absolute_decay": 1e-4}


def test_novograd():
    native = _native()
    cfg = {"otype": "Novograd", **NOVOGRAD}
    opt, twin = native.Optimizer(cfg, N, layer_sizes=LAYERS), native.Optimizer(cfg, N, layer_sizes=LAYERS)
    w32, w16 = _weights(9)
    w_init32, w_init16 = w32.copy(), w16.copy()
    wfp, wh = torch.from_numpy(w32.copy()).cuda(), h_t(w16.copy())
    wfp2, wh2 = wfp.clone(), wh.clone()
    m1 = np.zeros(N, np.float32)
    moments = np.zeros(len(LAYERS), np.float32)
    rng = np.random.default_rng(10)
    beta2 = float(np.float32(NOVOGRAD["beta2"]))
    for k in range(STEPS):
        g = R.gradients(rng, N)
        opt.step(wfp, wh, h_t(g))
        twin.step(wfp2, wh2, h_t(g))  # determinism: a second run from the same state
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
            R.novograd_step_layer(NOVOGRAD, 128.0, k == 0, new[l], w32, w16, g, m1, b, e)
        moments = new
        assert _same(opt.state_named("first_moments"), m1), k
        assert _same(wfp, w32), k
        assert _same(wh, w16), k
    assert _same(wfp2, w32) and _same(wh2, w16)
    assert np.array_equal(wfp.cpu().numpy()[3072:].view(np.uint32), w_init32[3072:].view(np.uint32)) and np.array_equal(h_np(wh)[3072:], w_init16[3072:])
    assert opt.step_count == STEPS and opt.custom_weights() is None


def test_chain_ordering_ema_over_exponential_decay_over_sgd():
    """exponential_decay.h:59-70 with decay_start = 2, decay_interval = 2: the factor drops before the steps whose nested count is 2, 4, 6"""
    cfg = {"otype": "Ema", "decay": 0.9, "nested": {"otype": "ExponentialDecay", "decay_base": 0.5, "decay_start": 2, "decay_interval": 2, "nested": SGD_CFG}}
    opt = _native().Optimizer(cfg, N, layer_sizes=LAYERS)
    ref = R.Ema(R.ExponentialDecay(_ref_sgd(), decay_base=0.5, decay_interval=2, decay_start=2), N, decay=0.9)
    w32, w16 = _weights(11)
    wfp, wh = torch.from_numpy(w32.copy()).cuda(), h_t(w16.copy())
    rng = np.random.default_rng(12)
    schedule = []
    for k in range(STEPS):
        g = R.gradients(rng, N)
        opt.step(wfp, wh, h_t(g))
        ref.step(128.0, w32, w16, g)
        torch.cuda.synchronize()
        lr = opt.hyperparams()["nested"]["nested"]["learning_rate"]
        schedule.append(lr)
        assert np.float32(lr) == ref.nested.nested.learning_rate, k
        assert _same(wfp, w32) and _same(wh, w16), k
        assert _same(opt.state_named("weights_ema"), ref.ema16), k
    assert np.allclose(schedule, [1e-2, 1e-2, 5e-3, 5e-3, 2.5e-3, 2.5e-3, 1.25e-3], rtol=1e-6)
    assert opt.custom_weights().data_ptr() == opt.state_named("weights_ema").data_ptr() and opt.step_count == STEPS


def test_snapshot_keys_and_round_trip_of_the_stand_alone_object():
    import ctypes as C
    import msgpack
    from tinycudann._C import _check, _lib
    cfg = {"otype": "Batched", "batch_size_multiplier": 3, "nested": {"otype": "Average", "n_samples": 3, "nested": {"otype": "Lookahead", "nested": {"otype": "Novograd"}}}}
    opt = _native().Optimizer(cfg, N, layer_sizes=LAYERS)
    w32, w16 = _weights(13)
    wfp, wh = torch.from_numpy(w32).cuda(), h_t(w16)
    rng = np.random.default_rng(14)
    for _ in range(4):
        opt.step(wfp, wh, h_t(R.gradients(rng, N)))
    n = C.c_size_t(0)
    _check(_lib.tcnn_optimizer_serialize(opt._h, None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value)
    _check(_lib.tcnn_optimizer_serialize(opt._h, buf, n.value, C.byref(n)))
    doc = msgpack.unpackb(buf.raw[:n.value], raw=False)
    assert set(doc) == {"averaged_gradients_binary", "averaged_gradients_half_binary", "current_step", "nested"} and doc["current_step"] == 4
    assert set(doc["nested"]) == {"weights_samples_binary", "weights_average_binary", "nested"} and len(doc["nested"]["weights_samples_binary"]) == 3 * N * 2
    assert set(doc["nested"]["nested"]) == {"weights_lookahead_binary", "nested"}
    novograd = doc["nested"]["nested"]["nested"]
    assert set(novograd) == {"first_moments_binary", "per_layer_second_moments_binary", "current_step", "base_learning_rate"}
    assert novograd["current_step"] == 1 and len(novograd["per_layer_second_moments_binary"]) == 4 * len(LAYERS)
    twin = _native().Optimizer(cfg, N, layer_sizes=LAYERS)
    _check(_lib.tcnn_optimizer_deserialize(twin._h, buf.raw[:n.value], n.value))
    wfp2, wh2 = wfp.clone(), wh.clone()
    for _ in range(3):
        g = h_t(R.gradients(rng, N))
        opt.step(wfp, wh, g)
        twin.step(wfp2, wh2, g)
    torch.cuda.synchronize()
    assert twin.step_count == opt.step_count == 7
    assert torch.equal(wfp, wfp2) and torch.equal(wh.view(torch.int16), wh2.view(torch.int16))
    for name in ("weights_average", "weights_samples", "weights_lookahead", "first_moments", "per_layer_second_moments", "averaged_gradients"):
        a, b = opt.state_named(name), twin.state_named(name)
        assert torch.equal(a.view(torch.int16) if a.element_size() == 2 else a, b.view(torch.int16) if b.element_size() == 2 else b), name

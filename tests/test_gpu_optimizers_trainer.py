"""The optimizers besides Adam through create_from_config: config_hash(log2_hashmap_size = 12, per_level_scale = 1.5) with the 64 x 2 network
(weight matrices 64 x 32, 64 x 64, 16 x 64 = 7168 network weights in front of the grid's), batch 512.

The restatement (tests/optimizer_reference.py) is fed with the trainer's own 16-bit gradients (tm.param_gradients after the step), so the
bars are those of tests/test_gpu_optimizers.py: bit-equal master and 16-bit weights; Novograd with the per-layer second moments read back
from the trainer.  Where two TRAINERS are compared after training_step (finalize fusion on / off, graph capture on / off) the network's
weights are held to bits and the encoding's to the run-to-run spread of the grid backward's packed 16-bit atomics on the coarse levels
(the bar of tests/test_gpu_parity_full.py::test_training_step_as_one_graph_launch_leaves_the_plain_steps_bits: gradients differ in < 5 % of
the entries by at most 2^-8 of the largest); where the optimizer alone is under test (snapshots, ranged stepping) the gradients are
written into the trainer and everything is held to bits."""
import msgpack
import numpy as np
import pytest
import torch

import optimizer_reference as R
from conftest import config_hash
from oracle import oracle as O
from test_gpu_parity import h_np, h_t, positions, targets_for, tcnn

pytestmark = pytest.mark.gpu

N_BATCH = 512
NET_BEGINS = [0, 64 * 32, 64 * 32 + 64 * 64, 64 * 32 + 64 * 64 + 16 * 64]
SGD_CFG = {"otype": "SGD", "learning_rate": 1e-2, "l2_reg": 1e-6}
NOVOGRAD = {"learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8, "relative_decay": 1e-3, "absolute_decay": 1e-4}


def _trainer(optimizer, seed=1337):
    cfg = config_hash(log2_hashmap_size=12, per_level_scale=1.5)
    cfg["optimizer"] = optimizer
    tm = tcnn().create_from_config(3, 4, cfg, seed=seed)
    init = tm.params_full_precision.cpu().numpy().copy()
    init[tm.n_mlp_params:] *= 1.0e3  # grid.h:1076-1079 initialises in U(-1e-4, 1e-4): mostly fp16 subnormals
    tm.set_params_full_precision(torch.from_numpy(init))
    return tm


def _batch(seed):
    pos = positions(N_BATCH, 3, seed=seed)
    return torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()


def _bits32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("which", ["SGD", "Novograd", "Lookahead"])
def test_two_training_steps_match_the_restatement(which):
    optimizer = {"SGD": SGD_CFG, "Novograd": {"otype": "Novograd", **NOVOGRAD}, "Lookahead": {"otype": "Lookahead", "n_steps": 1, "alpha": 0.5, "nested": SGD_CFG}}[which]
    tm = _trainer(optimizer)
    n, nm = tm.n_params, tm.n_mlp_params
    assert nm == NET_BEGINS[-1]
    w32 = tm.params_full_precision.cpu().numpy()
    w16 = h_np(tm.params_view).copy()
    ref = {"SGD": R.SGD(1e-2, 1e-6), "Lookahead": R.Lookahead(R.SGD(1e-2, 1e-6), n, alpha=0.5, n_steps=1), "Novograd": None}[which]
    m1, moments = np.zeros(n, np.float32), np.zeros(3, np.float32)
    for k in range(2):
        x, t = _batch(40 + k)
        tm.training_step(x, t)
        torch.cuda.synchronize()
        g = h_np(tm.param_gradients).copy()
        assert np.any(g[:nm] != 0) and np.any(g[nm:] != 0)
        if ref is not None:
            ref.step(128.0, w32, w16, g)
        else:
            new = tm.optimizer_state_named("per_layer_second_moments").cpu().numpy()
            for l in range(3):
                b, e = NET_BEGINS[l], NET_BEGINS[l + 1]
                b2 = 0.0 if k == 0 else float(np.float32(NOVOGRAD["beta2"]))
                want = b2 * float(moments[l]) + (1.0 - b2) * R.novograd_norm64(g, b, e) / 128.0 / 128.0
                assert abs(float(new[l]) - want) <= ((e - b) + 2) * 2.0 ** -24 * want, (k, l)
                R.novograd_step_layer(NOVOGRAD, 128.0, k == 0, new[l], w32, w16, g, m1, b, e)
            moments = new
        assert np.array_equal(_bits32(tm.params_full_precision), w32.view(np.uint32)), k
        assert np.array_equal(h_np(tm.params_view), w16), k
        assert tm.optimizer_step_count == k + 1
    if which == "Lookahead":
        assert np.array_equal(h_np(tm.params_inference), ref.slow16)
        assert tm.params_inference.data_ptr() == tm.optimizer_state_named("weights_lookahead").data_ptr() != tm.params_view.data_ptr()
    else:
        assert tm.params_inference.data_ptr() == tm.params_view.data_ptr()  # no wrapper with weights of its own
    if which == "Novograd":  # the encoding's parameters are never stepped (layer_sizes() are the network's matrices)
        init = _trainer(optimizer).params_full_precision
        assert torch.equal(tm.params_full_precision[nm:], init[nm:])
    assert tm.hyperparams()["optimizer"]["otype"] == which


def test_transposed_network_weights_are_not_stale_after_a_non_adam_step():
    """the backward kernels read a transposed copy of the network weights that only Adam's step keeps current"""
    tm = _trainer(SGD_CFG)
    x, t = _batch(50)
    for _ in range(2):
        tm.training_step(x, t)
    fresh = _trainer(SGD_CFG, seed=7)
    fresh.set_params_full_precision(tm.params_full_precision)
    dx, dx_fresh = torch.zeros((N_BATCH, 3), device="cuda"), torch.zeros((N_BATCH, 3), device="cuda")
    c = tm.forward(x, t, prepare_input_gradients=True)
    tm.backward(c, x, dL_dinput=dx)
    cf = fresh.forward(x, t, prepare_input_gradients=True)
    fresh.backward(cf, x, dL_dinput=dx_fresh)
    torch.cuda.synchronize()
    assert float(dx.abs().max()) > 0 and torch.equal(dx, dx_fresh)
    dx2, dx2_fresh = torch.zeros_like(dx), torch.zeros_like(dx)
    tm.training_step(x, t, run_optimizer=False, dL_dinput=dx2)
    fresh.training_step(x, t, run_optimizer=False, dL_dinput=dx2_fresh)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx2_fresh)


def _spread_ok(ga, gb):
    d = (ga.float() - gb.float()).abs()
    return float(d.max()) <= 2.0 ** -8 * float(ga.float().abs().max()) and float((d > 0).float().mean()) < 0.05


def _compare_trainers(a, b, lr=1e-2):
    """after ONE step from identical states"""
    nm = a.n_mlp_params
    assert torch.equal(a.params_full_precision[:nm].view(torch.int32), b.params_full_precision[:nm].view(torch.int32))
    assert torch.equal(a.params_view[:nm].view(torch.int16), b.params_view[:nm].view(torch.int16))
    ga, gb = a.param_gradients, b.param_gradients
    assert torch.equal(ga[:nm].view(torch.int16), gb[:nm].view(torch.int16)) and _spread_ok(ga[nm:], gb[nm:])
    # SGD moves a weight by lr * g / 128: the encoding's weights differ by what the gradients' spread allows (+ one rounding of the weight)
    bound = lr / 128.0 * 2.0 ** -8 * float(ga[nm:].float().abs().max()) + 2.0 ** -23 * float(a.params_full_precision[nm:].abs().max())
    assert float((a.params_full_precision[nm:] - b.params_full_precision[nm:]).abs().max()) <= bound
    assert a.optimizer_step_count == b.optimizer_step_count


def _resync(b, a):
    """b takes a's state: optimizer and parameters through a snapshot, the master weights' extra bits directly"""
    b.deserialize(a.serialize(serialize_optimizer=True))
    master = a.params_full_precision  # a copy made on torch's current stream; the library copies from it on the null stream
    torch.cuda.synchronize()
    b.set_params_full_precision(master)


def test_finalize_fusion_is_bypassed_for_sgd():
    """tcnn_set_finalize_in_optimizer on and off: the weight-gradient slabs are summed by their own launch either way"""
    T = tcnn()
    a, b = _trainer(SGD_CFG), _trainer(SGD_CFG, seed=5)
    try:
        for step in range(2):
            x, t = _batch(60 + step)
            _resync(b, a)
            T._C.set_finalize_in_optimizer(True)
            a.training_step(x, t)
            T._C.set_finalize_in_optimizer(False)
            b.training_step(x, t)
            torch.cuda.synchronize()
            _compare_trainers(a, b)
    finally:
        T._C.set_finalize_in_optimizer(True)


@pytest.mark.parametrize("which", ["Batched", "Lookahead"])
def test_training_step_under_graph_capture(which):
    """every step from identical states, as the Adam test of the captured step does; the chain's launches change from step to step (the
    nested step of Batched and the pull of Lookahead run every second call): the graph is re-instantiated, the bits stay"""
    optimizer = {"Batched": {"otype": "Batched", "batch_size_multiplier": 2, "nested": SGD_CFG}, "Lookahead": {"otype": "Lookahead", "n_steps": 2, "nested": SGD_CFG}}[which]
    a, b = _trainer(optimizer), _trainer(optimizer, seed=5)
    a.set_graph_capture(True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for step in range(5):
            x, t = _batch(70 + step)
            _resync(b, a)
            side.synchronize()
            a.training_step(x, t, want_context=False)
            b.training_step(x, t, want_context=False)
            side.synchronize()
            _compare_trainers(a, b)
            if which == "Lookahead":
                nm = a.n_mlp_params
                assert torch.equal(a.params_inference[:nm].view(torch.int16), b.params_inference[:nm].view(torch.int16))
    assert a.graph_capture_stats()[0] == 4 and b.graph_capture_stats() == (0, 0)
    assert a.optimizer_step_count == 5


def _write_gradients(tm, rng):
    g = R.gradients(rng, tm.n_params)
    tm.param_gradients.copy_(h_t(g))
    return g


@pytest.mark.parametrize("which", ["Novograd", "Average"])
def test_snapshot_resumes_to_the_same_bits(which):
    optimizer = {"Novograd": {"otype": "Novograd", **NOVOGRAD}, "Average": {"otype": "Average", "n_samples": 2, "nested": SGD_CFG}}[which]
    a, b = _trainer(optimizer), _trainer(optimizer, seed=3)
    rng = np.random.default_rng(80)
    for _ in range(3):
        _write_gradients(a, rng)
        a.optimizer_step()
    blob = a.serialize(serialize_optimizer=True)
    doc = msgpack.unpackb(blob, raw=False)
    o = doc["optimizer"]
    if which == "Novograd":
        assert set(o) == {"first_moments_binary", "per_layer_second_moments_binary", "current_step", "base_learning_rate"}
        assert o["current_step"] == 3 and len(o["per_layer_second_moments_binary"]) == 12 and len(o["first_moments_binary"]) == 4 * a.n_params
    else:
        assert set(o) == {"weights_samples_binary", "weights_average_binary", "nested"} and set(o["nested"]) == {"current_step", "learning_rate"}
        assert len(o["weights_samples_binary"]) == 2 * 2 * a.n_params and o["nested"]["current_step"] == 3
        assert doc["params_binary"] == bytes(h_np(a.params_inference).tobytes())  # trainer.h:448: the inference parameters
    b.deserialize(blob)
    b.set_params_full_precision(a.params_full_precision)  # (the snapshot holds 16-bit parameters; the master weights' extra bits travel here)
    assert b.optimizer_step_count == 3
    g = _write_gradients(a, rng)
    b.param_gradients.copy_(h_t(g))
    a.optimizer_step()
    b.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(a.params_full_precision.view(torch.int32), b.params_full_precision.view(torch.int32))
    assert torch.equal(a.params_view.view(torch.int16), b.params_view.view(torch.int16))
    assert torch.equal(a.params_inference.view(torch.int16), b.params_inference.view(torch.int16))
    name = "first_moments" if which == "Novograd" else "weights_samples"
    sa, sb = a.optimizer_state_named(name), b.optimizer_state_named(name)
    assert torch.equal(sa.view(torch.int16) if sa.element_size() == 2 else sa, sb.view(torch.int16) if sb.element_size() == 2 else sb)


def test_ranged_stepping():
    a, b = _trainer(SGD_CFG), _trainer(SGD_CFG)
    g = _write_gradients(a, np.random.default_rng(90))
    b.param_gradients.copy_(h_t(g))
    a.optimizer_step()
    cut = 4096 + 8
    b.optimizer_step_range(0, cut)
    b.optimizer_step_range(cut, b.n_params)
    torch.cuda.synchronize()
    assert a.optimizer_step_count == b.optimizer_step_count == 1
    assert torch.equal(a.params_full_precision.view(torch.int32), b.params_full_precision.view(torch.int32))
    assert torch.equal(a.params_view.view(torch.int16), b.params_view.view(torch.int16))
    for optimizer, name in (({"otype": "Novograd"}, "Novograd"), ({"otype": "Lookahead", "nested": SGD_CFG}, "Lookahead"),
                            ({"otype": "Ema", "nested": {"otype": "Average", "nested": SGD_CFG}}, "Average"), ({"otype": "Batched", "nested": {"otype": "Adam"}}, "Batched")):
        tm = _trainer(optimizer)
        before = tm.params_full_precision
        with pytest.raises(RuntimeError, match=name):
            tm.optimizer_step_range(0, 4096)
        with pytest.raises(RuntimeError, match=name):
            tm.optimizer_step_ranges([(0, 4096)])
        assert torch.equal(before, tm.params_full_precision) and tm.optimizer_step_count == 0
    with pytest.raises(RuntimeError, match="not Adam"):
        _trainer(SGD_CFG).optimizer_state()

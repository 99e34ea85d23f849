"""The host side of the fp32 optimizers and losses (no GPU, no compute calls): the header declares tcnn_create_optimizer_precision,
tcnn_optimizer_precision, tcnn_loss_evaluate_precision and tcnn_module_network_layers and the library exports them;
create_optimizer_precision with the library's own precision is create_optimizer (hyperparameters, step count 0, the refusals' texts), with
TCNN_PRECISION_FP32 it reports fp32 and round-trips update_hyperparams for every chain of tests/test_library_optimizers.py; the other
16-bit precision is refused by name; network_layers() of a module are the weight matrices that lead its parameter vector."""
import itertools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tcnn_create_optimizer_precision", "tcnn_optimizer_precision", "tcnn_loss_evaluate_precision", "tcnn_module_network_layers"]


def _native():
    from tinycudann import native
    return native


def _C():
    from tinycudann import _C
    return _C


def _optimizer(cfg, precision=None):
    return _native().Optimizer(cfg, 0, precision=precision)  # n_weights = 0: nothing is allocated, the device is not touched


def _chains():
    yield {"otype": "SGD"}
    yield {"otype": "Novograd"}
    yield {"otype": "Adam"}
    for wrapper in ("Lookahead", "Average", "Batched", "Ema", "ExponentialDecay"):
        yield {"otype": wrapper, "nested": {"otype": "SGD"}}
    for base in ("Adam", "SGD", "Novograd"):
        for order in itertools.islice(itertools.permutations(["Ema", "ExponentialDecay", "Lookahead", "Average", "Batched"]), 0, 120, 7):
            cfg = {"otype": base}
            for w in reversed(order):
                cfg = {"otype": w, "nested": cfg}
            yield cfg
    yield {"otype": "ExponentialDecay", "decay_base": 0.5, "nested": {"otype": "Lookahead", "nested": {"otype": "Novograd", "learning_rate": 0.125}}}


def test_header_declares_and_library_exports_the_new_entries():
    header = open(os.path.join(ROOT, "include", "tcnn_hip.h")).read()
    for name in NEW_ENTRIES:
        assert name + "(" in header, name
        assert name in _C().EXPORTED_SYMBOLS, name
        assert hasattr(_C()._lib, name)


def test_native_precision_is_create_optimizer():
    C = _C()
    native_precision = C.preferred_precision()
    for cfg in _chains():
        a, b = _optimizer(cfg), _optimizer(cfg, native_precision)
        assert a.precision == b.precision == native_precision
        assert a.hyperparams() == b.hyperparams() and a.step_count == b.step_count == 0


REFUSED = [
    ({"otype": "Shampoo"}, "not available"),
    ({"otype": "Composite", "nested": [{"otype": "SGD"}]}, "Composite"),
    ({"otype": "Lookahead", "nested": {"otype": "NoSuchOptimizer"}}, "not available"),
    ({"otype": "Lookahead", "n_steps": 0, "nested": {"otype": "SGD"}}, "must be positive"),
] + [({"otype": w, "nested": {"otype": "Batched" if w != "Batched" else "Average", "nested": {"otype": w, "nested": {"otype": "SGD"}}}}, "nested .* inside")
     for w in ("Lookahead", "Average", "Batched", "Ema", "ExponentialDecay")]


@pytest.mark.parametrize("cfg,match", REFUSED)
def test_the_same_chains_are_refused_with_the_same_texts(cfg, match):
    C = _C()
    texts = []
    for precision in (None, C.preferred_precision(), C.Precision.Fp32):
        with pytest.raises(RuntimeError, match=match) as e:
            _optimizer(cfg, precision)
        texts.append(str(e.value))
    assert texts[0] == texts[1] == texts[2]


def test_fp32_reports_fp32_and_round_trips_hyperparams():
    C = _C()
    for cfg in _chains():
        opt, half = _optimizer(cfg, C.Precision.Fp32), _optimizer(cfg)
        assert opt.precision == C.Precision.Fp32
        h = opt.hyperparams()
        assert h == half.hyperparams() and opt.step_count == 0 and opt.custom_weights() is None
        opt.update_hyperparams(h)  # what hyperparams() gave goes back in
        assert opt.hyperparams() == h
        base = h
        path = {}
        cur = path
        while "nested" in base:
            base = base["nested"]
            cur["nested"] = {}
            cur = cur["nested"]
        cur["learning_rate"] = 0.25
        opt.update_hyperparams(path)
        got = opt.hyperparams()
        while "nested" in got:
            got = got["nested"]
        assert got["learning_rate"] == 0.25 and got["otype"] == base["otype"]
    opt = _optimizer({"otype": "Lookahead", "nested": {"otype": "SGD"}}, C.Precision.Fp32)
    with pytest.raises(RuntimeError, match="structure does not match"):
        opt.update_hyperparams({"otype": "Average", "nested": {"otype": "SGD"}})
    with pytest.raises(RuntimeError, match="no state buffer"):
        opt.state_named("weights_average")


def test_the_other_16_bit_precision_is_refused_by_name():
    C = _C()
    other = C.Precision.Bf16 if C.preferred_precision() == C.Precision.Fp16 else C.Precision.Fp16
    with pytest.raises(RuntimeError, match="not %s ones" % other.name.lower()):
        _optimizer({"otype": "SGD"}, other)
    import ctypes
    assert C._lib.tcnn_loss_evaluate_precision(b"L2", None, 1, 8, 1, 1.0, int(other), None, None, None, None, None) != 0
    assert ("not %s ones" % other.name.lower()).encode() in C._lib.tcnn_last_error()
    del ctypes


MLP_64x2 = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
HASHGRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}


def _n_matrix(layers):
    return sum(r * c for r, c in layers)


def test_network_layers():
    C = _C()
    net = C.create_network(3, 4, MLP_64x2)
    assert net.network_layers() == [(64, 16), (64, 64), (16, 64)] and _n_matrix(net.network_layers()) == net.n_params()
    encoding = C.create_encoding(3, HASHGRID)
    assert encoding.network_layers() == []
    nwie = C.create_network_with_input_encoding(3, 4, HASHGRID, {**MLP_64x2, "n_neurons": 128, "n_hidden_layers": 4})
    layers = nwie.network_layers()
    assert layers == [(128, 16)] + [(128, 128)] * 3 + [(16, 128)]
    assert _n_matrix(layers) == nwie.n_params() - encoding.n_params()
    wide = C.create_network_with_input_encoding_precision(3, 4, HASHGRID, {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 272,
                                                                         "n_hidden_layers": 2}, C.Precision.Fp32)
    layers = wide.network_layers()
    assert len(layers) == 3 and layers[1] == (272, 272) and layers[0][0] == 272 and layers[2][1] == 272
    assert _n_matrix(layers) == wide.n_params() - C.create_encoding(3, HASHGRID, C.Precision.Fp32).n_params()

"""The optimizer chains' host side (no GPU, no compute calls): tcnn_create_optimizer / native.Optimizer build every chain of the wrappers
Ema, ExponentialDecay, Lookahead, Average, Batched around one base out of Adam, SGD, Novograd without touching the device; hyperparams()
carries the reference's keys, otype spellings and defaults (sgd.h:139-140, novograd.h:247-254, lookahead.h:163-164, average.h:166,
batched.h:155) and round-trips through update_hyperparams; Composite, Shampoo, a wrapper nested in itself and unknown otypes are refused;
the C++ facade compiles for the host with a caller that builds Lookahead(SGD)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _native():
    from tinycudann import native
    return native


def _optimizer(cfg):
    return _native().Optimizer(cfg, 0)  # n_weights = 0: nothing is allocated, the device is not touched


DEFAULTS = {
    "SGD": {"otype": "SGD", "learning_rate": 1e-3, "l2_reg": 1e-8},
    "Novograd": {"otype": "Novograd", "beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8, "learning_rate": 1e-3, "relative_decay": 0.0, "absolute_decay": 0.0},
}
WRAPPER_DEFAULTS = {
    "Lookahead": {"alpha": 0.5, "n_steps": 16},
    "Average": {"n_samples": 128},
    "Batched": {"batch_size_multiplier": 16},
}


def _close(a, b):
    return a == b if isinstance(b, (str, bool)) else abs(a - b) <= 1e-6 * abs(b)


@pytest.mark.parametrize("base", ["SGD", "Novograd"])
def test_base_defaults_and_keys(base):
    h = _optimizer({"otype": base}).hyperparams()
    assert set(h) == set(DEFAULTS[base])
    assert all(_close(h[k], v) for k, v in DEFAULTS[base].items()), h


@pytest.mark.parametrize("wrapper", ["Lookahead", "Average", "Batched"])
def test_wrapper_defaults_keys_and_round_trip(wrapper):
    opt = _optimizer({"otype": wrapper, "nested": {"otype": "SGD"}})
    h = opt.hyperparams()
    assert h["otype"] == wrapper and set(h) == {"otype", "nested", *WRAPPER_DEFAULTS[wrapper]}
    assert all(h[k] == v for k, v in WRAPPER_DEFAULTS[wrapper].items()), h
    assert h["nested"]["otype"] == "SGD"
    changed = {"otype": wrapper, "nested": {"otype": "SGD", "learning_rate": 0.25, "l2_reg": 0.0}, **{k: 3 if isinstance(v, int) else 0.25 for k, v in WRAPPER_DEFAULTS[wrapper].items()}}
    opt.update_hyperparams(changed)
    assert opt.hyperparams() == changed
    opt.update_hyperparams(h)  # what hyperparams() gave goes back in
    assert opt.hyperparams() == h


def test_every_order_of_all_wrappers_builds():
    import itertools
    for base in ("Adam", "SGD", "Novograd"):
        for order in itertools.islice(itertools.permutations(["Ema", "ExponentialDecay", "Lookahead", "Average", "Batched"]), 0, 120, 7):
            cfg = {"otype": base}
            for w in reversed(order):
                cfg = {"otype": w, "nested": cfg}
            h = _optimizer(cfg).hyperparams()
            seen = []
            while "nested" in h:
                seen.append(h["otype"])
                h = h["nested"]
            assert seen == ["EMA" if w == "Ema" else w for w in order] and h["otype"] == base


def test_learning_rate_reaches_the_base_through_exponential_decay():
    opt = _optimizer({"otype": "ExponentialDecay", "decay_base": 0.5, "nested": {"otype": "Lookahead", "nested": {"otype": "Novograd", "learning_rate": 0.125}}})
    assert opt.hyperparams()["nested"]["nested"]["learning_rate"] == 0.125
    opt.update_hyperparams({"nested": {"nested": {"learning_rate": 0.5}}})
    h = opt.hyperparams()
    assert h["decay_base"] == 0.5 and h["nested"]["nested"]["learning_rate"] == 0.5 and h["nested"]["nested"]["otype"] == "Novograd"


def test_refusals():
    with pytest.raises(RuntimeError, match="not available"):
        _optimizer({"otype": "Shampoo"})
    with pytest.raises(RuntimeError, match="Composite"):
        _optimizer({"otype": "Composite", "nested": [{"otype": "SGD"}]})
    with pytest.raises(RuntimeError, match="not available"):
        _optimizer({"otype": "Lookahead", "nested": {"otype": "NoSuchOptimizer"}})
    for w in ("Lookahead", "Average", "Batched", "Ema", "ExponentialDecay"):
        with pytest.raises(RuntimeError, match="nested .* inside"):
            _optimizer({"otype": w, "nested": {"otype": "Batched" if w != "Batched" else "Average", "nested": {"otype": w, "nested": {"otype": "SGD"}}}})
    opt = _optimizer({"otype": "Lookahead", "nested": {"otype": "SGD"}})
    with pytest.raises(RuntimeError, match="structure does not match"):
        opt.update_hyperparams({"otype": "Average", "nested": {"otype": "SGD"}})
    with pytest.raises(RuntimeError, match="structure does not match"):
        opt.update_hyperparams({"otype": "Lookahead", "nested": {"otype": "Adam"}})
    for bad in ({"otype": "Lookahead", "n_steps": 0}, {"otype": "Average", "n_samples": 0}, {"otype": "Batched", "batch_size_multiplier": 0}):
        with pytest.raises(RuntimeError, match="must be positive"):
            _optimizer({**bad, "nested": {"otype": "SGD"}})
    with pytest.raises(RuntimeError, match="no state buffer"):
        opt.state_named("weights_average")
    assert opt.custom_weights() is None and opt.step_count == 0  # nothing allocated


def test_cpp_facade_builds_lookahead_over_sgd(tmp_path):
    """the compile command of tests/test_library.py::test_cpp_facade_headers_compile_for_the_host (built-in JSON value)"""
    src = tmp_path / "caller.cpp"
    src.write_text(r'''
#include <tiny-cuda-nn/config.h>
using namespace tcnn;
int caller(hipStream_t stream, float* master, precision_t* weights, const precision_t* gradients) {
	json sgd = json::object();
	sgd["otype"] = "SGD";
	json config = json::object();
	config["otype"] = "Lookahead";
	config["nested"] = sgd;
	std::shared_ptr<Optimizer<precision_t>> opt{create_optimizer<precision_t>(config)};
	opt->allocate(4099, {{64, 32}, {16, 64}});
	opt->step(stream, 128.0f, master, weights, gradients);
	opt->set_learning_rate(opt->learning_rate() * 0.5f);
	opt->update_hyperparams(opt->hyperparams());
	precision_t* slow = opt->custom_weights();
	std::vector<uint8_t> state = opt->serialize();
	opt->deserialize(state);
	return (int)opt->step() + (int)opt->n_nested() + (int)opt->nested(0)->n_nested() + (int)opt->n_weights() + (slow ? 1 : 0);
}
''')
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

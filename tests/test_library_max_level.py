"""max_level / set_max_level_gpu of the grid encoding, host side (no GPU): the C ABI entry points of both libraries, setters and getters
through the ctypes binding and the compiled binding, the defaults, the refusals for everything but a lone grid, and the C++ facade's
methods under the reference's names (encodings/multi_level_interface.h:101-123)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}
NET_64 = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
NESTED_GRID = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "Identity"}, dict(GRID, n_dims_to_encode=3)]}
ENTRY_POINTS = ["tcnn_module_set_max_level", "tcnn_module_max_level", "tcnn_module_set_max_level_gpu",
                "tcnn_trainer_set_max_level", "tcnn_trainer_max_level", "tcnn_trainer_set_max_level_gpu"]


def _lib():
    import tinycudann
    return tinycudann._C


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    C = _lib()
    if request.param == "compiled" and C.EXT is None:
        pytest.skip("the compiled binding is not built")
    if request.param == "ctypes":
        monkeypatch.setattr(C, "EXT", None)
    return request.param


@pytest.mark.parametrize("lib_name", ["libtcnn_hip.so", "libtcnn_hip_bf16.so"])
def test_c_abi_entry_points_exist_in_both_libraries(lib_name):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tiny-cuda-nn_amd", "lib", lib_name)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in ENTRY_POINTS if s not in exported]
    header = open(os.path.join(ROOT, "include", "tcnn_hip.h")).read()
    assert not [s for s in ENTRY_POINTS if s + "(" not in header]


def test_defaults_and_round_trip(binding):
    C = _lib()
    for m in (C.create_encoding(3, GRID), C.create_encoding(3, GRID, C.Precision.Fp32), C.create_network_with_input_encoding(3, 4, GRID, NET_64)):
        assert type(m).__name__ == ("ExtModule" if binding == "compiled" else "Module")
        assert m.max_level() == 1.0
        for v in (0.5, 0.25, 2.0, 0.0, 1.0):
            m.set_max_level(v)
            assert m.max_level() == v
        m.set_max_level_gpu(None)  # clearing what was never set is fine
        assert "max_level" not in str(m.hyperparams())  # run-time state, not a hyperparameter


def test_both_bindings_drive_the_same_state():
    """a value set through the compiled binding's method is what the C ABI reports for the same native module, and the other way round"""
    C = _lib()
    if C.EXT is None:
        pytest.skip("the compiled binding is not built")
    m = C.create_encoding(3, GRID)
    assert type(m).__name__ == "ExtModule"
    m.set_max_level(0.375)
    v = ctypes.c_float()
    assert C._lib.tcnn_module_max_level(m._h, ctypes.byref(v)) == 0 and v.value == 0.375
    assert C._lib.tcnn_module_set_max_level(m._h, 0.75) == 0
    assert m.max_level() == 0.75 and C.Module.max_level(m) == 0.75


@pytest.mark.parametrize("make,named", [
    (lambda C: C.create_encoding(3, {"otype": "Frequency", "n_frequencies": 4}), "FrequencyEncoding"),
    (lambda C: C.create_encoding(6, NESTED_GRID), "CompositeEncoding"),
    (lambda C: C.create_network_with_input_encoding(6, 4, NESTED_GRID, NET_64), "CompositeEncoding"),
    (lambda C: C.create_network(16, 4, NET_64), "IdentityEncoding"),
], ids=["frequency", "composite-with-grid", "network-over-composite", "bare-network"])
def test_refused_for_everything_but_a_lone_grid(binding, make, named):
    C = _lib()
    m = make(C)
    for call in (lambda: m.set_max_level(0.5), lambda: m.max_level(), lambda: m.set_max_level_gpu(None)):
        with pytest.raises(RuntimeError, match=named):
            call()
    v = ctypes.c_float()
    assert C._lib.tcnn_module_set_max_level(m._h, 0.5) == 2 and named.encode() in C._lib.tcnn_last_error()  # TCNN_ERROR_UNSUPPORTED
    assert C._lib.tcnn_module_max_level(m._h, ctypes.byref(v)) == 2
    assert C._lib.tcnn_module_set_max_level_gpu(m._h, None) == 2


def test_set_max_level_gpu_wants_a_float32_gpu_tensor(binding):
    import torch
    m = _lib().create_encoding(3, GRID)
    for bad in (torch.zeros(256), torch.zeros(256, dtype=torch.float64), torch.zeros(16, 16)):
        with pytest.raises((RuntimeError, TypeError)):
            m.set_max_level_gpu(bad)


def test_trainer_entry_points_host_side():
    """the trainer's three, through the C ABI alone (creating a trainable model allocates on a device, so only the refusals' text is
    checked here; tests/test_gpu_max_level.py drives them)"""
    C = _lib()
    for name in ENTRY_POINTS[3:]:
        assert hasattr(C._lib, name)
    from tinycudann import native
    assert isinstance(native.TrainableModel.max_level, property) and callable(native.TrainableModel.set_max_level_gpu)


def test_torch_module_surface():
    import tinycudann as T
    assert isinstance(T.modules.Module.max_level, property) and callable(T.modules.Module.set_max_level_gpu)


def test_cpp_facade_exposes_the_reference_names(tmp_path):
    """a caller spelled like instant-ngp's (network->encoding()->set_max_level(...), set_max_level_gpu(float*)) and one of cpp_api.h's module
    compile for the host with g++"""
    src = tmp_path / "caller.cpp"
    src.write_text(r'''
#include <tiny-cuda-nn/config.h>
#include <tiny-cuda-nn/cpp_api.h>
using namespace tcnn;
float caller(json config, float* per_sample) {
	TrainableModel m = create_from_config(3, 4, config);
	std::shared_ptr<MultiLevelEncoding<precision_t>> enc = m.network->encoding();
	enc->set_max_level(0.5f);
	enc->set_max_level_gpu(per_sample);
	float* back = enc->max_level_gpu();
	enc->set_max_level_gpu(nullptr);
	cpp::Module* mod = cpp::create_encoding(3, config.value("encoding", json::object()), cpp::Precision::Fp16);
	auto* hip = static_cast<cpp::HipModule*>(mod);
	hip->set_max_level(0.25f);
	hip->set_max_level_gpu(per_sample);
	float v = hip->max_level() + enc->max_level() + (hip->max_level_gpu() == back ? 1.0f : 0.0f);
	delete mod;
	return v;
}
''')
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

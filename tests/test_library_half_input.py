"""16-bit inputs of the network modules, host side (no GPU): the four C ABI entry points in both libraries and in the header, which modules
report support (exactly those create_network makes), the refusals of every other one -- TCNN_ERROR_UNSUPPORTED with the encoding's name,
before anything touches a device -- through the ctypes binding and the compiled one, and the C++ facade's methods."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}
NESTED = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "Identity"}, {"n_dims_to_encode": 3, "otype": "TriangleWave", "n_frequencies": 4}]}
ENTRY_POINTS = ["tcnn_module_supports_half_input", "tcnn_module_inference_half_input", "tcnn_module_forward_half_input", "tcnn_module_backward_half_input"]


def _net(width, otype=None, n_hidden_layers=2):
    otype = otype or ("FullyFusedMLP" if width in (16, 32, 64, 128) else "CutlassMLP")
    return {"otype": otype, "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": n_hidden_layers}


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


@pytest.mark.parametrize("width", [16, 64, 128, 256])
@pytest.mark.parametrize("n_in,n_out", [(3, 4), (16, 16), (20, 3), (64, 144), (32, 256)])
def test_supported_by_every_bare_network(binding, width, n_in, n_out):
    C = _lib()
    m = C.create_network(n_in, n_out, _net(width))
    assert type(m).__name__ == ("ExtModule" if binding == "compiled" else "Module")
    assert m.supports_half_input() is True
    assert C._lib.tcnn_module_supports_half_input(m._h) == 1


def test_supported_whatever_the_activation_or_the_way_the_identity_was_asked_for(binding):
    C = _lib()
    assert C.create_network(8, 4, dict(_net(64, "CutlassMLP"), activation="Sine")).supports_half_input()
    assert C.create_network_with_input_encoding(8, 4, {"otype": "Identity"}, _net(64)).supports_half_input()  # what create_network makes, spelled out


REFUSED = [
    (lambda C: C.create_encoding(3, GRID), "GridEncoding"),
    (lambda C: C.create_encoding(3, GRID, C.Precision.Fp32), "GridEncoding"),
    (lambda C: C.create_encoding(3, {"otype": "Frequency", "n_frequencies": 4}), "FrequencyEncoding"),
    (lambda C: C.create_encoding(16, {"otype": "Identity"}), "IdentityEncoding"),
    (lambda C: C.create_network_with_input_encoding(3, 4, GRID, _net(64)), "GridEncoding"),
    (lambda C: C.create_network_with_input_encoding(6, 4, NESTED, _net(64)), "CompositeEncoding"),
    (lambda C: C.create_network_with_input_encoding(16, 4, {"otype": "Identity", "scale": 2.0}, _net(64)), "IdentityEncoding"),
    (lambda C: C.create_network_with_input_encoding(16, 4, {"otype": "Identity", "offset": 0.5}, _net(64)), "IdentityEncoding"),
]
REFUSED_IDS = ["hashgrid", "hashgrid-fp32", "frequency", "bare-identity", "network-over-grid", "network-over-composite", "identity-scaled", "identity-offset"]


@pytest.mark.parametrize("make,named", REFUSED, ids=REFUSED_IDS)
def test_refused_for_every_other_module(binding, make, named):
    """the three calls come back with TCNN_ERROR_UNSUPPORTED (2) and the encoding's name as the last error; the pointers are never looked at"""
    C = _lib()
    m = make(C)
    assert m.supports_half_input() is False
    assert C._lib.tcnn_module_supports_half_input(m._h) == 0
    L = C._lib
    h = ctypes.c_void_p()
    calls = [lambda: L.tcnn_module_inference_half_input(m._h, None, 256, None, None, None),
             lambda: L.tcnn_module_forward_half_input(m._h, None, 256, None, None, None, 1, ctypes.byref(h)),
             lambda: L.tcnn_module_backward_half_input(m._h, None, None, 256, None, None, None, None, None, None)]
    for call in calls:
        assert L.tcnn_module_grid_level_n_params(m._h, 1 << 20, ctypes.byref(ctypes.c_size_t())) == 1  # (another last error: the one checked next is this call's)
        assert b"half_input" not in L.tcnn_last_error()
        assert call() == 2
        assert named.encode() in L.tcnn_last_error() and b"half_input" in L.tcnn_last_error()
    assert h.value is None  # no context was made


def test_both_bindings_ask_the_library(binding):
    """the answer the torch modules act on (Module.forward) is the library's, whichever binding made the native module"""
    C = _lib()
    for make, want in ((lambda: C.create_network(16, 4, _net(64)), 1), (lambda: C.create_network_with_input_encoding(3, 4, GRID, _net(64)), 0)):
        m = make()
        assert int(m.supports_half_input()) == want == C._lib.tcnn_module_supports_half_input(m._h)


def test_cpp_facade_has_the_half_input_methods(tmp_path):
    src = tmp_path / "caller.cpp"
    src.write_text(r'''
#include <tiny-cuda-nn/config.h>
#include <tiny-cuda-nn/cpp_api.h>
using namespace tcnn;
bool caller(json network, hipStream_t stream, const void* x16, void* y, void* params, void* dx16, const void* dy, void* dparams) {
	cpp::Module* mod = cpp::create_network(20, 4, network);
	auto* hip = static_cast<cpp::HipModule*>(mod);
	const bool ok = hip->supports_half_input();
	hip->inference_half_input(stream, 256, x16, y, params);
	cpp::Context ctx = hip->forward_half_input(stream, 256, x16, y, params, true);
	hip->backward_half_input(stream, ctx, 256, dx16, dy, dparams, x16, y, params);
	delete mod;
	return ok;
}
''')
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

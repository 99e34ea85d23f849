"""Host-side dispatch of tcnn_module_backward_backward_input for modules with a network (csrc/api_module.hip): the fp32 network behind the
plain Identity encoding (tcnn_create_network_precision with TCNN_PRECISION_FP32) has a second-order pass; the 16-bit network, an fp32 network
behind any other encoding and an Identity encoding that scales or shifts keep the reference's refusal (object.h:468).  No GPU, no compute."""
def _lib():
    import tinycudann
    return tinycudann._C


NET = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}
OK, ERROR, UNSUPPORTED = 0, 1, 2


def call(module, n=256, ddx=None):
    lib = _lib()._lib
    rc = lib.tcnn_module_backward_backward_input(module._h, None, None, n, ddx, None, None, None, None, None, None)
    return rc, lib.tcnn_last_error().decode()


def test_the_fp32_network_has_a_second_order_pass():
    C = _lib()
    for cfg in (NET, dict(NET, otype="FullyFusedMLP", activation="ReLU"), dict(NET, activation="Sine", n_neurons=272, n_hidden_layers=1)):
        rc, text = call(C.create_network_precision(32, 4, cfg, C.Precision.Fp32))
        assert rc == ERROR and "missing forward context" in text, (rc, text)


def test_the_16_bit_network_keeps_its_refusal():
    C = _lib()
    for m in (C.create_network(32, 4, NET), C.create_network_precision(32, 4, NET, C.preferred_precision()), C.create_network_with_input_encoding(3, 4, GRID, NET)):
        rc, text = call(m)
        assert rc == UNSUPPORTED and "not implemented" in text, (rc, text)


def test_an_fp32_network_behind_another_encoding_keeps_its_refusal():
    C = _lib()
    composite = {"otype": "Composite", "nested": [{"otype": "Frequency", "n_dims_to_encode": 2, "n_frequencies": 3}, {"otype": "Identity"}]}
    for n_dims, enc in [(3, GRID), (3, {"otype": "Frequency", "n_frequencies": 4}), (2, {"otype": "OneBlob", "n_bins": 8}), (3, composite),
                        (3, {"otype": "Identity", "scale": 2.0}), (3, {"otype": "Identity", "offset": 0.5})]:
        rc, text = call(C.create_network_with_input_encoding_precision(n_dims, 4, enc, NET, C.Precision.Fp32))
        assert rc == UNSUPPORTED and "not implemented" in text, (enc, rc, text)
    # the explicit plain Identity is the module create_network_precision makes
    rc, text = call(C.create_network_with_input_encoding_precision(3, 4, {"otype": "Identity"}, NET, C.Precision.Fp32))
    assert rc == ERROR and "missing forward context" in text


def test_bare_encodings_are_as_they_were():
    C = _lib()
    rc, text = call(C.create_encoding(3, GRID, C.Precision.Fp32))
    assert rc == ERROR and "missing forward context" in text
    rc, text = call(C.create_encoding(3, {"otype": "Frequency", "n_frequencies": 4}, C.Precision.Fp32))
    assert rc == UNSUPPORTED and "not implemented" in text


def test_the_header_says_which_modules_have_the_pass():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tcnn_hip.h")).read()
    assert "as for every network" not in header and"tcnn_create_network_precision(..., TCNN_PRECISION_FP32): the double backward" in header

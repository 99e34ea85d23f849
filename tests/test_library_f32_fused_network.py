"""Host logic of the fused fp32 network kernel's dispatch (csrc/mlp_kernels.h mlp_f32_fused_supported, tcnn_set_fp32_fused_network,
tcnn_module_fp32_fused_network): the switch round-trips and defaults to on, the query names exactly the kernel's shapes and answers 0 with
the switch off, and nothing a module reports about itself changes.  No GPU, no compute calls."""
import pytest

GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}


def _C():
    import tinycudann
    return tinycudann._C


def _net(width, hidden=2):
    return {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}


def _fp32(C, n_in, n_out, width, hidden=2):
    return C.create_network_precision(n_in, n_out, _net(width, hidden), C.Precision.Fp32)


def test_the_switch_round_trips_and_defaults_to_on():
    C = _C()
    assert C.get_fp32_fused_network() is True
    try:
        C.set_fp32_fused_network(False)
        assert C.get_fp32_fused_network() is False
    finally:
        C.set_fp32_fused_network(True)
    assert C.get_fp32_fused_network() is True
    for name in ("tcnn_set_fp32_fused_network", "tcnn_get_fp32_fused_network", "tcnn_module_fp32_fused_network"):
        assert name in C.EXPORTED_SYMBOLS


# (inputs, outputs, neurons, hidden layers): the limits are 128 inputs and 64 padded outputs, any depth
@pytest.mark.parametrize("shape", [(16, 1, 16, 1), (48, 20, 32, 3), (128, 64, 64, 2), (32, 50, 64, 12), (3, 4, 64, 2)])
def test_the_query_says_1_inside_the_limits(shape):
    C = _C()
    m = _fp32(C, *shape)
    before = m.hyperparams()
    assert m.fp32_fused_network(256) == 1 and m.fp32_fused_network(768) == 1 and m.fp32_fused_network(1 << 18) == 1
    assert m.fp32_fused_network(0) == 0 and m.fp32_fused_network(128) == 0  # (not a batch a module accepts: nothing would run)
    try:
        C.set_fp32_fused_network(False)
        assert m.fp32_fused_network(256) == 0 and m.hyperparams() == before and before["network"]["otype"] == "CutlassMLP"
    finally:
        C.set_fp32_fused_network(True)
    assert m.fp32_fused_network(256) == 1


@pytest.mark.parametrize("shape", [(32, 4, 48, 2), (32, 4, 128, 2), (32, 80, 64, 2), (144, 4, 64, 2)], ids=["W48", "W128", "out80", "in144"])
def test_the_query_says_0_outside_the_limits(shape):
    assert _fp32(_C(), *shape).fp32_fused_network(256) == 0


def test_the_query_says_0_for_16_bit_networks_and_bare_encodings():
    C = _C()
    assert C.create_network(32, 4, _net(64)).fp32_fused_network(256) == 0
    assert C.create_encoding(3, GRID, C.Precision.Fp32).fp32_fused_network(256) == 0
    assert C.create_network_with_input_encoding_precision(3, 4, GRID, _net(64), C.Precision.Fp32).fp32_fused_network(256) == 1

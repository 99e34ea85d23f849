"""Host logic of the network factory for widths outside 16/32/64/128 (model_desc.hip create_network_desc, reference src/network.cu:51-141):
"MLP" / "CutlassMLP" build the layer-by-layer network for every other multiple of 16 up to 1024 and report "CutlassMLP"
(networks/cutlass_mlp.h:152); "FullyFusedMLP" keeps refusing them.  No GPU, no compute calls -- that the initial parameters of these
networks are the oracle's Xavier draw bit for bit needs a device buffer and is asserted in tests/test_gpu_general_mlp.py."""
import pytest

from oracle import oracle as O


def _lib():
    import tinycudann
    return tinycudann._C


@pytest.mark.parametrize("cfg,width,hidden", [
    ({"n_neurons": 256, "n_hidden_layers": 2}, 256, 2),                          # `otype` left alone: "MLP" (network.cu:51)
    ({"otype": "CutlassMLP", "n_neurons": 48}, 48, 5),                           # n_hidden_layers defaults to 5
    ({"otype": "MLP", "n_neurons": 1024, "n_hidden_layers": 1}, 1024, 1),        # the widest
])
def test_mlp_and_cutlass_mlp_take_any_multiple_of_16(cfg, width, hidden):
    m = _lib().create_network(3, 4, cfg)  # identity encoding: 3 inputs padded to 16; 4 outputs padded to 16
    assert m.n_params() == width * 16 + (hidden - 1) * width * width + 16 * width
    assert m.n_params() == O.mlp_init(16, width, 4, hidden).n_params
    assert m.n_output_dims() == 16
    hp = m.hyperparams()["network"]  # (a network module is a NetworkWithInputEncoding around an identity encoding)
    assert hp["otype"] == "CutlassMLP" and hp["n_neurons"] == width and hp["n_hidden_layers"] == hidden
    assert hp["activation"] == "ReLU" and hp["output_activation"] == "None"


def test_behind_an_encoding_wider_than_the_fused_kernels_take():
    """32 levels x 8 features: a 256-wide encoded input -- only the layer-by-layer network accepts more than 128 inputs"""
    enc = {"otype": "HashGrid", "n_levels": 32, "n_features_per_level": 8, "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 1.2}
    m = _lib().create_network_with_input_encoding(3, 3, enc, {"n_neurons": 256, "n_hidden_layers": 2})
    assert m.hyperparams()["network"]["otype"] == "CutlassMLP"
    with pytest.raises(RuntimeError, match="at most 128"):
        _lib().create_network_with_input_encoding(3, 3, enc, {"n_neurons": 64, "n_hidden_layers": 2})


@pytest.mark.parametrize("otype", ["MLP", "CutlassMLP", "FullyFusedMLP"])
def test_the_fused_widths_stay_fully_fused(otype):
    m = _lib().create_network(3, 4, {"otype": otype, "n_neurons": 64, "n_hidden_layers": 2})
    assert m.hyperparams()["network"]["otype"] == "FullyFusedMLP"


@pytest.mark.parametrize("cfg,msg", [
    ({"n_neurons": 40}, "must be a multiple of 16, but got 40"),
    ({"otype": "CutlassMLP", "n_neurons": 2048}, "between 16 and 1024 neurons .* but got 2048"),
    ({"otype": "FullyFusedMLP", "n_neurons": 256}, "FullyFusedMLP only supports 16, 32, 64, and 128 neurons, but got 256"),
    ({"otype": "MegakernelMLP", "n_neurons": 48}, "only supports 16, 32, 64, and 128 neurons"),
    ({"n_neurons": 256, "n_hidden_layers": 0}, "CutlassMLP requires at least 1 hidden layer"),  # the reference allows it; the oracle does not
])
def test_refused_configurations_name_the_limit(cfg, msg):
    C = _lib()
    C.set_log_callback(lambda sev, m: None)
    try:
        with pytest.raises(RuntimeError, match=msg):
            C.create_network(3, 4, cfg)
    finally:
        C.set_log_callback(None)

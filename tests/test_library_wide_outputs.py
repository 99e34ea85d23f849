"""Host logic of the network factory for more than 128 (padded) outputs (model_desc.hip create_network_desc, mlp_kernels.h
mlp_layer_by_layer): such a network is a layer-by-layer one at every hidden width and under both spellings of the otype, reports
"CutlassMLP", and has the oracle's parameter count; the limit is 1024 padded outputs (MLP_GENERAL_MAX_OUT_WIDTH), and the message of a
refusal names it.  Networks of at most 128 outputs stay what they were.  No GPU, no compute calls."""
import pytest

from conftest import ADAM_HASH, HASH_ENCODING_SMALL
from oracle import oracle as O


def _lib():
    import tinycudann
    return tinycudann._C


FUSED_WIDTHS = (16, 32, 64, 128)
CASES = [(w, out, otype) for w, out in ((16, 129), (64, 256), (128, 1000), (256, 1024)) for otype in ("FullyFusedMLP", "MLP") if otype == "MLP" or w in FUSED_WIDTHS]


@pytest.mark.parametrize("width,n_output_dims,otype", CASES)
def test_wide_outputs_build_the_layer_by_layer_network(width, n_output_dims, otype):
    m = _lib().create_network(3, n_output_dims, {"otype": otype, "n_neurons": width, "n_hidden_layers": 2})  # identity encoding: 3 inputs padded to 16
    padded = (n_output_dims + 15) // 16 * 16
    assert m.n_params() == O.mlp_init(16, width, n_output_dims, 2).n_params == width * 16 + width * width + padded * width
    assert m.n_output_dims() == padded
    hp = m.hyperparams()["network"]
    assert hp["otype"] == "CutlassMLP" and hp["n_neurons"] == width and hp["n_hidden_layers"] == 2


@pytest.mark.parametrize("otype", ["FullyFusedMLP", "MLP"])
def test_128_outputs_at_a_fused_width_stay_fully_fused(otype):
    m = _lib().create_network(3, 128, {"otype": otype, "n_neurons": 64, "n_hidden_layers": 2})
    assert m.n_output_dims() == 128
    assert m.hyperparams()["network"]["otype"] == "FullyFusedMLP"


@pytest.mark.parametrize("cfg", [{"otype": "MLP", "n_neurons": 256}, {"otype": "FullyFusedMLP", "n_neurons": 64}, {"otype": "CutlassMLP", "n_neurons": 16}])
def test_more_than_1024_outputs_are_refused_and_the_message_names_the_limit(cfg):
    C = _lib()
    C.set_log_callback(lambda sev, m: None)
    try:
        with pytest.raises(RuntimeError, match="more than 1024 output dimensions"):
            C.create_network(3, 1025, cfg)
    finally:
        C.set_log_callback(None)


def test_create_from_config_with_144_outputs():
    """tcnn_create_from_config builds the model description (where the width is accepted or refused) and then allocates the parameters on the
    device.  With a device the call succeeds; without one it must get as far as that allocation: the only error allowed is the HIP
    runtime's about the missing device, never the factory's about the configuration."""
    import tinycudann
    cfg = {"loss": {"otype": "RelativeL2"}, "optimizer": dict(ADAM_HASH), "encoding": dict(HASH_ENCODING_SMALL),
           "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}}
    C = _lib()
    C.set_log_callback(lambda sev, m: None)
    try:
        tm = tinycudann.create_from_config(3, 144, cfg, seed=1337)
    except RuntimeError as e:
        assert "output dimensions" not in str(e) and "MLP" not in str(e), e
        assert "hipMalloc failed" in str(e) or "no ROCm-capable device" in str(e), e
    else:
        assert tm.n_output_dims == 144 and tm.padded_output_width == 144
    finally:
        C.set_log_callback(None)

"""Host logic of the fp32 networks (tcnn_create_network_precision / tcnn_create_network_with_input_encoding_precision with
TCNN_PRECISION_FP32; csrc/model_desc.hip, api_module.hip): every `otype` spelling makes the fp32 layer-by-layer network and reports
"CutlassMLP", the precisions are fp32, the parameter layout is the 16-bit network's, the refusals carry the 16-bit network's texts, and the
library's own precision through the new creators is the old creators' module.  No GPU, no compute calls -- except the last test, which needs
a device buffer for the initial parameters and is marked `gpu`."""
import ctypes

import numpy as np
import pytest


def _lib():
    import tinycudann
    return tinycudann._C


GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}


def _net(otype, width, **more):
    return dict({"otype": otype, "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": 2}, **more)


@pytest.mark.parametrize("width", [16, 64, 48, 272])
@pytest.mark.parametrize("otype", ["FullyFusedMLP", "MLP", "CutlassMLP"])
def test_every_spelling_makes_an_fp32_cutlass_mlp(otype, width):
    C = _lib()
    m = C.create_network_precision(32, 5, _net(otype, width), C.Precision.Fp32)
    hp = m.hyperparams()
    assert hp["otype"] == "NetworkWithInputEncoding" and hp["encoding"]["otype"] == "Identity"
    assert hp["network"] == {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": 2}
    assert m.param_precision() == C.Precision.Fp32 and m.output_precision() == C.Precision.Fp32
    assert C.default_loss_scale(m.param_precision()) == 1.0
    assert m.n_input_dims() == 32 and m.n_output_dims() == 16
    assert m.n_params() == width * 32 + width * width + 16 * width
    assert not m.supports_half_input()
    if not (otype == "FullyFusedMLP" and width in (48, 272)):  # (which the 16-bit FullyFusedMLP refuses)
        assert m.n_params() == C.create_network(32, 5, _net(otype, width)).n_params()


def test_behind_every_kind_of_encoding():
    C = _lib()
    composite = {"otype": "Composite", "nested": [{"otype": "HashGrid", "n_dims_to_encode": 3, "n_levels": 2, "n_features_per_level": 2, "log2_hashmap_size": 8,
                                                   "base_resolution": 4}, {"otype": "Frequency", "n_dims_to_encode": 1, "n_frequencies": 3}, {"otype": "Identity"}]}
    for n_dims, enc in [(3, GRID), (3, {"otype": "Frequency", "n_frequencies": 4}), (2, {"otype": "OneBlob", "n_bins": 8}), (3, {"otype": "TriangleWave", "n_frequencies": 4}),
                        (5, composite)]:
        m = C.create_network_with_input_encoding_precision(n_dims, 3, enc, _net("FullyFusedMLP", 48), C.Precision.Fp32)
        old = C.create_network_with_input_encoding(n_dims, 3, enc, _net("CutlassMLP", 48))
        assert m.n_params() == old.n_params() and m.n_output_dims() == old.n_output_dims() == 16
        assert m.hyperparams()["encoding"] == old.hyperparams()["encoding"] and m.hyperparams()["network"]["otype"] == "CutlassMLP"
        assert m.param_precision() == C.Precision.Fp32 and not m.supports_half_input()


def test_max_level_of_a_lone_grid_and_its_refusal():
    C = _lib()
    m = C.create_network_with_input_encoding_precision(3, 3, GRID, _net("MLP", 64), C.Precision.Fp32)
    assert m.max_level() == 1.0
    m.set_max_level(0.5)
    assert m.max_level() == 0.5
    plain = C.create_network_precision(3, 3, _net("MLP", 64), C.Precision.Fp32)
    with pytest.raises(RuntimeError, match="set_max_level: IdentityEncoding is not a multi-level grid encoding"):
        plain.set_max_level(0.5)


@pytest.mark.parametrize("cfg,n_out,msg", [
    (_net("CutlassMLP", 64, output_activation="Sine"), 4, "Activation 'Sine' is not supported as output_activation"),
    (_net("FullyFusedMLP", 24), 4, "CutlassMLP: the number of neurons must be a multiple of 16, but got 24"),
    (_net("MLP", 2048), 4, "between 16 and 1024 neurons .* but got 2048"),
    (_net("MLP", 64), 1040, "CutlassMLP: more than 1024 output dimensions are not supported by this build"),
    (_net("MLP", 48, n_hidden_layers=0), 4, "CutlassMLP requires at least 1 hidden layer"),
    (_net("NoSuchMLP", 64), 4, "Invalid network type: NoSuchMLP"),
])
def test_refusals_carry_the_16_bit_networks_texts(cfg, n_out, msg):
    C = _lib()
    C.set_log_callback(lambda sev, m: None)
    try:
        with pytest.raises(RuntimeError, match=msg):
            C.create_network_precision(32, n_out, cfg, C.Precision.Fp32)
        if cfg["otype"] != "FullyFusedMLP":  # the same text from the 16-bit network of that spelling
            with pytest.raises(RuntimeError, match=msg):
                C.create_network(32, n_out, cfg)
    finally:
        C.set_log_callback(None)


def test_sine_and_silu_hidden_activations_under_every_spelling():
    C = _lib()
    for act in ("Sine", "SiLU"):
        for otype in ("FullyFusedMLP", "CutlassMLP"):
            m = C.create_network_precision(16, 1, _net(otype, 64, activation=act), C.Precision.Fp32)
            assert m.hyperparams()["network"]["activation"] == act and m.hyperparams()["network"]["otype"] == "CutlassMLP"


def test_the_trainer_stays_16_bit():
    C = _lib()
    cfg = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam"}, "encoding": {"otype": "Identity"}, "network": _net("MLP", 64)}
    h = ctypes.c_void_p()
    code = C._lib.tcnn_create_from_config_precision(16, 4, C._dumps(cfg), 1, int(C.Precision.Fp32), ctypes.byref(h))
    assert code == 2 and not h.value  # TCNN_ERROR_UNSUPPORTED
    text = C._lib.tcnn_last_error().decode()
    assert "trainer" in text and "tcnn_create_from_config" in text and "training_step" in text and "data-parallel" in text and "16-bit only" in text


def test_data_parallel_refuses_an_fp32_module():
    import tinycudann.parallel as P
    C = _lib()
    m = C.create_network_precision(16, 4, _net("MLP", 64), C.Precision.Fp32)
    with pytest.raises(RuntimeError, match="data-parallel entry points take a trainable model .* an fp32 module is not supported"):
        P.DataParallel(m)


def test_an_unknown_precision_is_refused():
    C = _lib()
    other = C.Precision.Bf16 if C.preferred_precision() == C.Precision.Fp16 else C.Precision.Fp16
    with pytest.raises(RuntimeError, match="create_network: this build .*provides (fp16|bf16) and fp32 networks"):
        C.create_network_precision(16, 4, _net("MLP", 64), other)


@pytest.mark.parametrize("otype,width", [("FullyFusedMLP", 64), ("MLP", 64), ("CutlassMLP", 48), ("MLP", 272)])
def test_the_librarys_own_precision_is_the_old_creators_module(otype, width):
    C = _lib()
    for new, old in [(C.create_network_precision(32, 5, _net(otype, width), C.preferred_precision()), C.create_network(32, 5, _net(otype, width))),
                     (C.create_network_precision(32, 5, _net(otype, width)), C.create_network(32, 5, _net(otype, width))),
                     (C.create_network_with_input_encoding_precision(3, 5, GRID, _net(otype, width), C.preferred_precision()),
                      C.create_network_with_input_encoding(3, 5, GRID, _net(otype, width)))]:
        assert new.hyperparams() == old.hyperparams() and new.n_params() == old.n_params() and new.name() == old.name()
        assert new.param_precision() == old.param_precision() == C.preferred_precision() and new.output_precision() == old.output_precision()
        assert new.supports_half_input() == old.supports_half_input()


def test_the_header_declares_the_new_entry_points():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tcnn_hip.h")).read()
    for name in ("tcnn_create_network_precision", "tcnn_create_network_with_input_encoding_precision", "tcnn_create_from_config_precision",
                 "tcnn_module_inference_matrix", "tcnn_module_backward_gradient_mode"):
        assert name + "(" in header and name in _lib().EXPORTED_SYMBOLS


def test_modules_reject_other_dtypes():
    import torch
    import tinycudann as tcnn
    with pytest.raises(ValueError, match="only supports fp32, fp16 or bf16 precision"):
        tcnn.Network(16, 4, _net("MLP", 64), dtype=torch.float64)
    with pytest.raises(ValueError, match="only supports fp32, fp16 or bf16 precision"):
        tcnn.NetworkWithInputEncoding(3, 4, GRID, _net("MLP", 64), dtype=torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [False, True], ids=["bare", "hashgrid"])
@pytest.mark.parametrize("act", ["ReLU", "Sine"])
def test_initial_params_are_what_the_16_bit_network_rounds_its_own_from(act, grid):
    """initialize_params writes to device memory, so this one needs a GPU: the fp32 network's initial parameters, rounded to the library's
    16-bit type, are the 16-bit network's (Xavier; SIREN for Sine), and before rounding they are the same fp32 numbers"""
    import torch
    C = _lib()
    net = _net("CutlassMLP", 48, activation=act)
    if grid:
        m32, m16 = C.create_network_with_input_encoding_precision(3, 3, GRID, net, C.Precision.Fp32), C.create_network_with_input_encoding(3, 3, GRID, net)
    else:
        m32, m16 = C.create_network_precision(16, 3, net, C.Precision.Fp32), C.create_network(16, 3, net)
    half = C.TORCH_DTYPE[C.preferred_precision()]
    p32, p16 = m32.initial_params(1337), m16.initial_params(1337)
    assert p32.dtype == torch.float32 and p32.shape == p16.shape == (m16.n_params(),)
    assert np.array_equal(p32.to(half).cpu().view(torch.int16).numpy(), p16.to(half).cpu().view(torch.int16).numpy())
    assert np.array_equal(p32.cpu().numpy().view(np.uint32), p16.cpu().numpy().view(np.uint32))
    assert float(p32.abs().max()) > 0

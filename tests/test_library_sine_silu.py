"""Host logic for the Sine and SiLU hidden activations (model_desc.hip create_network_desc; reference src/network.cu:51-141,
src/cutlass_mlp.cu): accepted as the hidden activation of "MLP" / "CutlassMLP" networks of EVERY width -- 16/32/64/128 included, which
then run layer by layer and report "CutlassMLP" -- refused by FullyFusedMLP and as output activations.  No GPU, no compute calls.

The second half pins the numpy restatement the emulator and GPU tests compare with (tests/sine_silu_reference.py) against an
independent derivation, and checks the shared cases' accumulation band."""
import numpy as np
import pytest

import sine_silu_reference as S
from oracle import oracle as O


def _lib():
    import tinycudann
    return tinycudann._C


@pytest.mark.parametrize("activation", ["Sine", "SiLU"])
@pytest.mark.parametrize("otype", ["MLP", "CutlassMLP", None])
@pytest.mark.parametrize("width", [48, 64, 128, 256])
def test_accepted_on_every_width_and_reported_as_cutlass_mlp(width, otype, activation):
    cfg = {"activation": activation, "n_neurons": width, "n_hidden_layers": 2}
    if otype:
        cfg["otype"] = otype
    m = _lib().create_network(3, 4, cfg)  # identity encoding: 3 inputs padded to 16; 4 outputs padded to 16
    assert m.n_params() == width * 16 + width * width + 16 * width == S.n_params(16, width, 4, 2)
    assert m.n_output_dims() == 16
    hp = m.hyperparams()["network"]
    assert hp["otype"] == "CutlassMLP" and hp["activation"] == activation and hp["output_activation"] == "None"
    assert hp["n_neurons"] == width and hp["n_hidden_layers"] == 2


def test_activation_names_are_case_insensitive_like_the_others():
    hp = _lib().create_network(3, 4, {"activation": "sine", "n_neurons": 64, "n_hidden_layers": 1}).hyperparams()["network"]
    assert hp["activation"] == "Sine" and hp["otype"] == "CutlassMLP"


def test_input_width_limit_is_the_layer_by_layer_one():
    """32 levels x 8 features = 256 encoded inputs: more than the fused kernels take, fine for a 64-wide Sine network"""
    enc = {"otype": "HashGrid", "n_levels": 32, "n_features_per_level": 8, "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 1.2}
    m = _lib().create_network_with_input_encoding(3, 3, enc, {"activation": "Sine", "n_neurons": 64, "n_hidden_layers": 2})
    assert m.hyperparams()["network"]["otype"] == "CutlassMLP"


@pytest.mark.parametrize("cfg,msg", [
    ({"otype": "FullyFusedMLP", "activation": "Sine", "n_neurons": 64}, "Activation 'Sine' is not supported by FullyFusedMLP \\(it needs stored pre-activations\\).*use CutlassMLP"),
    ({"otype": "MegakernelMLP", "activation": "SiLU", "n_neurons": 128}, "Activation 'SiLU' is not supported by FullyFusedMLP .*use CutlassMLP"),
    ({"output_activation": "Sine", "n_neurons": 64}, "'Sine'.*output activations must be expressible from the output value"),
    ({"otype": "CutlassMLP", "output_activation": "SiLU", "n_neurons": 256}, "'SiLU'.*output activations must be expressible from the output value"),
    ({"activation": "Sine", "n_neurons": 40}, "must be a multiple of 16, but got 40"),
])
def test_refused_configurations_say_why(cfg, msg):
    C = _lib()
    C.set_log_callback(lambda sev, m: None)
    try:
        with pytest.raises(RuntimeError, match=msg):
            C.create_network(3, 4, cfg)
    finally:
        C.set_log_callback(None)


@pytest.mark.parametrize("activation", ["ReLU", "Tanh"])
def test_the_other_activations_stay_on_the_fused_kernels(activation):
    m = _lib().create_network(3, 4, {"otype": "CutlassMLP", "activation": activation, "n_neurons": 64, "n_hidden_layers": 2})
    assert m.hyperparams()["network"]["otype"] == "FullyFusedMLP"


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
def test_siren_draw_has_the_two_scales_and_leaves_the_stream_where_xavier_does():
    IN, W, OUT, H = 32, 64, 4, 2
    rng = O.pcg32(1337)
    p = S.siren_init_params(IN, W, OUT, H, rng)
    first, hidden, out = S.split(p, IN, W, OUT, H)
    assert np.abs(first).max() <= 30.0 / IN and np.abs(first).max() > 0.95 * 30.0 / IN
    for m in (hidden, out):
        assert np.abs(m).max() <= np.sqrt(6.0 / W) and np.abs(m).max() > 0.95 * np.sqrt(6.0 / W)
    # same number of draws as Xavier: what follows in the stream (the encoding's parameters) is unchanged
    rng_x = O.pcg32(1337)
    O.mlp_init_params(O.mlp_init(IN, W, OUT, H), rng_x)
    assert (rng.state, rng.inc) == (rng_x.state, rng_x.inc)
    # the same uniform numbers under both: (w + s) / (2 s) is the draw
    x = O.mlp_init_params(O.mlp_init(IN, W, OUT, H), O.pcg32(1337))
    sx, ss = np.sqrt(6.0 / (W + IN)), 30.0 / IN
    assert np.allclose((x[:W * IN] + sx) / (2 * sx), (p[:W * IN] + ss) / (2 * ss), atol=1e-6)


def _torch_network(act, shape, ph, x_h, dy_h):
    """float64 torch network on the 16-bit-rounded weights, autograd; no intermediate rounding anywhere"""
    import torch
    IN, W, OUT, H = shape
    mats = [torch.tensor(O.h2f(m).astype(np.float64), requires_grad=True) for m in S.split(ph, IN, W, OUT, H)]
    x = torch.tensor(O.h2f(x_h).astype(np.float64), requires_grad=True)
    a = x
    for Wl in mats[:-1]:
        pre = a @ Wl.T
        a = torch.sin(pre) if act == S.ACT_SINE else torch.nn.functional.silu(pre)
    out = a @ mats[-1].T
    out.backward(torch.tensor(O.h2f(dy_h).astype(np.float64)))
    return out.detach().numpy(), np.concatenate([m.grad.numpy().reshape(-1) for m in mats]), x.grad.numpy()


@pytest.mark.parametrize("act", [S.ACT_SINE, S.ACT_SILU], ids=["Sine", "SiLU"])
def test_restatement_against_an_independent_float64_network(act):
    """The restatement (float64 accumulation mode) against torch float64 with autograd on the same fp16-rounded weights, by relative L2.
    What separates the two is the restatement's fp16 rounding of every stored matrix -- pure rounding noise, not derivable in advance:
    measured on the middle case (32, 64, 4, 2, 256):
        Sine: output 5.44e-4, weight gradients 5.45e-4, dL/dinput 7.62e-4;  SiLU: output 5.22e-4, weight gradients 3.61e-4, dL/dinput 5.40e-4.
    Bar: 4 x the largest of them, 4 x 7.62e-4 = 3.05e-3, for all six."""
    c = S.case(act, S.CASES[1])
    out, g, dx = _torch_network(act, c.shape, c.ph, c.x, c.dy)
    rel = lambda a, b: np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)  # noqa: E731
    figures = rel(O.h2f(c.out_ref), out), rel(c.g_ref, g), rel(O.h2f(c.dx_ref), dx)
    print(S.NAMES[act], "relative L2: output %.3g, weight gradients %.3g, dL/dinput %.3g" % figures)
    assert max(figures) < 3.05e-3


@pytest.mark.parametrize("act", [S.ACT_SINE, S.ACT_SILU], ids=["Sine", "SiLU"])
@pytest.mark.parametrize("shape", S.CASES, ids=[str(c) for c in S.CASES])
def test_accumulation_band_of_the_shared_cases_is_within_half_of_every_bar(act, shape):
    """fp32-in-k-order against float64 accumulation on the inputs the emulator and GPU tests use, compared as those tests compare (layer by
    layer on shared stacks): at most half of each of their bars.  The bfloat16 case asserts the same in tests/test_emu_sine_silu.py, where
    the 16-bit format is switched.  The cases did not have to be changed for this; what had to change was comparing two sides that each
    run their own chain, which at (80, 272, 40, 3, 768) is past the bars between the two modes themselves (sine_silu_reference.py has
    the figures)."""
    S.band(S.case(act, shape), S.BARS_FP16)

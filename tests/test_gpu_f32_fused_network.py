"""The fused fp32 network kernel (csrc/mlp_f32_fused.hip: inference, inference into the caller's matrix, the forward pass that saves
activations) on a real MI355X against the numpy float64 MLP of tests/test_gpu_f32_network.py on the same float32 weights and inputs.

The bar is tests/test_gpu_f32_network.py's rule and its FACTOR, unchanged: per compared quantity, the max error of a numpy float32
restatement against float64 on the same inputs, times FACTOR.  Every case prints the GPU error, the CPU float32 error and the bar (-s).
Inputs U(-1, 1), Xavier weights, dL/doutput U(-1, 1) from a fixed seed; where gradients are compared through ReLU / LeakyReLU the seed is
advanced until no float64 pre-activation lies within 2e-6 of zero, as there.  Every case also runs with tcnn_set_fp32_fused_network(0),
where the query answers 0 and the layer-by-layer kernels are held to the same bar: the test compares two paths.

The exact case restates the recipe of tests/exact_f32_network_cases.py for one network: inputs and dL/doutput in {-1, 0, 1}, weights small
integers over 4 (input and output matrix) or 2 (hidden matrix), ReLU -- every product and partial sum of every pass is an fp32 number in any
order (largest sum of |terms| over the common power of two, measured on these data: 2^12.8, far below 2^24), so both paths must agree in
every bit; a dropped tile, a wrong lane or a permuted neuron cannot hide under a bar."""
import numpy as np
import pytest
import torch

import second_order_mlp_reference as R
from test_gpu_f32_network import FACTOR, GRID, HIDDEN, mlp  # (its bar, and its numpy network: forward and backward in a given dtype)

pytestmark = pytest.mark.gpu


def C():
    import tinycudann
    return tinycudann._C


_cache = {}


def case(IN, W, H, OUT, n, hidden_act="ReLU", output_act="None", given_x=None, away_from_kinks=False):
    """inputs, the float64 reference and the bars (FACTOR x the CPU float32 errors), computed once and shared"""
    key = (IN, W, H, OUT, n, hidden_act, output_act, away_from_kinks, given_x is not None)
    seed = 5150 + IN + 3 * W + 7 * H
    while key not in _cache:
        rng = np.random.default_rng(seed)
        OUTP = (OUT + 15) // 16 * 16
        mats = [rng.uniform(-1, 1, size=(r, c)).astype(np.float32) * np.float32(np.sqrt(6.0 / (r + c))) for r, c in [(W, IN)] + [(W, W)] * (H - 1) + [(OUTP, W)]]
        mats[-1][OUT:] = 0  # the padded output rows
        x = rng.uniform(-1, 1, size=(n, IN)).astype(np.float32) if given_x is None else given_x
        dy = np.zeros((n, OUTP), np.float32)
        dy[:, :OUT] = rng.uniform(-1, 1, size=(n, OUT))
        ref = mlp(np.float64, mats, x, dy, hidden_act, output_act)
        if away_from_kinks and hidden_act in ("ReLU", "LeakyReLU") and min(float(np.abs(p).min()) for p in ref[3]) <= 2e-6:
            seed += 1000
            continue
        f32 = mlp(np.float32, mats, x, dy, hidden_act, output_act)
        _cache[key] = (mats, x, dy, ref[:3], [FACTOR * float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(f32[:3], ref[:3])])
    return _cache[key]


def network(W, H, hidden_act="ReLU", output_act="None"):
    return {"otype": "CutlassMLP", "activation": hidden_act, "output_activation": output_act, "n_neurons": W, "n_hidden_layers": H}


def held(name, got, ref, bar):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    print(f"{name}: GPU max error {err:.3e}, CPU float32 {bar / FACTOR:.3e}, bar {bar:.3e}, max |reference| {np.abs(ref).max():.3e}")
    assert np.isfinite(got).all() and err <= bar, f"{name}: GPU max error {err:.3e} exceeds the bar {bar:.3e}"


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def run(m, data, n, backward):
    """inference, forward (bit-equal to it) and, if asked, backward of `m` under both settings of the switch, each held to the bars;
    -> per setting (prediction, dL/dinput, parameter gradients, context and tensors for a second-order call)"""
    mats, x, dy, ref, bars = data
    flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda()
    results = {}
    for fused in (True, False):
        C().set_fp32_fused_network(fused)
        try:
            assert m.fp32_fused_network(n) == int(fused)
            xt = torch.from_numpy(x).cuda()
            pt = flat
            _, y_inference = m.fwd(xt, pt)
            xt, pt = xt.clone().requires_grad_(True), pt.clone().requires_grad_(True)
            ctx, y = m.fwd(xt, pt)
            tag = "fused" if fused else "layer by layer"
            held(f"{tag} inference", y_inference, ref[0], bars[0])
            held(f"{tag} forward", y, ref[0], bars[0])
            assert np.array_equal(bits(y), bits(y_inference))
            dx = dp = None
            if backward:
                dx, dp = m.bwd(ctx, xt, pt, y, torch.from_numpy(dy).cuda())
                held(f"{tag} dL/dinput", dx, ref[1], bars[1])
                held(f"{tag} parameter gradients", dp, ref[2], bars[2])
            results[fused] = (y, dx, dp, ctx, xt, pt)
        finally:
            C().set_fp32_fused_network(True)
    return results


# (inputs, hidden layers, outputs): padded outputs 16 / 32 / 64; input k-loops longer and shorter than the width; the register hand-over twice
SHAPES = [(16, 1, 5), (48, 3, 20), (128, 2, 50)]


@pytest.mark.parametrize("n", [256, 768])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-x%d-%d" % s)
@pytest.mark.parametrize("W", [16, 32, 64])
def test_widths_depths_and_batches(W, shape, n):
    IN, H, OUT = shape
    run(C().create_network_precision(IN, OUT, network(W, H), C().Precision.Fp32), case(IN, W, H, OUT, n), n, backward=False)


def test_a_network_too_deep_for_resident_weights():
    """12 hidden layers of 64 neurons: over 200 KiB of weights, staged through LDS one matrix at a time"""
    run(C().create_network_precision(32, 4, network(64, 12), C().Precision.Fp32), case(32, 64, 12, 4, 256), 256, backward=False)


@pytest.mark.parametrize("output_act", ["None", "Sigmoid"])
@pytest.mark.parametrize("hidden_act", HIDDEN)
def test_activations(hidden_act, output_act):
    """(SiLU / Sine: backward reads the pre-activations the fused forward pass saved behind the post-activations)"""
    m = C().create_network_precision(32, 4, network(32, 2, hidden_act, output_act), C().Precision.Fp32)
    run(m, case(32, 32, 2, 4, 256, hidden_act, output_act, away_from_kinks=True), 256, backward=True)


@pytest.mark.parametrize("hidden_act", ["ReLU", "Softplus", "Sine"])
def test_saved_activations_are_what_backward_reads(hidden_act):
    n = 768
    data = case(32, 64, 2, 4, n, hidden_act, away_from_kinks=True)
    m = C().create_network_precision(32, 4, network(64, 2, hidden_act), C().Precision.Fp32)
    results = run(m, data, n, backward=True)
    if hidden_act != "Softplus":
        return
    # the second-order pass on the fused forward pass's context, under tests/test_gpu_mlp_second_order.py's rule
    mats, x, dy = data[:3]
    v = np.random.default_rng(99).uniform(-1, 1, size=x.shape).astype(np.float32)
    ref, cpu_error = R.errors(mats, x, dy, v, hidden_act, "None")
    _, _, _, ctx, xt, pt = results[True]
    ddy, dp, dx = m.bwd_bwd_input(ctx, xt, pt, torch.from_numpy(v).cuda(), torch.from_numpy(dy).cuda().requires_grad_(True))
    for name, g, r, e in zip(("dL/d(dL/doutput)", "second-order dL/dinput", "second-order parameter gradients"), (ddy, dx, dp), ref, cpu_error):
        held(name, g, r, FACTOR * e)


def test_exact_case_agrees_in_every_bit():
    IN, W, OUTP, n = 32, 64, 16, 256
    rng = np.random.default_rng(64)
    mats = [rng.integers(-2, 3, size=(W, IN)) / 4.0, rng.integers(-1, 2, size=(W, W)) / 2.0, rng.integers(-2, 3, size=(OUTP, W)) / 4.0]
    x, dy = rng.integers(-1, 2, size=(n, IN)).astype(np.float32), rng.integers(-1, 2, size=(n, OUTP)).astype(np.float32)
    mats = [a.astype(np.float32) for a in mats]
    ref = mlp(np.float64, mats, x, dy, "ReLU", "None")[:3]
    assert all(np.array_equal(r.astype(np.float32).astype(np.float64), r) for r in ref)  # (every result is an fp32 number)
    m = C().create_network_precision(IN, OUTP, network(W, 2), C().Precision.Fp32)
    results = run(m, (mats, x, dy, ref, [0.0, 0.0, 0.0]), n, backward=True)  # bar 0: both paths equal float64, hence each other
    for fused_result, plain_result in zip(results[True][:3], results[False][:3]):
        assert np.array_equal(bits(fused_result), bits(plain_result))


@pytest.mark.parametrize("layout", ["sample rows, stride 24", "sample rows, stride 23", "output rows, stride n + 8"])
def test_trimmed_inference_writes_the_trimmed_block_only(layout):
    IN, W, H, OUT, n = 32, 32, 2, 20, 256
    mats, x = case(IN, W, H, OUT, n)[:2]
    m = C().create_network_precision(IN, OUT, network(W, H), C().Precision.Fp32)
    xt, pt = torch.from_numpy(x).cuda(), torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda()
    assert m.fp32_fused_network(n) == 1
    _, padded = m.fwd(xt, pt)
    sentinel = -12345.0
    buffer = torch.full((n, 24) if "24" in layout else (n, 23) if "23" in layout else (OUT + 3, n + 8), sentinel, device="cuda")
    block = buffer[:, :OUT] if layout.startswith("sample") else buffer[:OUT, :n]
    m.inference_into(xt, pt, block)
    torch.cuda.synchronize()
    want = padded[:, :OUT] if layout.startswith("sample") else padded[:, :OUT].T
    assert np.array_equal(bits(block.contiguous()), bits(want.contiguous()))
    block.fill_(sentinel)  # (what the call was allowed to write)
    assert bool((buffer == sentinel).all())


def test_behind_an_fp32_grid():
    n = 256
    rng = np.random.default_rng(77)
    pos = torch.from_numpy(rng.uniform(0, 1, size=(n, 3)).astype(np.float32)).cuda()
    enc = C().create_encoding(3, GRID, C().Precision.Fp32)
    table = torch.from_numpy(rng.uniform(-1, 1, size=enc.n_params()).astype(np.float32)).cuda()
    feat = np.zeros((n, 16), np.float32)
    feat[:, :8] = enc.fwd(pos, table)[1].cpu().numpy()
    mats, _, _, ref, bars = case(16, 64, 2, 4, n, given_x=feat)
    m = C().create_network_with_input_encoding_precision(3, 4, GRID, network(64, 2), C().Precision.Fp32)
    assert m.fp32_fused_network(n) == 1
    _, y = m.fwd(pos, torch.cat([torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda(), table]))
    held("behind a HashGrid: prediction", y, ref[0], bars[0])

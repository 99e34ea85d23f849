"""Composite and TriangleWave encodings on the GPU, in the build the process loaded (fp16; the last test runs this file again in a process
with TCNN_PRECISION=bf16, the pattern of tests/test_gpu_bf16.py).  The reference is composed in tests/composite_reference.py: the oracle's
per-encoding functions on sliced inputs, laid out by the reference's width rules, plus a numpy-fp32 restatement of the triangle wave and
of the reductions.  Batches are 512 and 768 (two and three granules of 256).

Bars -- every one is an existing test's:
  * TriangleWave, OneBlob, Identity, grid features: bit for bit; Frequency: test_gpu_parity.py::test_frequency_encoding's (device vs host
    sinf: < 0.2 % of the outputs differ, by at most 2^-10; bf16: two ulps below 1 = 2^-7);
  * dL_dinput: TriangleWave bit for bit in fp32 (the restatement sums in the kernel's order); OneBlob allclose 1e-5, Frequency 1e-4,
    grid rtol 1e-4 / atol 1e-3 max (test_oneblob_encoding, test_frequency_encoding, test_grid_backward_and_input_gradient);
  * grid parameter gradients: |got - ref| <= 2^-8 sum|terms| + 2e-3 (test_grid_backward_and_input_gradient, the default mode); bf16:
    max |got - ref| <= 2^-6 max |ref| (bf16_cases.py::test_grid_forward_bit_exact_and_backward);
  * network: loss 2e-3, prediction RAE p99 < 3e-3, weight gradients RAE p99 < 5e-3, dL_dinput relative L2 < 2e-2
    (test_gpu_parity_full.py::check_grads and its dx comparison); bf16: 2e-2 / 3e-2 / 5e-2 / 2e-2 (bf16_cases.py).  The p99 bars leave
    out 1 % of the elements."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import composite_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = os.environ.get("TCNN_PRECISION") == "bf16"
HALF = torch.bfloat16 if BF16 else torch.half
SIZES = [512, 768]
NRC = {"otype": "NRC"}
GRID = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 4, "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 2.0}
MIXED = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "Identity"}, dict(GRID, n_dims_to_encode=3),
                                          {"n_dims_to_encode": 2, "otype": "TriangleWave", "n_frequencies": 2}]}
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
FREQ_ULPS = 2.0 ** -7 if BF16 else 2.0 ** -10


@pytest.fixture(autouse=True, scope="module")
def _oracle_half_format():
    O.set_half_format(BF16)
    yield
    O.set_half_format(False)


def tcnn():
    import tinycudann
    return tinycudann


def h_np(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def h_t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(HALF).cuda()


def rae(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (0.5 * (np.abs(a) + np.abs(b)) + np.abs(b).mean() * 1e-2 + 1e-12)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dy_half(shape, seed):
    return O.f2h(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def oracle_grid(enc, d):
    return O.grid_init(d, enc["n_levels"], enc["n_features_per_level"], enc["log2_hashmap_size"], enc["base_resolution"], enc["per_level_scale"])


def mixed_parts(og, alignment=1):
    last = 4 + (-16 % alignment)
    return [dict(kind="Identity", begin=0, dims=3, row=0, padded=4), dict(kind="Grid", begin=3, dims=3, row=4, padded=8, grid=og, params_offset=0),
            dict(kind="TriangleWave", begin=6, dims=2, row=12, padded=last, n_frequencies=2)]


def check_grid_gradient(got, og, pos, dy):
    ref = O.grid_backward(og, pos, dy)
    if BF16:
        assert np.abs(got - ref).max() <= 2.0 ** -6 * np.abs(ref).max()
    else:
        absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))))
        assert np.all(np.abs(got - ref) <= absacc * 2.0 ** -8 + 2e-3)
    assert np.abs(ref).max() > 0


def test_the_library_of_this_process():
    T = tcnn()
    assert T._C.library_path().endswith("libtcnn_hip_bf16.so" if BF16 else "libtcnn_hip.so")


@pytest.mark.parametrize("n", SIZES)
def test_triangle_wave_alone(n):
    """D = 3, 12 frequencies: width 36, 48 behind alignment 16 (padding 1); 16-bit and fp32; inputs on the kinks"""
    C = tcnn()._C
    x_np = R.kink_inputs(n, 3, seed=n)
    for precision, fp32 in ((None, False), (C.Precision.Fp32, True)):
        m = C.create_encoding(3, {"otype": "TriangleWave"}, *([precision] if precision is not None else []))
        assert m.n_output_dims() == 36 and m.n_params() == 0
        x = torch.from_numpy(x_np).cuda().requires_grad_(True)
        p = torch.zeros(0, dtype=torch.float32 if fp32 else HALF, device="cuda")
        ctx, y = m.fwd(x, p)
        want = R.triangle_wave_forward(x_np, 12, fp32=fp32)
        got = y.cpu().numpy() if fp32 else h_np(y)
        assert np.array_equal(got, want)
        dy = dy_half((n, 36), 1)
        dy = (O.h2f(dy) * np.float32(1.37)).astype(np.float32) if fp32 else dy
        dx, _ = m.bwd(ctx, x, p, y, torch.from_numpy(dy).cuda() if fp32 else h_t(dy))
        assert np.array_equal(bits(dx.cpu().numpy()), bits(R.triangle_wave_backward(x_np, 12, dy)))
    # behind a network's alignment of 16 the encoded matrix is 48 wide and rows 36.. are 1: the network's output says so
    net = C.create_network_with_input_encoding(3, 3, {"otype": "TriangleWave"}, {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 1})
    assert net.n_params() == 64 * 48 + 16 * 64
    om = O.mlp_init(48, 64, 3, 1)
    ph = O.f2h(O.mlp_init_params(om, O.pcg32(3)))
    _, y = net.fwd(torch.from_numpy(x_np).cuda(), h_t(ph))
    _, ref = O.mlp_forward(om, ph, R.triangle_wave_forward(x_np, 12, 48))
    assert np.percentile(rae(O.h2f(h_np(y)), O.h2f(ref)), 99) < (3e-2 if BF16 else 3e-3)  # (leaves out 1 % of the elements)


@pytest.mark.parametrize("n", SIZES)
def test_nrc_as_a_bare_encoding(n):
    C = tcnn()._C
    m = C.create_encoding(14, NRC)
    assert m.n_output_dims() == 62
    parts = R.nrc_parts(14)
    x_np = R.kink_inputs(n, 14, seed=2 * n)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    p = torch.zeros(0, dtype=HALF, device="cuda")
    ctx, y = m.fwd(x, p)
    assert np.array_equal(h_np(y), R.composite_forward(parts, x_np, 62))  # triangle wave | one-blob | identity, bit for bit
    _, y_inf = m.fwd(x.detach(), p)
    assert torch.equal(y, y_inf)
    dy = dy_half((n, 62), 2)
    dx, _ = m.bwd(ctx, x, p, y, h_t(dy))
    dx, ref = dx.cpu().numpy(), R.composite_backward_input(parts, x_np, dy, 14)
    assert np.array_equal(bits(dx[:, :3]), bits(ref[:, :3])) and np.array_equal(dx[:, 8:], ref[:, 8:])
    assert np.allclose(dx[:, 3:8], ref[:, 3:8], rtol=1e-5, atol=1e-5 * np.abs(ref[:, 3:8]).max())
    # fp32 values
    mf = C.create_encoding(14, NRC, C.Precision.Fp32)
    pf = torch.zeros(0, dtype=torch.float32, device="cuda")
    ctx, yf = mf.fwd(x, pf)
    yf = yf.cpu().numpy()
    assert np.array_equal(yf[:, :36], R.triangle_wave_forward(x_np[:, :3], 12, fp32=True)) and np.array_equal(yf[:, 56:], x_np[:, 8:])
    assert np.abs(yf[:, 36:56] - O.h2f(O.oneblob_forward(x_np[:, 3:8], 4))).max() <= (2.0 ** -8 if BF16 else 2.0 ** -11)  # one rounding of a value below 1 to the 16-bit type
    dyf = (O.h2f(dy) * np.float32(1.37)).astype(np.float32)
    dxf, _ = mf.bwd(ctx, x, pf, torch.from_numpy(yf).cuda(), torch.from_numpy(dyf).cuda())
    dxf = dxf.cpu().numpy()
    assert np.array_equal(bits(dxf[:, :3]), bits(R.triangle_wave_backward(x_np[:, :3], 12, dyf[:, :36]))) and np.array_equal(dxf[:, 8:], dyf[:, 56:])


@pytest.mark.parametrize("n", SIZES)
def test_composite_with_a_frequency_part_and_unread_dims(n):
    """[Frequency 3 on dims 5..6, OneBlob 2 bins on dims 0..1]: dims 2..4 and 7 are read by nobody, their dL_dinput is zero"""
    C = tcnn()._C
    cfg = {"otype": "Composite", "nested": [{"n_dims_to_encode": 2, "dims_to_encode_begin": 5, "otype": "Frequency", "n_frequencies": 3},
                                            {"n_dims_to_encode": 2, "dims_to_encode_begin": 0, "otype": "OneBlob", "n_bins": 2}]}
    m = C.create_encoding(8, cfg)
    assert m.n_output_dims() == 16
    parts = [dict(kind="Frequency", begin=5, dims=2, row=0, padded=12, n_frequencies=3), dict(kind="OneBlob", begin=0, dims=2, row=12, padded=4, n_bins=2)]
    x_np = R.kink_inputs(n, 8, seed=5)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    p = torch.zeros(0, dtype=HALF, device="cuda")
    ctx, y = m.fwd(x, p)
    got, ref = h_np(y), R.composite_forward(parts, x_np, 16)
    assert np.array_equal(got[:, 12:], ref[:, 12:])
    assert np.mean(got[:, :12] != ref[:, :12]) < 2e-3 and np.max(np.abs(O.h2f(got[:, :12]) - O.h2f(ref[:, :12]))) <= FREQ_ULPS
    dy = dy_half((n, 16), 3)
    dx, _ = m.bwd(ctx, x, p, y, h_t(dy))
    dx, dref = dx.cpu().numpy(), R.composite_backward_input(parts, x_np, dy, 8)
    assert not dx[:, 2:5].any() and not dx[:, 7].any()
    assert np.allclose(dx[:, 5:7], dref[:, 5:7], rtol=1e-4, atol=1e-4 * np.abs(dref[:, 5:7]).max())
    assert np.allclose(dx[:, :2], dref[:, :2], rtol=1e-5, atol=1e-5 * np.abs(dref[:, :2]).max())


@pytest.mark.parametrize("n", SIZES)
def test_identity_grid_triangle_wave(n):
    C = tcnn()._C
    m = C.create_encoding(8, MIXED)
    og = oracle_grid(GRID, 3)
    assert m.n_output_dims() == 16 and m.n_params() == og.n_params
    parts = mixed_parts(og)
    x_np = R.kink_inputs(n, 8, seed=7)
    params = O.f2h(O.generate_random_uniform(O.pcg32(9), og.n_params, -0.5, 0.5))
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    assert np.array_equal(h_np(y), R.composite_forward(parts, x_np, 16, params))  # identity (padded 3 -> 4 with 1) | grid | triangle wave
    dy = dy_half((n, 16), 4)
    dx, dp = m.bwd(ctx, x, p, y, h_t(dy))
    pos = np.ascontiguousarray(x_np[:, 3:6])
    check_grid_gradient(dp.float().cpu().numpy().astype(np.float64), og, pos, np.ascontiguousarray(dy[:, 4:12]))
    dx, ref = dx.cpu().numpy(), R.composite_backward_input(parts, x_np, dy, 8, params)
    assert np.array_equal(dx[:, :3], ref[:, :3]) and np.array_equal(bits(dx[:, 6:]), bits(ref[:, 6:]))
    assert np.allclose(dx[:, 3:6], ref[:, 3:6], rtol=1e-4, atol=1e-3 * np.abs(ref[:, 3:6]).max())
    # fp32 instantiation: the grid slice is the oracle's fp32 grid, bit for bit
    mf = C.create_encoding(8, MIXED, C.Precision.Fp32)
    pf32 = (np.random.default_rng(1).standard_normal(og.n_params) * 0.3).astype(np.float32)
    _, yf = mf.fwd(x.detach(), torch.from_numpy(pf32).cuda())
    yf = yf.cpu().numpy()
    assert np.array_equal(bits(yf[:, 4:12]), bits(O.grid_forward_f32(og, pf32, pos)))
    assert np.array_equal(yf[:, :3], x_np[:, :3]) and np.all(yf[:, 3] == 1.0) and np.array_equal(yf[:, 12:], R.triangle_wave_forward(x_np[:, 6:], 2, fp32=True))


def test_grid_gradients_behind_a_network_overwrite_accumulate_and_two_grids():
    """through the Trainer: the grid slice's gradients land at the nested grid's own parameter offset; a second backward in
    GradientMode::Accumulate doubles them (exactly: the same rounded sums are added); with two grids, the one whose dL_dy rows are zero
    keeps a zero slice"""
    T = tcnn()
    GM = T._C.GradientMode
    n = 768
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    tm = T.create_from_config(8, 3, {"loss": {"otype": "L2"}, "optimizer": ADAM, "encoding": MIXED, "network": net}, seed=11)
    og = oracle_grid(GRID, 3)
    nm = 64 * 16 + 64 * 64 + 16 * 64
    assert tm.n_params == nm + og.n_params
    w = tm.params_full_precision.cpu().numpy().copy()
    w[nm:] *= 1.0e3  # grid.h:1076-1079 initialises in U(-1e-4, 1e-4)
    tm.set_params_full_precision(torch.from_numpy(w))
    x_np = R.kink_inputs(n, 8, seed=13)
    x = torch.from_numpy(x_np).cuda()
    t = torch.from_numpy(np.random.default_rng(3).random((n, 3), dtype=np.float32)).cuda()
    # composed reference: encode, network forward, loss, network backward, the grid's backward on ITS rows of dL_denc
    ph = h_np(tm.params)
    om = O.mlp_init(16, 64, 3, 2)
    enc = R.composite_forward(mixed_parts(og, 16), x_np, 16, ph[nm:])
    hid, out = O.mlp_forward(om, ph[:nm], enc)
    dx = torch.zeros((n, 8), device="cuda")
    ctx = tm.training_step(x, t, run_optimizer=False, dL_dinput=dx)
    _, g_loss = O.loss(O.LOSS_L2, h_np(ctx.output), t.cpu().numpy(), 3)
    assert np.array_equal(h_np(ctx.dL_doutput), g_loss)
    _, denc = O.mlp_backward(om, ph[:nm], enc, hid, out, g_loss)
    g1 = tm.param_gradients.float().cpu().numpy().astype(np.float64)
    check_grid_gradient(g1[nm:], og, np.ascontiguousarray(x_np[:, 3:6]), np.ascontiguousarray(denc[:, 4:12]))
    tm.training_step(x, t, run_optimizer=False, gradient_mode=GM.Accumulate)
    g2 = tm.param_gradients.float().cpu().numpy().astype(np.float64)
    assert np.array_equal(g2[nm:], 2 * g1[nm:])
    tm.training_step(x, t, run_optimizer=False, gradient_mode=GM.Overwrite)
    assert np.array_equal(tm.param_gradients.float().cpu().numpy().astype(np.float64)[nm:], g1[nm:])

    # two grids, bare: each at its own offset
    C = T._C
    g_b = dict(GRID, n_levels=3, n_features_per_level=2)
    m = C.create_encoding(5, {"otype": "Composite", "nested": [dict(GRID, n_dims_to_encode=3), dict(g_b, n_dims_to_encode=2)]})
    oa, ob = og, oracle_grid(g_b, 2)
    assert m.n_params() == oa.n_params + ob.n_params and m.n_output_dims() == 14
    params = O.f2h(O.generate_random_uniform(O.pcg32(4), m.n_params(), -0.5, 0.5))
    x5 = R.kink_inputs(n, 5, seed=2)
    xt, p = torch.from_numpy(x5).cuda().requires_grad_(True), h_t(params).requires_grad_(True)
    ctx, y = m.fwd(xt, p)
    parts = [dict(kind="Grid", begin=0, dims=3, row=0, padded=8, grid=oa, params_offset=0), dict(kind="Grid", begin=3, dims=2, row=8, padded=6, grid=ob, params_offset=oa.n_params)]
    assert np.array_equal(h_np(y), R.composite_forward(parts, x5, 14, params))
    dy = dy_half((n, 14), 6)
    dy[:, :8] = 0  # the first grid receives no gradient
    dxx, dp = m.bwd(ctx, xt, p, y, h_t(dy))
    dp = dp.float().cpu().numpy().astype(np.float64)
    assert not dp[:oa.n_params].any()
    check_grid_gradient(dp[oa.n_params:], ob, np.ascontiguousarray(x5[:, 3:]), np.ascontiguousarray(dy[:, 8:]))
    ref = R.composite_backward_input(parts, x5, dy, 5, params)
    assert not dxx.cpu().numpy()[:, :3].any() and np.allclose(dxx.cpu().numpy()[:, 3:], ref[:, 3:], rtol=1e-4, atol=1e-3 * np.abs(ref[:, 3:]).max())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("reduction", ["Sum", "Product"])
def test_sum_and_product(n, reduction):
    """OneBlob 4 bins on 4 dims and TriangleWave 4 frequencies on 4 other dims, width 16"""
    C = tcnn()._C
    product = reduction == "Product"
    m = C.create_encoding(8, {"otype": "Composite", "reduction": reduction, "nested": [{"n_dims_to_encode": 4, "otype": "OneBlob", "n_bins": 4},
                                                                                       {"n_dims_to_encode": 4, "otype": "TriangleWave", "n_frequencies": 4}]})
    assert m.n_output_dims() == 16
    parts = [dict(kind="OneBlob", begin=0, dims=4, row=0, padded=16, n_bins=4), dict(kind="TriangleWave", begin=4, dims=4, row=16, padded=16, n_frequencies=4)]
    x_np = R.kink_inputs(n, 8, seed=17)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    p = torch.zeros(0, dtype=HALF, device="cuda")
    ctx, y = m.fwd(x, p)
    unreduced = R.composite_forward(parts, x_np, 32)
    assert np.array_equal(h_np(y), R.reduce_forward(unreduced, 16, product))
    _, y_inf = m.fwd(x.detach(), p)
    assert torch.equal(y, y_inf)
    dy = dy_half((n, 16), 8)
    dx, _ = m.bwd(ctx, x, p, y, h_t(dy))
    ref = R.composite_backward_input(parts, x_np, R.reduce_backward(unreduced, dy, 16, 2, product), 8)
    dx = dx.cpu().numpy()
    assert np.array_equal(bits(dx[:, 4:]), bits(ref[:, 4:]))  # the triangle wave's rows of the reduction's gradient, bit for bit
    assert np.allclose(dx[:, :4], ref[:, :4], rtol=1e-5, atol=1e-5 * np.abs(ref[:, :4]).max())


@pytest.mark.parametrize("net", [{"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2}, {"otype": "CutlassMLP", "n_neurons": 256, "n_hidden_layers": 2}], ids=["fused-64x2", "cutlass-256x2"])
def test_nrc_network_training_step(net):
    """NRC -> network -> 3 outputs: one training_step(run_optimizer=False, dL_dinput) against encode (oracle parts) -> O.mlp_forward -> O.loss ->
    O.mlp_backward -> the parts' backward; inference == the forward's output; 30 optimizer steps lower the loss"""
    T = tcnn()
    net = dict(net, activation="ReLU", output_activation="None")
    tm = T.create_from_config(14, 3, {"loss": {"otype": "RelativeL2"}, "optimizer": ADAM, "encoding": NRC, "network": net}, seed=21)
    W = net["n_neurons"]
    om = O.mlp_init(64, W, 3, 2)
    assert tm.n_params == om.n_params
    n = 768
    x_np = R.kink_inputs(n, 14, seed=23)
    tgt = np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c + 1) * x_np[:, 0]) * np.cos(2 * np.pi * x_np[:, 4]) for c in range(3)], 1).astype(np.float32)
    x, t = torch.from_numpy(x_np).cuda(), torch.from_numpy(tgt).cuda()
    ph = h_np(tm.params)
    parts = R.nrc_parts(14, 16)
    enc = R.composite_forward(parts, x_np, 64)
    hid, out = O.mlp_forward(om, ph, enc)
    values, g_loss = O.loss(O.LOSS_RELATIVE_L2, out, tgt, 3)
    gref, denc = O.mlp_backward(om, ph, enc, hid, out, g_loss)
    dx_ref = R.composite_backward_input(parts, x_np, denc, 14)
    dx = torch.full((n, 14), 7.0, device="cuda")
    ctx = tm.training_step(x, t, run_optimizer=False, dL_dinput=dx)
    loss_ref = float(values.sum(dtype=np.float64))
    assert abs(tm.loss(ctx) - loss_ref) <= (2e-2 if BF16 else 2e-3) * abs(loss_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(out)), 99) < (3e-2 if BF16 else 3e-3)  # (1 % of the elements left out)
    _, g_own = O.loss(O.LOSS_RELATIVE_L2, h_np(ctx.output), tgt, 3)
    assert np.array_equal(h_np(ctx.dL_doutput), g_own)
    g = tm.param_gradients.float().cpu().numpy()
    assert np.percentile(rae(g, gref), 99) < (5e-2 if BF16 else 5e-3)  # (1 % of the elements left out)
    assert rel_l2(dx.cpu().numpy(), dx_ref) < 2e-2
    # external_dL_dy and Accumulate through the composite: twice the network gradient (to a rounding), the same dL_dinput
    dx2 = torch.zeros((n, 14), device="cuda")
    tm.training_step(x, t, run_optimizer=False, dL_dinput=dx2, external_dL_dy=ctx.dL_doutput, gradient_mode=T._C.GradientMode.Accumulate)
    assert rel_l2(dx2.cpu().numpy(), dx_ref) < 2e-2
    g2 = tm.param_gradients.float().cpu().numpy()
    assert np.percentile(rae(g2, 2 * gref), 99) < (5e-2 if BF16 else 5e-3)  # (1 % of the elements left out)
    y_inf = tm.inference(x).cpu().numpy()
    assert np.array_equal(y_inf, ctx.output.float().cpu().numpy()[:, :3])
    first = tm.loss(tm.training_step(x, t))
    for _ in range(29):
        tm.training_step(x, t, want_context=False)
    assert tm.loss(tm.training_step(x, t, run_optimizer=False)) < first


def test_torch_modules():
    """tcnn.Encoding(14, nrc) and tcnn.NetworkWithInputEncoding(14, 3, nrc, net): a batch of 300 is padded to 512 inside the module; autograd
    to the input and to the parameters equals the native calls on the padded batch"""
    T = tcnn()
    n = 300
    x_np = R.kink_inputs(512, 14, seed=29)[:n]
    enc = T.Encoding(14, NRC)
    assert enc.n_output_dims == 62
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    y = enc(x)
    assert y.shape == (n, 62) and y.dtype == HALF
    assert np.array_equal(h_np(y), R.composite_forward(R.nrc_parts(14), x_np, 62))
    w_np = O.h2f(dy_half((n, 62), 5))
    (y.float() * torch.from_numpy(w_np).cuda()).sum().backward()
    # the module multiplies the incoming gradient by its loss scale, rounds it to the 16-bit type and divides dL_dinput by the scale again
    scale = enc.loss_scale
    dy16 = O.f2h(w_np * np.float32(scale))
    ref = R.composite_backward_input(R.nrc_parts(14), x_np, dy16, 14) / np.float32(scale)
    got = x.grad.cpu().numpy()
    assert np.allclose(got[:, :3], ref[:, :3], rtol=1e-6, atol=0) and np.allclose(got[:, 8:], ref[:, 8:], rtol=1e-6, atol=0)
    assert np.allclose(got[:, 3:8], ref[:, 3:8], rtol=1e-5, atol=1e-5 * np.abs(ref[:, 3:8]).max())

    net_cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    model = T.NetworkWithInputEncoding(14, 3, NRC, net_cfg, seed=3)
    native = model.native_tcnn_module
    assert model.params.shape[0] == native.n_params() == 64 * 64 * 2 + 16 * 64
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    y = model(x)
    assert y.shape == (n, 3) and torch.equal(y, model(x))
    tgt = torch.from_numpy(np.random.default_rng(1).random((n, 3), dtype=np.float32)).cuda()
    ((y.float() - tgt) ** 2).mean().backward()
    g, gx = model.params.grad, x.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0 and torch.isfinite(gx).all() and gx.abs().sum() > 0
    # the same through the native calls on the padded batch
    xp = torch.zeros((512, 14), device="cuda")
    xp[:n] = x.detach()
    xp.requires_grad_(True)
    ph = model.params.detach().to(HALF).requires_grad_(True)
    ctx, yp = native.fwd(xp, ph)
    assert torch.equal(yp[:n, :3], y)
    dy = torch.zeros((512, 16), device="cuda")
    # (autograd hands the module the loss gradient rounded to the 16-bit type -- the backward of `.float()` -- and the module scales THAT)
    dy[:n, :3] = (2.0 * (y.float().detach() - tgt) / (n * 3)).to(HALF).float() * scale
    dxp, dpp = native.bwd(ctx, xp, ph, yp, dy.to(HALF))
    assert np.allclose(gx.cpu().numpy(), dxp[:n].cpu().numpy() / scale, rtol=1e-5, atol=1e-12)
    assert np.allclose(g.cpu().numpy(), dpp.float().cpu().numpy() / scale, rtol=2.0 ** (-7 if BF16 else -10), atol=2.0 ** -24)


def test_bf16_build_passes_the_composite_cases():
    assert not BF16  # (the bf16 run deselects this test)
    env = dict(os.environ, TCNN_PRECISION="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "--tb=short",
                        "--deselect", "tests/test_gpu_composite.py::test_bf16_build_passes_the_composite_cases"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout.split("\n")[-2], tail

"""The fp32 network on a real MI355X against a numpy float64 MLP, all ten hidden activations and the seven output activations, at
n = 512 for 32 -> 64 x 2 -> 4 and 16 -> 272 x 1 -> 144; inputs U(-1, 1), Xavier weights and dL/doutput U(-1, 1) from a fixed seed.

The bar is not a constant.  For each compared quantity (prediction, dL/dinput, parameter gradients) the test measures, on the CPU, the
maximum absolute error of a plain numpy float32 restatement (layer by layer, np.float32 matmul, float32 activations) against the float64
reference ON THE SAME INPUTS; the GPU may exceed that by FACTOR = 8, which covers its different summation order (16x16x4 MFMA chains, K in
stages, batch slabs) and the few-ulp differences of the device's expf / sinf / tanhf.  Measured CPU figures (max |float32 - float64|,
ReLU hidden, None output):
    32 -> 64 x 2 -> 4:     prediction 2.2e-07, dL/dinput 1.2e-07, parameter gradients 7.2e-06
    16 -> 272 x 1 -> 144:  prediction 3.2e-07, dL/dinput 7.0e-07, parameter gradients 6.4e-06
so the GPU is held to about 2e-6 on predictions of magnitude 1 and 5e-5 on gradient sums over 512 samples of magnitude 10.  The other
activations measure between a third and four times these; Exponential more (2.7e-05 on its predictions, whose values are larger).  On
the MI355X the fp32 network measured 0.3 to 1.5 times the CPU figure on every quantity; the 16-bit modules 3e-04 to 4e-02 on the prediction.
For ReLU / LeakyReLU the seed is advanced until no float64 pre-activation lies within 2e-6 of zero (twenty times the fp32 error of a
pre-activation): closer than that, fp32 rounding decides the branch of the derivative and no summation-order bar applies.
The 16-bit module of the same configuration on the same inputs must EXCEED the fp32 bar on the prediction: the bar separates the paths.
Further cases: an fp32 HashGrid in front of the network (features bit-equal to the bare fp32 encoding's; prediction and gradients under the
same rule), and the PyTorch modules (dtype=torch.float32, a batch padded from n = 300; gradients bit-equal to the C-ABI path's)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FACTOR = 8.0
N = 512
SHAPES = {"32-64x2-4": (32, 64, 2, 4), "16-272x1-144": (16, 272, 1, 144)}
HIDDEN = ["None", "ReLU", "LeakyReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh", "SiLU", "Sine"]
OUTPUT = ["ReLU", "LeakyReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh"]
K = 10.0


def tcnn():
    import tinycudann
    return tinycudann


def act(name, x):
    """activation and its derivative in the dtype of x (float64: the reference; float32: the restatement)"""
    t = x.dtype.type
    one, k = t(1), t(K)
    if name == "None":
        return x, np.ones_like(x)
    if name == "ReLU":
        return np.maximum(x, t(0)), (x > 0).astype(x.dtype)
    if name == "LeakyReLU":
        return np.where(x > 0, x, x * t(0.01)), np.where(x > 0, one, t(0.01))
    if name == "Exponential":
        return np.exp(x), np.exp(x)
    if name == "Sigmoid":
        s = one / (one + np.exp(-x))
        return s, s * (one - s)
    if name == "Squareplus":
        y = x * k
        r = np.sqrt(y * y + t(4))
        return t(0.5) * (y + r) / k, t(0.5) * (one + y / r)
    if name == "Softplus":
        return np.log(np.exp(x * k) + one) / k, one / (one + np.exp(-x * k))
    if name == "Tanh":
        y = np.tanh(x)
        return y, one - y * y
    if name == "SiLU":
        s = one / (one + np.exp(-x))
        return x * s, s + x * (s * (one - s))
    if name == "Sine":
        return np.sin(x), np.cos(x)
    raise KeyError(name)


def mlp(dtype, mats, x, dy, hidden_act, output_act):
    """forward and backward of the network in `dtype` -> prediction [n][OUTP], dL/dinput [n][IN], parameter gradients (flat), the
    pre-activations of the hidden layers"""
    mats, a, dy = [m.astype(dtype) for m in mats], x.astype(dtype), dy.astype(dtype)
    acts, derivs, pres = [a], [], []
    for m in mats[:-1]:
        pre = a @ m.T
        a, d = act(hidden_act, pre)
        acts.append(a)
        derivs.append(d)
        pres.append(pre)
    out, dout = act(output_act, acts[-1] @ mats[-1].T)
    d = dy * dout
    grads = [None] * len(mats)
    for l in range(len(mats) - 1, -1, -1):
        grads[l] = d.T @ acts[l]
        back = d @ mats[l]
        d = back * derivs[l - 1] if l > 0 else back
    return out, d, np.concatenate([g.reshape(-1) for g in grads]), pres


def draw(shape, hidden_act, seed, given_x=None):
    """Xavier weights, inputs (given_x: the caller's instead) and dL/doutput from `seed`, advanced as the module's docstring says"""
    IN, W, H, OUT = shape
    OUTP = (OUT + 15) // 16 * 16
    while True:
        rng = np.random.default_rng(seed)
        mats = []
        for rows, cols in [(W, IN)] + [(W, W)] * (H - 1) + [(OUTP, W)]:
            s = np.sqrt(6.0 / (rows + cols))
            mats.append(rng.uniform(-s, s, size=(rows, cols)).astype(np.float32))
        mats[-1][OUT:] = 0  # the padded output rows
        x = rng.uniform(-1, 1, size=(N, IN)).astype(np.float32)
        if given_x is not None:
            x = given_x
        dy = np.zeros((N, OUTP), np.float32)
        dy[:, :OUT] = rng.uniform(-1, 1, size=(N, OUT))
        if hidden_act not in ("ReLU", "LeakyReLU"):
            return mats, x, dy
        pres = mlp(np.float64, mats, x, dy, hidden_act, "None")[3]
        if min(float(np.abs(p).min()) for p in pres) > 2e-6:
            return mats, x, dy
        seed += 1000


_cache = {}


def reference(shape_name, hidden_act, output_act):
    """inputs, the float64 reference and the measured CPU float32 errors, computed once and shared"""
    key = (shape_name, hidden_act, output_act)
    if key not in _cache:
        mats, x, dy = draw(SHAPES[shape_name], hidden_act, seed=20260 + 7 * len(shape_name))
        ref = mlp(np.float64, mats, x, dy, hidden_act, output_act)[:3]
        f32 = mlp(np.float32, mats, x, dy, hidden_act, output_act)[:3]
        cpu_error = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(f32, ref)]
        _cache[key] = (mats, x, dy, ref, cpu_error)
    return _cache[key]


def network(W, H, hidden_act, output_act, otype="CutlassMLP"):
    return {"otype": otype, "activation": hidden_act, "output_activation": output_act, "n_neurons": W, "n_hidden_layers": H}


NAMES = ("prediction", "dL/dinput", "parameter gradients")


def run_fp32(shape_name, hidden_act, output_act):
    C = tcnn()._C
    IN, W, H, OUT = SHAPES[shape_name]
    mats, x, dy, ref, cpu_error = reference(shape_name, hidden_act, output_act)
    m = C.create_network_precision(IN, OUT, network(W, H, hidden_act, output_act), C.Precision.Fp32)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    pt = torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda().requires_grad_(True)
    ctx, y = m.fwd(xt, pt)
    dx, dp = m.bwd(ctx, xt, pt, y, torch.from_numpy(dy).cuda())
    torch.cuda.synchronize()
    got = [t.detach().cpu().numpy().astype(np.float64) for t in (y, dx, dp)]
    report = []
    for name, g, r, e in zip(NAMES, got, ref, cpu_error):
        err = float(np.abs(g - r).max())
        print(f"{shape_name} {hidden_act}/{output_act} {name}: GPU max error {err:.3e}, CPU float32 {e:.3e}, bar {FACTOR * e:.3e}, max |reference| {np.abs(r).max():.3e}")
        assert np.isfinite(g).all()
        if not err <= FACTOR * e:
            report.append(f"{name}: GPU max error {err:.3e} exceeds {FACTOR} x the CPU float32 error {e:.3e}")
    assert not report, "; ".join(report)
    return cpu_error


@pytest.mark.parametrize("hidden_act", HIDDEN)
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_hidden_activations(shape_name, hidden_act):
    run_fp32(shape_name, hidden_act, "None")


@pytest.mark.parametrize("output_act", OUTPUT)
def test_output_activations(output_act):
    run_fp32("32-64x2-4", "ReLU", output_act)


@pytest.mark.parametrize("hidden_act", HIDDEN)
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_the_bar_separates_fp32_from_16_bit(shape_name, hidden_act):
    """the 16-bit module of the same configuration on the same inputs exceeds the fp32 bar on the prediction"""
    C = tcnn()._C
    IN, W, H, OUT = SHAPES[shape_name]
    mats, x, dy, ref, cpu_error = reference(shape_name, hidden_act, "None")
    m = C.create_network(IN, OUT, network(W, H, hidden_act, "None"))
    half = C.TORCH_DTYPE[C.preferred_precision()]
    _, y = m.fwd(torch.from_numpy(x).cuda(), torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda().to(half))
    torch.cuda.synchronize()
    err = float(np.abs(y.float().cpu().numpy().astype(np.float64) - ref[0]).max())
    print(f"{shape_name} {hidden_act}: 16-bit prediction max error {err:.3e} against the fp32 bar {FACTOR * cpu_error[0]:.3e}")
    assert err > FACTOR * cpu_error[0]


GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}


def test_fp32_hashgrid_in_front_of_the_network():
    C = tcnn()._C
    rng = np.random.default_rng(77)
    pos = torch.from_numpy(rng.uniform(0, 1, size=(N, 3)).astype(np.float32)).cuda()
    enc = C.create_encoding(3, GRID, C.Precision.Fp32)
    n_grid = enc.n_params()
    table = torch.from_numpy(rng.uniform(-1, 1, size=n_grid).astype(np.float32)).cuda()
    _, feat = enc.fwd(pos, table)
    assert feat.shape == (N, 8)
    # 1. the features the network is handed: a 16-wide linear network with unit matrices copies them (1 * x + 0 + ... is exact)
    copy = C.create_network_with_input_encoding_precision(3, 8, GRID, network(16, 1, "None", "None"), C.Precision.Fp32)
    eye = np.eye(16, dtype=np.float32)
    p = torch.cat([torch.from_numpy(np.concatenate([eye.reshape(-1), eye.reshape(-1)])).cuda(), table])
    _, y = copy.fwd(pos, p)
    torch.cuda.synchronize()
    assert y.shape == (N, 16) and np.array_equal(y[:, :8].cpu().numpy().view(np.uint32), feat.cpu().numpy().view(np.uint32))
    assert bool((y[:, 8:] == 0).all())  # the padded features are zero
    # 2. a real network behind it: the float64 MLP on the bare encoding's features; the encoding's share of the backward pass is linear in
    # dL/dfeatures, so its reference is the bare fp32 encoding's backward pass on the float64 network's dL/dfeatures, and its bar the same
    # pass on the difference between the CPU float32 and the float64 dL/dfeatures
    IN, W, H, OUT = 16, 64, 2, 4
    x = np.zeros((N, 16), np.float32)
    x[:, :8] = feat.cpu().numpy()
    mats, _, dy = draw((IN, W, H, OUT), "ReLU", seed=4242, given_x=x)
    ref = mlp(np.float64, mats, x, dy, "ReLU", "None")[:3]
    f32 = mlp(np.float32, mats, x, dy, "ReLU", "None")[:3]
    m = C.create_network_with_input_encoding_precision(3, OUT, GRID, network(W, H, "ReLU", "None"), C.Precision.Fp32)
    assert m.n_params() == sum(a.size for a in mats) + n_grid
    pt = torch.cat([torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda(), table]).requires_grad_(True)
    post = pos.clone().requires_grad_(True)
    ctx, y = m.fwd(post, pt)
    dx, dp = m.bwd(ctx, post, pt, y, torch.from_numpy(dy).cuda())

    def encoding_backward(dfeat):
        pe, te = pos.clone().requires_grad_(True), table.clone().requires_grad_(True)
        c, f = enc.fwd(pe, te)
        gx, gt = enc.bwd(c, pe, te, f, torch.from_numpy(np.ascontiguousarray(dfeat[:, :8], np.float32)).cuda())
        return gx.cpu().numpy().astype(np.float64), gt.cpu().numpy().astype(np.float64)

    ref_dx, ref_dtable = encoding_backward(ref[1])
    cpu_dx, cpu_dtable = encoding_backward(f32[1])
    torch.cuda.synchronize()
    n_mlp = sum(a.size for a in mats)
    pairs = [("prediction", y.cpu().numpy(), ref[0], np.abs(f32[0] - ref[0]).max()),
             ("network parameter gradients", dp[:n_mlp].cpu().numpy(), ref[2], np.abs(f32[2] - ref[2]).max()),
             ("grid parameter gradients", dp[n_mlp:].cpu().numpy(), ref_dtable, np.abs(cpu_dtable - ref_dtable).max()),
             ("dL/dinput", dx.cpu().numpy(), ref_dx, np.abs(cpu_dx - ref_dx).max())]
    report = []
    for name, g, r, e in pairs:
        err = float(np.abs(g.astype(np.float64) - r).max())
        print(f"hashgrid + 64x2 {name}: GPU max error {err:.3e}, CPU float32 {float(e):.3e}, max |reference| {np.abs(r).max():.3e}")
        if not err <= FACTOR * float(e):
            report.append(f"{name}: GPU max error {err:.3e} exceeds {FACTOR} x {float(e):.3e}")
    assert not report, "; ".join(report)
    # max_level keeps working on the lone grid
    m.set_max_level(0.5)
    assert m.max_level() == 0.5


def test_pytorch_modules_in_fp32():
    """Network(dtype=torch.float32): forward and backward() on a batch padded from n = 300; dtypes, loss scale, and the C-ABI path's bits"""
    T = tcnn()
    C = T._C
    IN, W, H, OUT = SHAPES["32-64x2-4"]
    cfg = network(W, H, "ReLU", "None", otype="FullyFusedMLP")
    net = T.Network(IN, OUT, cfg, seed=7, dtype=torch.float32)
    assert net.dtype == torch.float32 and net.params.dtype == torch.float32 and net.loss_scale == 1.0
    assert net.native_tcnn_module.hyperparams()["network"]["otype"] == "CutlassMLP"
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(300, IN)).astype(np.float32)).cuda().requires_grad_(True)
    w = torch.from_numpy(rng.uniform(-1, 1, size=(300, OUT)).astype(np.float32)).cuda()
    y = net(x)
    assert y.dtype == torch.float32 and y.shape == (300, OUT)
    (y * w).sum().backward()
    assert x.grad.dtype == torch.float32 and net.params.grad.dtype == torch.float32 and net.params.grad.shape == net.params.shape
    # the C-ABI path on the batch padded to 512 with zero rows and zero output gradients
    m = C.create_network_precision(IN, OUT, cfg, C.Precision.Fp32)
    xp = torch.zeros((512, IN), device="cuda")
    xp[:300] = x.detach()
    dyp = torch.zeros((512, 16), device="cuda")
    dyp[:300, :OUT] = w
    xp.requires_grad_(True)
    p = net.params.detach().clone().requires_grad_(True)
    ctx, yp = m.fwd(xp, p)
    dx, dp = m.bwd(ctx, xp, p, yp, dyp)
    torch.cuda.synchronize()
    assert torch.equal(yp[:300, :OUT], y.detach())
    assert np.array_equal(dx[:300].cpu().numpy().view(np.uint32), x.grad.cpu().numpy().view(np.uint32))
    assert np.array_equal(dp.cpu().numpy().view(np.uint32), net.params.grad.cpu().numpy().view(np.uint32))
    # NetworkWithInputEncoding(dtype=torch.float32) runs end to end in fp32 as well
    nwie = T.NetworkWithInputEncoding(3, OUT, GRID, cfg, dtype=torch.float32)
    pos = torch.rand((300, 3), device="cuda", requires_grad=True)
    out = nwie(pos)
    out.sum().backward()
    assert out.dtype == torch.float32 and nwie.params.grad.dtype == torch.float32 and pos.grad.dtype == torch.float32
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(nwie.params.grad).all())

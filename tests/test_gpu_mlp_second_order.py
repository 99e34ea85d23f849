"""The second-order pass of the fp32 network on a real MI355X (tcnn_module_backward_backward_input on the modules of
tcnn_create_network_precision): dL/d(dL/doutput), dL/dinput and the parameter gradients of S = <v, dL/dinput> against the float64 numpy
restatement of tests/second_order_mlp_reference.py.

Through the C ABI: 32 -> 64 x 2 -> 4 and 16 -> 272 x 1 -> 144 at n = 512, all ten hidden activations with a None output, the seven output
activations with Tanh hidden on the first shape; weights, inputs and dL/doutput from the generator of tests/test_gpu_f32_network.py (its
seeds, its advance away from ReLU kinks), v ~ U(-1, 1).  The bar is that file's rule, unchanged: per result, the CPU float32 restatement's
max error against float64 on the same inputs, times FACTOR = 8.  Measured, max |. - float64| as CPU float32 / MI355X, for
dL/d(dL/doutput), dL/dinput and the parameter gradients:
    32 -> 64 x 2 -> 4     Tanh / None      5.5e-07 / 4.9e-07,  1.3e-07 / 1.5e-07,  6.7e-06 / 3.0e-06
    32 -> 64 x 2 -> 4     Softplus / None  3.1e-07 / 3.0e-07,  2.4e-07 / 2.3e-07,  4.7e-06 / 2.3e-06
    16 -> 272 x 1 -> 144  Tanh / None      7.0e-07 / 8.0e-07,  1.1e-07 / 1.2e-07,  1.2e-05 / 7.8e-06
    16 -> 272 x 1 -> 144  Softplus / None  4.3e-07 / 3.7e-07,  7.2e-07 / 6.1e-07,  6.8e-06 / 5.0e-06
so the GPU sits at about the CPU float32 restatement's own error, an eighth of the bar.  Every case prints its figures (run with -s).
Through torch, on both bindings: Network(32, 4, Softplus, dtype=torch.float32) on a batch padded from n = 300 under the eikonal loss
((|dy/dx| - 1)^2).mean(): params.grad against a float64 torch MLP with the same weights, the bar FACTOR times the error of the same torch
MLP in float32; the same behind Encoding(HashGrid, dtype=torch.float32) composed in torch, against that encoding composed with the float64
MLP; and a 16-bit Network still raises "not implemented"."""
import numpy as np
import pytest
import torch

import second_order_mlp_reference as R
import test_gpu_f32_network as G

pytestmark = pytest.mark.gpu

FACTOR = G.FACTOR
NAMES = ("dL/d(dL/doutput)", "dL/dinput", "parameter gradients")
_cache = {}


def tcnn():
    import tinycudann
    return tinycudann


def reference(shape_name, hidden_act, output_act):
    key = (shape_name, hidden_act, output_act)
    if key not in _cache:
        mats, x, dy = G.draw(G.SHAPES[shape_name], hidden_act, seed=20260 + 7 * len(shape_name))
        v = np.random.default_rng(99 + len(shape_name)).uniform(-1, 1, size=x.shape).astype(np.float32)
        ref, cpu_error = R.errors(mats, x, dy, v, hidden_act, output_act)
        _cache[key] = (mats, x, dy, v, ref, cpu_error)
    return _cache[key]


def run(shape_name, hidden_act, output_act):
    C = tcnn()._C
    IN, W, H, OUT = G.SHAPES[shape_name]
    mats, x, dy, v, ref, cpu_error = reference(shape_name, hidden_act, output_act)
    m = C.create_network_precision(IN, OUT, G.network(W, H, hidden_act, output_act), C.Precision.Fp32)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    pt = torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda().requires_grad_(True)
    dyt = torch.from_numpy(dy).cuda().requires_grad_(True)
    ctx, _ = m.fwd(xt, pt)
    ddy, dp, dx = m.bwd_bwd_input(ctx, xt, pt, torch.from_numpy(v).cuda(), dyt)
    torch.cuda.synchronize()
    report = []
    for name, g, r, e in zip(NAMES, (ddy, dx, dp), ref, cpu_error):
        g = g.detach().cpu().numpy().astype(np.float64)
        err = float(np.abs(g - r).max())
        print(f"{shape_name} {hidden_act}/{output_act} {name}: GPU max error {err:.3e}, CPU float32 {e:.3e}, bar {FACTOR * e:.3e}, max |reference| {np.abs(r).max():.3e}")
        assert np.isfinite(g).all()
        if not err <= FACTOR * e:
            report.append(f"{name}: GPU max error {err:.3e} exceeds {FACTOR} x the CPU float32 error {e:.3e}")
    assert not report, "; ".join(report)


@pytest.mark.parametrize("hidden_act", G.HIDDEN)
@pytest.mark.parametrize("shape_name", list(G.SHAPES))
def test_hidden_activations(shape_name, hidden_act):
    run(shape_name, hidden_act, "None")


@pytest.mark.parametrize("output_act", G.OUTPUT)
def test_output_activations(output_act):
    run("32-64x2-4", "Tanh", output_act)


def test_single_results_and_argument_checks():
    """each result asked for alone has the bits it has next to the others; the argument checks carry the grid path's texts"""
    C = tcnn()._C
    IN, W, H, OUT = G.SHAPES["32-64x2-4"]
    mats, x, dy, v, _, _ = reference("32-64x2-4", "Softplus", "None")
    m = C.create_network_precision(IN, OUT, G.network(W, H, "Softplus", "None"), C.Precision.Fp32)
    p = torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).cuda()
    xt, vt, dyt = torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(dy).cuda()
    ctx, _ = m.fwd(xt.clone().requires_grad_(True), p.clone().requires_grad_(True))
    full = m.bwd_bwd_input(ctx, xt.clone().requires_grad_(True), p.clone().requires_grad_(True), vt, dyt.clone().requires_grad_(True))
    for k, flags in enumerate([(False, False, True), (False, True, False), (True, False, False)]):  # (x, params, dy) require a gradient
        alone = m.bwd_bwd_input(ctx, xt.clone().requires_grad_(flags[0]), p.clone().requires_grad_(flags[1]), vt, dyt.clone().requires_grad_(flags[2]))
        assert [r is not None for r in alone] == [flags[2], flags[1], flags[0]]
        assert torch.equal(alone[k], full[k])
    lib = C._lib
    import ctypes
    h = ctx._h if isinstance(ctx, C.Context) else ctypes.c_void_p(ctx.handle())  # (either binding's context)
    rc = lib.tcnn_module_backward_backward_input(m._h, None, h, 256, C._ptr(vt), C._ptr(xt), C._ptr(dyt), None, None, None, C._ptr(p))
    assert rc == 1 and b"batch size does not match the forward context" in lib.tcnn_last_error()
    rc = lib.tcnn_module_backward_backward_input(m._h, None, h, 512, None, C._ptr(xt), C._ptr(dyt), None, None, None, C._ptr(p))
    assert rc == 1 and b"dL_ddLdinput is required" in lib.tcnn_last_error()
    out = torch.empty_like(p)
    rc = lib.tcnn_module_backward_backward_input(m._h, None, h, 512, C._ptr(vt), C._ptr(xt), None, C._ptr(out), None, None, C._ptr(p))
    assert rc == 1 and b"dL_doutput is required" in lib.tcnn_last_error()


# ---- through torch ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    C = tcnn()._C
    if request.param == "compiled" and C.EXT is None:
        pytest.skip("the compiled binding is not built")
    if request.param == "ctypes":
        monkeypatch.setattr(C, "EXT", None)
    return request.param


IN, W, H, OUT, OUTP = 32, 64, 2, 4, 16
CFG = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": W, "n_hidden_layers": H}
GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}


def torch_mlp(params, feat, in_width, dtype):
    """the network of CFG as plain torch in `dtype`, on the module's flat parameters; the input padded with ones like the Identity encoding's"""
    p = params.detach().to(dtype).requires_grad_(True)
    sizes = [(W, in_width)] + [(W, W)] * (H - 1) + [(OUTP, W)]
    a = torch.cat([feat.to(dtype), torch.ones((feat.shape[0], in_width - feat.shape[1]), dtype=dtype, device=feat.device)], dim=1)
    off = 0
    for k, (rows, cols) in enumerate(sizes):
        a = a @ p[off:off + rows * cols].view(rows, cols).T
        off += rows * cols
        if k < len(sizes) - 1:
            a = torch.log(torch.exp(a * R.K) + 1.0) / R.K
    return p, a[:, :OUT]


def eikonal(y, x):
    gx, = torch.autograd.grad(y.sum(), [x], create_graph=True)
    return ((gx.norm(dim=1) - 1.0) ** 2).mean()


def held_to(name, got, ref, f32):
    err, e = float((got.double() - ref).abs().max()), float((f32.double() - ref).abs().max())
    print(f"{name}: GPU max error {err:.3e}, float32 torch MLP {e:.3e}, bar {FACTOR * e:.3e}, max |reference| {float(ref.abs().max()):.3e}")
    assert bool(torch.isfinite(got).all()) and float(ref.abs().max()) > 0
    assert err <= FACTOR * e, f"{name}: GPU max error {err:.3e} exceeds {FACTOR} x {e:.3e}"


def test_eikonal_loss_on_a_network(binding):
    T = tcnn()
    net = T.Network(IN, OUT, CFG, seed=11, dtype=torch.float32)
    x0 = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, size=(300, IN)).astype(np.float32)).cuda()
    x = x0.clone().requires_grad_(True)
    eikonal(net(x), x).backward()
    torch.cuda.synchronize()
    assert net.params.grad.dtype == torch.float32 and net.params.grad.shape == net.params.shape
    grads = {}
    for dtype in (torch.float64, torch.float32):
        xr = x0.to(dtype).requires_grad_(True)
        p, y = torch_mlp(net.params, xr, IN, dtype)
        eikonal(y, xr).backward()
        grads[dtype] = p.grad
    held_to(f"eikonal params.grad ({binding})", net.params.grad, grads[torch.float64], grads[torch.float32])
    _results[binding] = net.params.grad.detach().cpu().numpy().view(np.uint32)
    if len(_results) == 2:
        assert np.array_equal(_results["compiled"], _results["ctypes"]), "the two bindings give different bits"


_results = {}


def test_eikonal_loss_behind_a_hashgrid_composed_in_torch(binding):
    T = tcnn()
    enc = T.Encoding(3, GRID, seed=5, dtype=torch.float32)
    net = T.Network(enc.n_output_dims, OUT, CFG, seed=11, dtype=torch.float32)
    with torch.no_grad():
        enc.params.mul_(1000.0)  # (the grid's initial values are 1e-4: features that the network's curvature does not see)
    pos0 = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(300, 3)).astype(np.float32)).cuda()
    pos = pos0.clone().requires_grad_(True)
    eikonal(net(enc(pos)), pos).backward()
    torch.cuda.synchronize()
    got_net, got_enc = net.params.grad.clone(), enc.params.grad.clone()
    grads = {}
    for dtype in (torch.float64, torch.float32):
        enc.params.grad = None
        pos = pos0.clone().requires_grad_(True)
        p, y = torch_mlp(net.params, enc(pos), 16, dtype)
        eikonal(y, pos).backward()
        grads[dtype] = (p.grad, enc.params.grad.clone())
    held_to(f"hashgrid + network, network params.grad ({binding})", got_net, grads[torch.float64][0], grads[torch.float32][0])
    held_to(f"hashgrid + network, grid params.grad ({binding})", got_enc, grads[torch.float64][1].double(), grads[torch.float32][1])


def test_a_16_bit_network_still_refuses(binding):
    T = tcnn()
    net = T.Network(IN, OUT, dict(CFG, otype="FullyFusedMLP", activation="ReLU"), seed=11)
    x = torch.rand((256, IN), device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="not implemented"):
        eikonal(net(x), x).backward()

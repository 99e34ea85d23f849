"""max_level and the per-sample max_level array of the grid encoding on the GPU, against the oracle with the off (sample, level) blocks masked
(tests/max_level_reference.py): features and dy_dx-based input gradients bit for bit, parameter and second-order gradients within the bars
tests/test_gpu_parity.py states for the same passes (restated at each assert).

n = 512: two granules of 256 -- one tile of the tiled gather (512 samples) whose waves meet different fates, two workgroups of the
reference-form kernels' 256 threads.  A D = 3, F = 2 hash grid with 8 levels and T = 2^12 (dense and hashed levels) and a D = 2, F = 4 dense
grid with 4 levels and Smoothstep.  Arrays: a constant (must equal the scalar), samples 0-255 coarse and 256-511 full (whole waves off for
the upper levels), and lanes interleaved from {2/8, 5/8, 1.0}."""
import numpy as np
import pytest
import torch

import max_level_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 512
HASH3D = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}
DENSE2D = {"otype": "DenseGrid", "n_levels": 4, "n_features_per_level": 4, "base_resolution": 8, "per_level_scale": 2.0, "interpolation": "Smoothstep"}
GRIDS = {
    "hash3d": (3, HASH3D, lambda: O.grid_init(3, 8, 2, 12, 4, 1.5, O.GRID_HASH, O.INTERP_LINEAR)),
    "dense2d": (2, DENSE2D, lambda: O.grid_init(2, 4, 4, 19, 8, 2.0, O.GRID_DENSE, O.INTERP_SMOOTHSTEP)),
}
MLP_64x2 = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}


def tcnn():
    import tinycudann
    return tinycudann


def h_np(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def rae(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (0.5 * (np.abs(a) + np.abs(b)) + np.abs(b).mean() * 1e-2 + 1e-12)

MARGINS = {"fractional": 1e-2}  # t = 2.4 / 1.2: no integer, the full margin holds (tests/max_level_reference.py)


def patterns(n):
    """name -> (scalar, array or None)"""
    coarse = np.where(np.arange(n) < n // 2, 2.0 / 8.0, 1.0).astype(np.float32)
    lanes = np.array([2.0 / 8.0, 5.0 / 8.0, 1.0], np.float32)[np.arange(n) % 3]
    return {"scalar": (0.5, None), "fractional": (0.3, None), "constant": (1.0, np.full(n, 0.5, np.float32)), "half-coarse": (1.0, coarse), "interleaved": (0.25, lanes)}


@pytest.fixture(scope="module", params=list(GRIDS))
def case(request):
    """inputs and nothing else: computed once per grid, never written to"""
    d, cfg, make = GRIDS[request.param]
    og = make()
    pos = O.generate_random_uniform(O.pcg32(41), N * d, 0.0, 1.0).reshape(N, d)
    r = np.random.default_rng(41)
    K = og.n_levels * og.n_features_per_level
    params = O.f2h((r.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    dy = O.f2h(r.standard_normal((N, K)).astype(np.float32))
    ddx = (r.standard_normal((N, d)) * 1e-2).astype(np.float32)
    return d, cfg, og, pos, params, dy, ddx


def _module(case, dtype, scalar, array):
    d, cfg, og, pos, params, dy, ddx = case
    m = tcnn().Encoding(d, cfg, dtype=dtype)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(O.h2f(params)))
    m.max_level = scalar
    m.set_max_level_gpu(None if array is None else torch.from_numpy(array).cuda())
    return m


def _passes(m, case):
    """forward, backward and double backward through torch.autograd.grad -> y, dL_dinput, dL_dparams, and the second-order d/dparams, d/dinput"""
    d, cfg, og, pos, params, dy, ddx = case
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    w = torch.from_numpy(O.h2f(dy)).cuda()
    y = m(x)
    gx, gp = torch.autograd.grad((y.float() * w).sum(), [x, m.params], create_graph=True)
    d_p, d_x = torch.autograd.grad((gx * torch.from_numpy(ddx).cuda()).sum(), [m.params, x])
    torch.cuda.synchronize()
    return y.detach(), gx.detach(), gp.detach(), d_p.detach(), d_x.detach()


@pytest.mark.parametrize("pattern", ["scalar", "fractional", "constant", "half-coarse", "interleaved"])
def test_encoding_fp16_against_the_masked_oracle(case, pattern, binding):
    d, cfg, og, pos, params, dy, ddx = case
    scalar, array = patterns(N)[pattern]
    L, F = og.n_levels, og.n_features_per_level
    off = R.off_mask(array if array is not None else scalar, N, L, F, margin=MARGINS.get(pattern, R.MARGIN))
    assert off.any() and not off.all()
    m = _module(case, torch.half, scalar, array)
    S = m.loss_scale  # the module multiplies dL/dy by it on the way down and divides the gradients on the way up (modules.py)
    y, gx, gp, d_p, d_x = _passes(m, case)
    want, dy_dx = R.forward(og, params, pos, off)
    assert np.array_equal(h_np(y), want)
    dy_s = O.f2h(O.h2f(dy) * S)  # (exact: a power of two, far from the format's ends)
    ref, absacc = R.backward(og, pos, dy_s, off)
    got = gp.cpu().numpy().astype(np.float64) * S
    # tests/test_gpu_parity.py::test_grid_backward_and_input_gradient, the default (bucketed) mode
    assert np.all(np.abs(got - ref) <= absacc * 2.0 ** -8 + 2e-3)
    assert not got[absacc == 0].any() and np.abs(ref).max() > 0
    dref = O.grid_backward_input(og, dy_s, dy_dx) / S
    assert np.allclose(gx.cpu().numpy(), dref, rtol=1e-4, atol=1e-3 * np.abs(dref).max())
    # second order: tests/test_gpu_parity.py::test_grid_second_order_through_c_abi_and_double_backward (the bucketed scatter takes every level here)
    gp_ref, mag, _, dx_ref = R.backward_backward(og, params, pos, ddx, dy_s, off)
    assert np.allclose(d_x.cpu().numpy() * S, dx_ref, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(dx_ref).max()))
    got2 = d_p.cpu().numpy().astype(np.float64) * S
    assert np.all(np.abs(got2 - gp_ref) <= 2.0 ** -8 * mag + 1e-3 * max(1.0, np.abs(gp_ref).max()))
    assert not got2[mag == 0].any()
    assert np.abs(gp_ref).max() > 0 and np.abs(dx_ref).max() > 0


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    C = tcnn()._C
    if request.param == "compiled" and C.EXT is None:
        pytest.skip("the compiled binding is not built")
    if request.param == "ctypes":
        monkeypatch.setattr(C, "EXT", None)
    return request.param


def test_constant_array_equals_the_scalar_and_clearing_restores_the_unset_bits(case):
    """a constant array against the scalar of the same value: every output bit for bit; then the array cleared and the scalar back at 1.0
    against a module nothing was ever set on"""
    d, cfg, og, pos, params, dy, ddx = case
    by_scalar = _passes(_module(case, torch.half, 0.5, None), case)
    m = _module(case, torch.half, 1.0, np.full(N, 0.5, np.float32))
    by_array = _passes(m, case)
    names = ["y", "dL_dinput", "dL_dparams", "second-order dL_dparams", "second-order dL_dinput"]
    for name, a, b in zip(names, by_scalar, by_array):
        assert torch.equal(a, b), name
    untouched = _passes(_module(case, torch.half, 1.0, None), case)
    assert not torch.equal(untouched[0], by_array[0])
    m.set_max_level_gpu(None)
    m.max_level = 1.0
    for name, a, b in zip(names, untouched, _passes(m, case)):
        assert torch.equal(a, b), name
    assert np.array_equal(h_np(untouched[0]), O.grid_forward(og, params, pos))


def test_a_pending_backward_reads_what_its_forward_read(case):
    """the values travel in the forward context: changing them between forward and backward changes nothing for that graph"""
    d, cfg, og, pos, params, dy, ddx = case
    _, array = patterns(N)["interleaved"]
    want = _passes(_module(case, torch.half, 1.0, array), case)
    m = _module(case, torch.half, 1.0, array)
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    m.set_max_level_gpu(None)
    m.max_level = 0.25
    gx, gp = torch.autograd.grad((y.float() * torch.from_numpy(O.h2f(dy)).cuda()).sum(), [x, m.params])
    assert torch.equal(gx, want[1]) and torch.equal(gp, want[2])


@pytest.mark.parametrize("pattern", ["scalar", "interleaved"])
def test_encoding_fp32_against_the_masked_oracle(case, pattern):
    """Encoding(dtype=float32): forward and the dy_dx-based input gradient bit for bit, parameter gradients within the rounding of a running
    fp32 sum (tests/test_gpu_parity.py::test_fp32_encoding_module)"""
    d, cfg, og, pos, params, dy, ddx = case
    scalar, array = patterns(N)[pattern]
    L, F = og.n_levels, og.n_features_per_level
    off = R.off_mask(array if array is not None else scalar, N, L, F, margin=MARGINS.get(pattern, R.MARGIN))
    m = tcnn().Encoding(d, cfg, dtype=torch.float32)
    p32 = (np.random.default_rng(4).standard_normal(og.n_params) * 0.3).astype(np.float32)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(p32))
    m.max_level = scalar
    m.set_max_level_gpu(None if array is None else torch.from_numpy(array).cuda())
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    want, dy_dx = R.forward_f32(og, p32, pos, off)
    assert np.array_equal(y.detach().cpu().numpy().view(np.uint32), want.view(np.uint32))
    w = O.h2f(dy)
    gx, gp = torch.autograd.grad((y * torch.from_numpy(w).cuda()).sum(), [x, m.params])
    ref, mag = R.backward_f32(og, pos, w, off)
    idx = O.grid_indices(og, pos)
    hits = np.zeros(og.n_params // F, np.int64)
    for l in range(L):
        np.add.at(hits, og.offsets[l] + idx[~off[:, l], l, :].reshape(-1), 1)
    hits = np.repeat(hits, F)
    g = gp.cpu().numpy()
    assert np.all(np.abs(g - ref) <= np.maximum(hits, 1) * 2.0 ** -24 * mag * 1.001)
    assert not g[hits == 0].any()
    assert np.array_equal(gx.cpu().numpy(), O.grid_backward_input_f32(og, R.masked(w, R.feature_mask(off, F)), dy_dx))


@pytest.mark.parametrize("pattern", ["scalar", "interleaved"])
def test_encoding_fp32_double_backward_against_the_masked_oracle(case, pattern):
    """Encoding(dtype=float32), double backward through torch.autograd.grad.  The second-order pass of an fp32 module runs the 16-bit
    kernels on stand-ins of the caller's tensors (api_module.hip): the parameters rounded to 16 bits -- exact here, the test's parameters
    are 16-bit numbers --, dL_doutput multiplied by the largest power of two s <= 1024 with max |dL_doutput| * s <= 16384 and the results
    divided by s again.  So the expected values are the masked oracle's on dL_dy * s, divided by s, under the bars of the 16-bit pass
    (tests/test_gpu_parity.py::test_grid_second_order_through_c_abi_and_double_backward); max_level and the array come from the forward
    context, as in the 16-bit module."""
    d, cfg, og, pos, params, dy, ddx = case
    scalar, array = patterns(N)[pattern]
    L, F = og.n_levels, og.n_features_per_level
    off = R.off_mask(array if array is not None else scalar, N, L, F)
    m = _module(case, torch.float32, scalar, array)
    S = m.loss_scale
    y, gx, gp, d_p, d_x = _passes(m, case)
    want, _ = R.forward_f32(og, O.h2f(params), pos, off)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want.view(np.uint32))
    w = O.h2f(dy) * np.float32(S)
    s = min(1024.0, 2.0 ** np.floor(np.log2(16384.0 / np.abs(w).max())))
    dy_s = O.f2h(w * np.float32(s))
    assert np.array_equal(O.h2f(dy_s), w * np.float32(s))  # the scaling is exact
    gp_ref, mag, _, dx_ref = R.backward_backward(og, params, pos, ddx, dy_s, off)
    gp_ref, mag, dx_ref = gp_ref / s, mag / s, dx_ref / np.float32(s)
    assert np.allclose(d_x.cpu().numpy() * S, dx_ref, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(dx_ref).max()))
    got2 = d_p.cpu().numpy().astype(np.float64) * S
    print(f"fp32 second-order parameter gradient: max |got - ref| / bound = {np.max(np.abs(got2 - gp_ref) / (2.0 ** -8 * mag + 1e-3 * max(1.0, np.abs(gp_ref).max()))):.4f}, s = {s}, S = {S}")
    assert np.all(np.abs(got2 - gp_ref) <= 2.0 ** -8 * mag + 1e-3 * max(1.0, np.abs(gp_ref).max()))
    assert not got2[mag == 0].any()
    assert np.abs(gp_ref).max() > 0 and np.abs(dx_ref).max() > 0


def _config():
    return {"loss": {"otype": "RelativeL2"},
            "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6},
            "encoding": HASH3D, "network": MLP_64x2}


def _targets(pos, out):
    return np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c + 1) * pos[:, 0]) * np.cos(2 * np.pi * pos[:, 1]) for c in range(out)], 1).astype(np.float32)


def _trainer(seed=1337):
    tm = tcnn().create_from_config(3, 4, _config(), seed=seed)
    w = tm.params_full_precision.cpu().numpy().copy()
    w[tm.n_mlp_params:] *= 1.0e3  # lift the U(-1e-4, 1e-4) grid init out of the fp16 subnormal range
    tm.set_params_full_precision(torch.from_numpy(w))
    return tm, w


def test_training_step_with_an_interleaved_array():
    """One training_step of a grid + 64x2 network.  oracle.training_step takes no masked encoding, so the step is compared piecewise, as
    tests/test_gpu_parity.py::test_network_with_input_encoding and ::test_training_step_matches_oracle do: the masked oracle encoding ->
    oracle network forward -> loss -> network backward -> masked dL/d(encoding) -> oracle grid scatter, each with the bar stated there.
    Grid gradient entries that only off (sample, level) pairs touch must be exactly zero."""
    tm, w = _trainer()
    og = GRIDS["hash3d"][2]()
    md = O.model_init(3, 4, og, 64, 2, O.LOSS_RELATIVE_L2)
    nm = md.mlp.n_params
    assert nm == tm.n_mlp_params
    pos = O.generate_random_uniform(O.pcg32(43), N * 3, 0.0, 1.0).reshape(N, 3)
    tgt = _targets(pos, 4)
    _, array = patterns(N)["interleaved"]
    off = R.off_mask(array, N, 8, 2)
    keep = torch.from_numpy(array).cuda()
    tm.set_max_level_gpu(keep)
    assert tm.max_level == 1.0
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    ctx = tm.training_step(x, t, run_optimizer=False)
    torch.cuda.synchronize()
    ph = O.f2h(w)
    enc_ref, _ = R.forward(og, ph[nm:], pos, off, out_stride=md.mlp.in_width)
    hid_ref, out_ref = O.mlp_forward(md.mlp, ph[:nm], enc_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(out_ref)), 99) < 3e-3
    _, g_ref = O.loss(md.loss_type, h_np(ctx.output), tgt, 4)
    assert np.array_equal(h_np(ctx.dL_doutput), g_ref)  # loss gradient: bit-exact on the GPU's own prediction
    _, g_out = O.loss(md.loss_type, out_ref, tgt, 4)
    gref, denc = O.mlp_backward(md.mlp, ph[:nm], enc_ref, hid_ref, out_ref, g_out)
    g = tm.param_gradients.float().cpu().numpy()
    assert np.percentile(rae(g[:nm], gref), 99) < 5e-3
    ggrid, absacc = R.backward(og, pos, denc, off)
    assert np.all(np.abs(g[nm:] - ggrid) <= absacc * 2.0 ** -7 + 1e-3 * np.abs(ggrid).max())
    assert not g[nm:][absacc == 0].any() and np.abs(ggrid).max() > 0
    # forward / backward as two calls, and inference, see the same values
    c2 = tm.forward(x, t)
    assert torch.equal(c2.output.view(torch.int16), ctx.output.view(torch.int16))
    out = tm.inference(x).cpu().numpy()
    assert np.percentile(np.abs(out - O.h2f(out_ref)[:, :4]), 99) < 5e-2
    tm.set_max_level_gpu(None)
    assert not torch.equal(tm.training_step(x, t, run_optimizer=False).output.view(torch.int16), ctx.output.view(torch.int16))


def test_graph_capture_follows_every_change():
    """With graph capture on: nothing set, the scalar at 0.5, back at 1.0, then the array, then cleared again.  The trainer counts the
    changes of either value and the count is part of a step's shape, so the first step after a change runs plainly and the next is a graph
    launch again (re-recording alone would also carry new values into the graph; the counter keeps the changed step out of it).  Every step equals the same step of a model that never captures, from the same state: prediction, loss,
    network gradients and weights bit for bit, the grid's gradients within the run-to-run spread of the coarse levels' packed-half atomics
    (tests/test_gpu_parity_full.py::test_training_step_as_one_graph_launch_leaves_the_plain_steps_bits, the same bars)."""
    a, _ = _trainer(seed=21)
    b, _ = _trainer(seed=22)
    nm = a.n_mlp_params
    _, array = patterns(N)["interleaved"]
    keep = torch.from_numpy(array).cuda()
    side = torch.cuda.Stream()
    a.set_graph_capture(True)
    settings = [(1.0, None), (1.0, None), (0.5, None), (0.5, None), (1.0, None), (1.0, keep), (1.0, keep), (1.0, None), (1.0, None)]
    plain = (0, 2, 4, 5, 7)  # the very first step (it fills the stream's scratch cache) and the first step after each change of either value
    with torch.cuda.stream(side):
        for step, (scalar, per_sample) in enumerate(settings):
            b.deserialize(a.serialize(serialize_optimizer=True))
            b.set_params_full_precision(a.params_full_precision.clone())
            for tm in (a, b):
                tm.max_level = scalar
                tm.set_max_level_gpu(per_sample)
            pos = O.generate_random_uniform(O.pcg32(500 + step), N * 3, 0.0, 1.0).reshape(N, 3)
            x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(_targets(pos, 4)).cuda()
            side.synchronize()
            launches = a.graph_capture_stats()[0]
            ca, cb = a.training_step(x, t), b.training_step(x, t)
            side.synchronize()
            assert a.graph_capture_stats()[0] - launches == (0 if step in plain else 1), step
            assert torch.equal(ca.output.view(torch.int16), cb.output.view(torch.int16)), step
            assert abs(a.loss(ca) - b.loss(cb)) <= 1e-6 * abs(b.loss(cb)), step
            ga, gb = a.param_gradients, b.param_gradients
            assert torch.equal(ga[:nm].view(torch.int16), gb[:nm].view(torch.int16)), step
            assert torch.equal(a.params[:nm].view(torch.int16), b.params[:nm].view(torch.int16)), step
            dgrid = (ga[nm:].float() - gb[nm:].float()).abs()
            assert float(dgrid.max()) <= 2.0 ** -8 * float(ga[nm:].float().abs().max()) and float((dgrid > 0).float().mean()) < 0.05, step
    assert b.graph_capture_stats() == (0, 0) and a.graph_capture_stats()[0] == len(settings) - len(plain)

"""The grid encodings on the GPU at positions OUTSIDE the unit cube and ON cell boundaries (tests/grid_domain_positions.py): cells that wrap
modulo 2^32 as the reference's pos_fract defines them (common_device.h:1016-1043).  The oracle is pinned to the reference's own kernels on
these positions (tests/test_oracle_ref.py), the kernel sources run on them under the host emulator (tests/test_emu_grid_domain.py); here
the compiled kernels run through the C ABI and the tinycudann modules, with the bars tests/test_gpu_parity.py states for the same passes
(restated at each assert).  n = 2048 forward, 4096 backward.

ENCODINGS of tests/test_gpu_parity.py plus SMALL_TABLE: F = 4 and T = 2^12, so the hashed levels (4096 entries) are ONE bucket of the
bucket-once backward (128 KiB / 32 B per entry) -- where the pair of a cell -1 stays together with tag 31 (grid_backward_plan.h)."""
import os

import numpy as np
import pytest
import torch

import grid_domain_positions as GD
from conftest import HASH_ENCODING, HASH_ENCODING_SMALL, config_hash
from oracle import oracle as O
from test_gpu_parity import ENCODINGS, oracle_grid

pytestmark = pytest.mark.gpu

SMALL_TABLE = (3, dict(HASH_ENCODING, n_levels=8, n_features_per_level=4, log2_hashmap_size=12, base_resolution=8, interpolation="Smoothstep"))
CASES = ENCODINGS + [SMALL_TABLE]
N_FWD, N_BWD = 2048, 4096
_cache = {}


def tcnn():
    import tinycudann
    return tinycudann


def h_np(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def h_t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.half).cuda()


def rae(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (0.5 * (np.abs(a) + np.abs(b)) + np.abs(b).mean() * 1e-2 + 1e-12)


def setup(d, enc, n, seed=43):
    """(oracle grid, positions): one draw per (encoding, n), shared and never written to"""
    key = (d, repr(sorted(enc.items())), n, seed)
    if key not in _cache:
        og = oracle_grid(enc, d)
        _cache[key] = (og, GD.for_grid(og, n, seed))  # (left writable: torch.from_numpy warns about read-only arrays)
    return _cache[key]


def hits_per_value(og, pos):
    F = og.n_features_per_level
    idx = O.grid_indices(og, pos)
    hits = np.zeros(og.n_params // F, np.int64)
    for l in range(og.n_levels):
        np.add.at(hits, og.offsets[l] + idx[:, l, :].reshape(-1), 1)
    return np.repeat(hits, F)


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    C = tcnn()._C
    if request.param == "compiled":
        assert C.EXT is not None, "the compiled binding is missing"
    else:
        monkeypatch.setattr(C, "EXT", None)
    return request.param


@pytest.mark.parametrize("d,enc", CASES)
def test_grid_indices_and_forward_bit_exact(d, enc):
    C = tcnn()._C
    m = C.create_encoding(d, enc)
    og, pos = setup(d, enc, N_FWD)
    assert m.n_params() == og.n_params
    x = torch.from_numpy(pos).cuda()
    assert np.array_equal(m.grid_indices(x).cpu().numpy().view(np.uint32), O.grid_indices(og, pos))
    params = O.f2h((np.random.default_rng(0).random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    _, y = m.fwd(x, h_t(params))
    torch.cuda.synchronize()
    assert np.array_equal(h_np(y), O.grid_forward(og, params, pos))


@pytest.mark.parametrize("d,enc", CASES)
def test_grid_backward_and_input_gradient(d, enc):
    """modes and bars of tests/test_gpu_parity.py::test_grid_backward_and_input_gradient"""
    C = tcnn()._C
    m = C.create_encoding(d, enc)
    og, pos = setup(d, enc, N_BWD)
    rng = np.random.default_rng(1)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    dy = O.f2h(rng.standard_normal((N_BWD, m.n_output_dims())).astype(np.float32))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    ref = O.grid_backward(og, pos, dy)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))))
    default_mode = C.get_grid_backward_mode()
    try:
        for mode in (0, 2, 3, 1):  # fp32 LDS slices, the reference's global atomics, bucket-once, packed-fp16 LDS slices
            if mode == 2 and enc.get("n_features_per_level", 2) == 1:
                continue
            C.set_grid_backward_mode(mode)
            dx, dp = m.bwd(ctx, x, p, y, h_t(dy))
            torch.cuda.synchronize()
            got = dp.float().cpu().numpy().astype(np.float64)
            err = np.abs(got - ref)
            print(f"mode {mode}: max |got - ref| / (absacc 2^-9 + 2e-3) = {np.max(err / (absacc * 2.0 ** -9 + 2e-3)):.3f}")
            assert np.all(err <= absacc * 2.0 ** (-9 if mode == 0 else -8) + 2e-3), f"grid backward mode {mode}"
            assert not got[absacc == 0].any(), f"grid backward mode {mode}"  # entries nothing was sent to stay exactly zero
    finally:
        C.set_grid_backward_mode(default_mode)
    if enc.get("interpolation", "Linear") != "Nearest":
        _, dy_dx = O.grid_forward(og, params, pos, want_dy_dx=True)
        dref = O.grid_backward_input(og, dy, dy_dx)
        assert np.allclose(dx.cpu().numpy(), dref, rtol=1e-4, atol=1e-3 * np.abs(dref).max())


@pytest.mark.parametrize("d,enc", [(3, dict(HASH_ENCODING, log2_hashmap_size=15, n_levels=8)),
                                   (2, {"otype": "DenseGrid", "n_levels": 4, "base_resolution": 8, "per_level_scale": 2.0, "interpolation": "Smoothstep"}),
                                   (3, dict(HASH_ENCODING, log2_hashmap_size=12, n_levels=6, n_features_per_level=1))])
def test_grid_stochastic_interpolation(d, enc):
    """cases and bars of tests/test_gpu_parity.py::test_grid_stochastic_interpolation"""
    C = tcnn()._C
    enc = dict(enc, stochastic_interpolation=True)
    m = C.create_encoding(d, enc)
    og, pos = setup(d, enc, N_BWD)
    n = N_BWD
    rng = np.random.default_rng(2)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    dy = O.f2h(rng.standard_normal((n, m.n_output_dims())).astype(np.float32))
    x = torch.from_numpy(pos).cuda()
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    assert np.array_equal(h_np(y), O.grid_forward(og, params, pos))
    _, dp = m.bwd(ctx, x, p, y, h_t(dy))
    got = dp.float().cpu().numpy().astype(np.float64)
    ref = O.grid_backward(og, pos, dy, stochastic_interpolation=True)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))), stochastic_interpolation=True)
    assert np.all(np.abs(got - ref) <= absacc * 2.0 ** -8 + 2e-3)
    assert not np.allclose(ref, O.grid_backward(og, pos, dy), atol=1e-2)  # not the interpolating scatter
    F = enc.get("n_features_per_level", 2)
    for level in range(og.n_levels):
        lo, hi = og.offsets[level] * F, og.offsets[level + 1] * F
        want = O.h2f(dy)[:, level * F:(level + 1) * F].astype(np.float64).sum()
        assert abs(got[lo:hi].sum() - want) <= 1e-2 * np.abs(O.h2f(dy)[:, level * F:(level + 1) * F]).sum() * 2.0 ** -6 + 0.5


def test_fp32_encoding_module(binding):
    """bars of tests/test_gpu_parity.py::test_fp32_encoding_module: features and the dy_dx-based input gradient bit for bit, parameter
    gradients within the rounding of a running fp32 sum (hits x 2^-24 x the sum of the magnitudes)"""
    T = tcnn()
    og, pos = setup(3, HASH_ENCODING_SMALL, N_FWD)
    enc_f = T.Encoding(3, HASH_ENCODING_SMALL, seed=5, dtype=torch.float32)
    rng = np.random.default_rng(2)
    params = (rng.standard_normal(og.n_params) * 0.3).astype(np.float32)
    with torch.no_grad():
        enc_f.params.copy_(torch.from_numpy(params))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = enc_f(x)
    want, dy_dx = O.grid_forward_f32(og, params, pos, want_dy_dx=True)
    assert y.dtype == torch.float32 and np.array_equal(y.detach().cpu().numpy().view(np.uint32), want.view(np.uint32))
    hits = hits_per_value(og, pos)
    for magnitude in (1.0e-3, 1.0e4):
        w = (rng.standard_normal((N_FWD, 32)) * magnitude).astype(np.float32)
        x.grad, enc_f.params.grad = None, None
        (enc_f(x) * torch.from_numpy(w).cuda()).sum().backward()
        g, dx = enc_f.params.grad.cpu().numpy(), x.grad.cpu().numpy()
        g_want, mag = O.grid_backward_f32(og, pos, w), O.grid_backward_f32(og, pos, np.abs(w))
        assert np.isfinite(g).all() and np.all(np.abs(g - g_want) <= np.maximum(hits, 1) * 2.0 ** -24 * mag * 1.001), magnitude
        assert not g[hits == 0].any() and np.array_equal(g[hits == 1], g_want[hits == 1].astype(np.float32))
        assert np.array_equal(dx, O.grid_backward_input_f32(og, w, dy_dx)), magnitude


@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
def test_grid_second_order_through_c_abi(interp):
    """the three native outputs of backward_backward_input against the oracle, as in
    tests/test_gpu_parity.py::test_grid_second_order_through_c_abi_and_double_backward"""
    C = tcnn()._C
    enc = dict(HASH_ENCODING_SMALL, interpolation=interp)
    d = 3
    m = C.create_encoding(d, enc)
    og, pos = setup(d, enc, N_FWD)
    n = N_FWD
    rng = np.random.default_rng(5)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    K = m.n_output_dims()
    dy = O.f2h(rng.standard_normal((n, K)).astype(np.float32))
    ddx = (rng.standard_normal((n, d)) * 1e-3).astype(np.float32)  # the finest level's scale is ~7e3: keep fp16 gradients in range
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    d_dy, d_p, d_x = m.bwd_bwd_input(ctx, x, p, torch.from_numpy(ddx).cuda(), h_t(dy).requires_grad_(True))
    torch.cuda.synchronize()
    _, dydx = O.grid_forward(og, params, pos, want_dy_dx=True)
    gp_ref, dLddy_ref, dx_ref = O.grid_backward_backward_input(og, params, pos, ddx, dy, dy_dx=dydx)
    KK = og.n_levels * og.n_features_per_level
    assert np.array_equal(h_np(d_dy)[:, :KK], dLddy_ref[:, :KK])
    assert np.allclose(d_x.cpu().numpy(), dx_ref, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(dx_ref).max()))
    mag = np.abs(O.grid_backward_backward_input(og, params, pos, np.abs(ddx), O.f2h(np.abs(O.h2f(dy))))[0]) + np.abs(gp_ref)
    assert np.abs(gp_ref).max() > 0
    assert np.all(np.abs(d_p.float().cpu().numpy().astype(np.float64) - gp_ref) <= 2.0 ** -8 * mag + 1e-3 * max(1.0, np.abs(gp_ref).max()))


def test_training_step_matches_oracle():
    """the fused step (k_grid_forward_tiles and the record scatter inside it) with run_optimizer=False against the oracle's whole-step
    restatement: bars of tests/test_gpu_parity.py::test_training_step_matches_oracle"""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=15, per_level_scale=1.5)
    tm = T.create_from_config(3, 4, cfg, seed=1337)
    og, pos = setup(3, cfg["encoding"], N_BWD, seed=21)
    md = O.model_init(3, 4, og, 64, 2, O.LOSS_RELATIVE_L2, O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=1e-6))
    init = tm.params_full_precision.cpu().numpy().copy()
    init[md.mlp.n_params:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))
    st = O.TrainState(md, init)
    tgt = np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c + 1) * pos[:, 0]) * np.cos(2 * np.pi * pos[:, 1]) for c in range(4)], 1).astype(np.float32)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-3 * abs(loss_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(pred_ref)), 99) < 3e-3
    _, g_ref = O.loss(md.loss_type, h_np(ctx.output), tgt, 4)
    assert np.array_equal(h_np(ctx.dL_doutput), g_ref)
    g = tm.param_gradients.float().cpu().numpy()
    gref = O.h2f(st.grads)
    nm = md.mlp.n_params
    assert np.percentile(rae(g[:nm], gref[:nm]), 99) < 5e-3
    big = np.abs(gref[nm:]) > 1e-2 * np.abs(gref[nm:]).max()
    assert big.sum() > 100 and np.percentile(rae(g[nm:][big], gref[nm:][big]), 99) < 3e-2


def test_encoding_module_pads_a_ragged_batch(binding):
    """tinycudann.Encoding with 1000 rows: the module pads to 1024.  The real rows come out as the oracle's bits, the parameter gradient
    is the oracle's on the 1000 rows (the default, bucketed mode's bar) and entries no real row touches stay exactly zero."""
    T = tcnn()
    n = 1000
    og, pos = setup(3, HASH_ENCODING_SMALL, n)
    m = T.Encoding(3, HASH_ENCODING_SMALL, dtype=torch.half)
    rng = np.random.default_rng(7)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(O.h2f(params)))
    S = m.loss_scale  # the module multiplies dL/dy by it on the way down and divides the gradients on the way up (modules.py)
    dy = O.f2h(rng.standard_normal((n, 32)).astype(np.float32))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = m(x)
    assert y.shape == (n, 32)
    want, dy_dx = O.grid_forward(og, params, pos, want_dy_dx=True)
    assert np.array_equal(h_np(y), want)
    gx, gp = torch.autograd.grad((y.float() * torch.from_numpy(O.h2f(dy)).cuda()).sum(), [x, m.params])
    dy_s = O.f2h(O.h2f(dy) * S)  # (exact: a power of two, far from the format's ends)
    ref = O.grid_backward(og, pos, dy_s)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy_s))))
    got = gp.cpu().numpy().astype(np.float64) * S
    assert np.all(np.abs(got - ref) <= absacc * 2.0 ** -8 + 2e-3)
    assert not got[absacc == 0].any() and np.abs(ref).max() > 0
    dref = O.grid_backward_input(og, dy_s, dy_dx) / S
    assert gx.shape == (n, 3) and np.allclose(gx.cpu().numpy(), dref, rtol=1e-4, atol=1e-3 * np.abs(dref).max())


def test_reference_domain_fixture():
    """tests/golden/reference_domain.npz -- THE REFERENCE'S OWN kernel_grid compiled for the host on 256 of these positions
    (tests/golden/make_ref_golden.py domain()): the HIP gather reproduces `encoded` bit for bit and dy_dx through one-hot dL_dy
    (kernel_grid_backward_input, grid.h:322-349), no oracle in the loop."""
    C = tcnn()._C
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_domain.npz"))
    pos = gold["positions"]
    assert np.mean((pos < 0) | (pos >= 1)) >= 0.5
    e = C.create_encoding(3, HASH_ENCODING_SMALL)
    u = C.Pcg32(int(gold["grid_seed"][0])).uniform_(torch.empty(e.n_params(), device="cuda"))
    grid = (2.0 * u - 1.0).half()  # exactly the fixture's fp32 arithmetic: 2u and 2u - 1 are single IEEE operations
    xg = torch.from_numpy(pos).cuda().requires_grad_(True)
    ctx, enc = e.fwd(xg, grid)
    assert np.array_equal(h_np(enc), gold["encoded"])
    rows = gold["dy_dx_first"].shape[0]
    for k in range(32):
        dy = torch.zeros_like(enc)
        dy[:, k] = 1.0
        dx, _ = e.bwd(ctx, xg, grid, enc, dy)
        assert np.array_equal(dx.cpu().numpy()[:rows], gold["dy_dx_first"][:, k, :]), k

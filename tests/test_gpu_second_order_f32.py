"""The second-order pass of an fp32 grid encoding on the GPU: tcnn.Encoding(dtype=torch.float32) differentiated twice with
torch.autograd.grad(..., create_graph=True), on both bindings, and once straight through tcnn_module_backward_backward_input, against the
numpy restatement (tests/grid_second_order_f32_reference.py).  Cases, inputs -- fp32 numbers that 16 bits cannot represent, dL_doutput at
magnitude 1, 1e4 and 1e-6 -- and the bars with their derivation: tests/second_order_f32_cases.py.  N = 512 and 768."""
import ctypes

import numpy as np
import pytest
import torch

import second_order_f32_cases as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def tcnn():
    import tinycudann
    return tinycudann


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    C = tcnn()._C
    if request.param == "compiled" and C.EXT is None:
        pytest.skip("the compiled binding is not built")
    if request.param == "ctypes":
        monkeypatch.setattr(C, "EXT", None)
    return request.param


@pytest.fixture
def mode1():
    C = tcnn()._C
    assert C.get_fp32_second_order() == 0
    try:
        C.set_fp32_second_order(1)
        yield
    finally:
        C.set_fp32_second_order(0)


def _module(case, params, scalar=1.0, array=None):
    m = tcnn().Encoding(case[0], K.config(*case), dtype=torch.float32)
    assert m.loss_scale == 1.0
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(params))
    m.max_level = scalar
    m.set_max_level_gpu(None if array is None else torch.from_numpy(array).cuda())
    return m


def _double_backward(m, pos, dy, ddx, after_forward=None):
    """-> second-order dL_dparams, dL_ddLdoutput, dL_dinput as numpy"""
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    w = torch.from_numpy(dy).cuda().requires_grad_(True)
    y = m(x)
    if after_forward:
        after_forward(m)
    gx, = torch.autograd.grad((y * w).sum(), [x], create_graph=True)
    d_p, d_y, d_x = torch.autograd.grad((gx * torch.from_numpy(ddx).cuda()).sum(), [m.params, w, x])
    torch.cuda.synchronize()
    return d_p.cpu().numpy(), d_y.cpu().numpy(), d_x.cpu().numpy()


@pytest.mark.parametrize("magnitude", K.MAGNITUDES)
@pytest.mark.parametrize("n", [512, 768])
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_double_backward_against_the_restatement(case, n, magnitude, binding):
    og = K.oracle_grid(*case)
    pos, params, dy, ddx = K.inputs(og, n, magnitude)
    ref, _ = K.expected(og, params, pos, ddx, dy)
    K.check(og, ref, *_double_backward(_module(case, params), pos, dy, ddx), label=f"{K.case_id(case)} n={n} x{magnitude:g} {binding}")


@pytest.mark.parametrize("pattern", ["scalar", "interleaved"])
@pytest.mark.parametrize("case", [(3, 2, "Smoothstep"), (2, 4, "Linear")], ids=K.case_id)
def test_max_level_as_the_forward_pass_saw_it(case, pattern, binding):
    """max_level (0.5) and a per-sample array (tests/test_gpu_max_level.py::patterns' "interleaved": lanes from {2/8, 5/8, 1}) are set
    before the forward pass and changed after it; the double backward must see what its forward saw"""
    n = 512
    og = K.oracle_grid(*case)
    from test_gpu_max_level import patterns
    scalar, array = patterns(n)[pattern]
    off = K.S.off_mask(array if array is not None else scalar, n, og.n_levels, og.n_features_per_level)
    assert off.any() and not off.all()
    pos, params, dy, ddx = K.inputs(og, n, 1.0)
    ref, _ = K.expected(og, params, pos, ddx, dy, off=off)

    def change(m):
        m.set_max_level_gpu(None)
        m.max_level = 1.0 if pattern == "scalar" else 0.75

    K.check(og, ref, *_double_backward(_module(case, params, scalar, array), pos, dy, ddx, after_forward=change), label=f"{K.case_id(case)} max_level {pattern} {binding}")


def _c_abi(case, params, pos, dy, ddx):
    """one call of tcnn_module_backward_backward_input on a module made with tcnn_create_encoding, through the ctypes classes"""
    C = tcnn()._C
    h = ctypes.c_void_p()
    C._check(C._lib.tcnn_create_encoding(case[0], C._dumps(K.config(*case)), int(C.Precision.Fp32), ctypes.byref(h)))
    m = C.Module(h.value)
    width = m.n_output_dims()
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    p = torch.from_numpy(params).cuda().requires_grad_(True)
    g = torch.zeros((pos.shape[0], width), device="cuda")
    g[:, : dy.shape[1]] = torch.from_numpy(dy).cuda()
    g.requires_grad_(True)
    ctx, _ = m.fwd(x, p)
    d_y, d_p, d_x = m.bwd_bwd_input(ctx, x, p, torch.from_numpy(ddx).cuda(), g)
    torch.cuda.synchronize()
    return d_p.cpu().numpy(), d_y.cpu().numpy(), d_x.cpu().numpy()


@pytest.mark.parametrize("case", [(3, 2, "Smoothstep"), (3, 1, "Linear")], ids=K.case_id)
def test_straight_through_the_c_abi(case):
    og = K.oracle_grid(*case)
    pos, params, dy, ddx = K.inputs(og, 768, 1e4)
    ref, _ = K.expected(og, params, pos, ddx, dy)
    K.check(og, ref, *_c_abi(case, params, pos, dy, ddx), label=f"{K.case_id(case)} C ABI")  # (columns beyond L*F, where the module pads, must be zero)


def _sixteen_bit_valued(og, n):
    pos, params, dy, ddx = K.inputs(og, n, 1.0)
    return pos, O.h2f(O.f2h(params)), O.h2f(O.f2h(dy)), ddx


def test_nearest_is_zero_and_equals_mode_1():
    """Nearest: dL_dinput all zeros; dL_dparams and dL_ddLdoutput bit-equal to mode 1's on the same 16-bit-valued inputs"""
    case = (3, 2, "Nearest")
    og = K.oracle_grid(*case)
    pos, params, dy, ddx = _sixteen_bit_valued(og, 512)
    C = tcnn()._C
    got = _double_backward(_module(case, params), pos, dy, ddx)
    try:
        C.set_fp32_second_order(1)
        want = _double_backward(_module(case, params), pos, dy, ddx)
    finally:
        C.set_fp32_second_order(0)
    assert not got[2].any()
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("pattern", ["scalar", "interleaved"])
def test_mode_1_on_16_bit_valued_inputs_is_the_former_pass(mode1, pattern):
    """set_fp32_second_order(1) on 16-bit-valued inputs: the expected values and bars of
    tests/test_gpu_max_level.py::test_encoding_fp32_double_backward_against_the_masked_oracle, on its grids, inputs and patterns"""
    import max_level_reference as R
    import test_gpu_max_level as T
    assert tcnn()._C.get_fp32_second_order() == 1
    for name in T.GRIDS:
        d, cfg, make = T.GRIDS[name]
        og = make()
        pos = O.generate_random_uniform(O.pcg32(41), T.N * d, 0.0, 1.0).reshape(T.N, d)
        r = np.random.default_rng(41)
        params = O.f2h((r.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
        dy = O.f2h(r.standard_normal((T.N, og.n_levels * og.n_features_per_level)).astype(np.float32))
        ddx = (r.standard_normal((T.N, d)) * 1e-2).astype(np.float32)
        case = (d, cfg, og, pos, params, dy, ddx)
        scalar, array = T.patterns(T.N)[pattern]
        off = R.off_mask(array if array is not None else scalar, T.N, og.n_levels, og.n_features_per_level)
        m = T._module(case, torch.float32, scalar, array)
        S = m.loss_scale
        y, gx, gp, d_p, d_x = T._passes(m, case)
        w = O.h2f(dy) * np.float32(S)
        s = min(1024.0, 2.0 ** np.floor(np.log2(16384.0 / np.abs(w).max())))
        dy_s = O.f2h(w * np.float32(s))
        assert np.array_equal(O.h2f(dy_s), w * np.float32(s))
        gp_ref, mag, _, dx_ref = R.backward_backward(og, params, pos, ddx, dy_s, off)
        gp_ref, mag, dx_ref = gp_ref / s, mag / s, dx_ref / np.float32(s)
        assert np.allclose(d_x.cpu().numpy() * S, dx_ref, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(dx_ref).max()))
        got2 = d_p.cpu().numpy().astype(np.float64) * S
        assert np.all(np.abs(got2 - gp_ref) <= 2.0 ** -8 * mag + 1e-3 * max(1.0, np.abs(gp_ref).max()))
        assert not got2[mag == 0].any()
        assert np.abs(gp_ref).max() > 0 and np.abs(dx_ref).max() > 0


def test_mode_1_misses_the_fp32_bars(mode1):
    """The 16-bit stand-ins on the unrepresentable inputs of (3, 2, Smoothstep) at magnitude 1: dL_dinput and dL_dparams EXCEED their fp32
    bars.  The emulator's 16-bit kernels on the same kind of inputs (tests/test_emu_second_order_f32.py, N = 256) exceed them 40.9 times
    (dL_dinput) and 2707.9 times (dL_dparams).  On the GPU (N = 512) mode 1 measured 48.7 times
    (dL_dinput) and 4661 times (dL_dparams).  Without the fp32 kernels there is no mode 0 to differ from this."""
    case = (3, 2, "Smoothstep")
    og = K.oracle_grid(*case)
    pos, params, dy, ddx = K.inputs(og, 512, 1.0)
    ref, _ = K.expected(og, params, pos, ddx, dy)
    d_p, d_y, d_x = _double_backward(_module(case, params), pos, dy, ddx)
    r = K.ratios(og, ref, d_p, d_y, d_x)
    print(f"mode 1, max |got - ref| / fp32 bar: {r}")
    assert r["dL_dinput"] > 1 and r["dL_dparams"] > 1


def test_the_switch_refuses_other_values():
    C = tcnn()._C
    with pytest.raises(RuntimeError):
        C.set_fp32_second_order(2)
    assert C.get_fp32_second_order() == 0

"""16-bit inputs of the network modules on the GPU: tcnn_module_{inference,forward,backward}_half_input against the fp32 entries on the
widened input, through the C ABI and through both Python bindings.  Everything is held to BITS: the Identity encoding in front of a bare
network (scale 1, offset 0) is exact on values the 16-bit type holds, so the encoded matrix -- and with it the output, the parameter
gradients and dL/d(encoded input) -- is the same matrix either way; identity_dL_dx rounds through the 16-bit type, so the fp32 dL_dinput
holds 16-bit values and narrowing it loses nothing.

Shapes: n = 256 (one tile of the pad kernels) and 768 (three); input widths 3 and 20 (padded to 16 / 32), 16 and 64 (nothing to pad: the
kernels only transpose); the fused networks at 16 x 1, 64 x 2, 128 x 2, the layer-by-layer ones at 256 x 2, at 64 x 2 with 144 outputs and
with a Sine activation.  The bfloat16 library runs the 64 x 2 cases in a process of its own (the pattern of tests/test_gpu_bf16.py)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = os.environ.get("TCNN_PRECISION") == "bf16"
SIZES = [256, 768]
WIDTHS = [3, 20, 16, 64]


def _net(otype, width, layers, activation="ReLU"):
    return {"otype": otype, "activation": activation, "output_activation": "None", "n_neurons": width, "n_hidden_layers": layers}


NETWORKS = {
    "fused-16x1": (_net("FullyFusedMLP", 16, 1), 4),
    "fused-64x2": (_net("FullyFusedMLP", 64, 2), 4),
    "fused-128x2": (_net("FullyFusedMLP", 128, 2), 4),
    "mlp-256x2": (_net("CutlassMLP", 256, 2), 4),
    "mlp-64x2-144-outputs": (_net("CutlassMLP", 64, 2), 144),
    "mlp-64x2-sine": (_net("CutlassMLP", 64, 2, "Sine"), 4),
}


def _C():
    import tinycudann
    return tinycudann._C


def _half():
    C = _C()
    return C.TORCH_DTYPE[C.preferred_precision()]


@pytest.fixture(params=["c-abi", "compiled", "ctypes"])
def route(request, monkeypatch):
    C = _C()
    assert C.library_path().endswith("libtcnn_hip_bf16.so" if BF16 else "libtcnn_hip.so")
    if request.param == "compiled":
        assert C.EXT is not None, "the compiled binding is not built"
    if request.param == "ctypes":
        monkeypatch.setattr(C, "EXT", None)
    return request.param


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _inputs(n, d, n_out_padded, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x_h = (torch.rand((n, d), device="cuda", generator=g) * 2 - 1).to(_half())  # drawn in fp32, rounded to the 16-bit type
    dy = torch.randn((n, n_out_padded), device="cuda", generator=g).to(_half())
    return x_h, dy


def _run_abi(m, x, params, dy, dx_out=None):
    """(inference output, forward output, dL_dparams, dL_dinput) through the C ABI: the *_half_input entries for a 16-bit x, the existing ones for fp32"""
    C = _C()
    L, s, p = C._lib, C._stream(), C._ptr
    half = x.dtype != torch.float32
    n = x.shape[0]
    y_inf = torch.empty((n, m.n_output_dims()), dtype=_half(), device="cuda")
    y = torch.empty_like(y_inf)
    dparams = torch.empty((m.n_params(),), dtype=_half(), device="cuda")
    dx = torch.empty_like(x) if dx_out is None else dx_out
    h = ctypes.c_void_p()
    inference, forward, backward = (L.tcnn_module_inference_half_input, L.tcnn_module_forward_half_input, L.tcnn_module_backward_half_input) if half else \
        (L.tcnn_module_inference, L.tcnn_module_forward, L.tcnn_module_backward)
    C._check(inference(m._h, s, n, p(x), p(y_inf), p(params)))
    C._check(forward(m._h, s, n, p(x), p(y), p(params), 1, ctypes.byref(h)))
    try:
        C._check(backward(m._h, s, h, n, p(dx), p(dy), p(dparams), p(x), p(y), p(params)))
    finally:
        L.tcnn_context_destroy(h)
    return y_inf, y, dparams, dx


def _run_binding(m, x, params, dy):
    with torch.no_grad():
        _, y_inf = m.fwd(x, params)
    xr, pr = x.detach().requires_grad_(True), params.detach().requires_grad_(True)
    ctx, y = m.fwd(xr, pr)
    dx, dparams = m.bwd(ctx, xr, pr, y, dy)
    return y_inf, y.detach(), dparams, dx


def _run(route, m, x, params, dy):
    return _run_abi(m, x, params, dy) if route == "c-abi" else _run_binding(m, x, params, dy)


def _check_against_fp32(route, m, x_h, params, dy, what):
    want_inf, want_y, want_dp, want_dx = _run(route, m, x_h.float(), params, dy)
    got_inf, got_y, got_dp, got_dx = _run(route, m, x_h, params, dy)
    assert _same_bits(got_inf, want_inf), f"{what}: inference output"  # (a)
    assert _same_bits(got_y, want_y), f"{what}: forward output"
    assert _same_bits(got_dp, want_dp), f"{what}: dL_dparams"  # (b)
    assert want_dx.dtype == torch.float32 and got_dx.dtype == _half()
    assert _same_bits(want_dx.to(_half()).float(), want_dx), f"{what}: the fp32 dL_dinput holds 16-bit values"  # (c)
    assert _same_bits(got_dx, want_dx.to(_half())), f"{what}: dL_dinput"
    assert bool(torch.isfinite(got_y.float()).all()) and float(got_dx.float().abs().max()) > 0.0  # (not vacuous)
    return got_inf, got_y, got_dp, got_dx


def _module(network, n_in, n_out, seed=11):
    C = _C()
    m = C.create_network(n_in, n_out, network)
    assert m.supports_half_input()
    params = m.initial_params(seed).to(_half())
    return m, params


@pytest.mark.parametrize("name", list(NETWORKS))
def test_bit_equal_to_the_fp32_entries(route, name):
    network, n_out = NETWORKS[name]
    for d in WIDTHS:
        m, params = _module(network, d, n_out)
        for n in SIZES:
            x_h, dy = _inputs(n, d, m.n_output_dims(), seed=1000 * d + n)
            _check_against_fp32(route, m, x_h, params, dy, f"{name} {d} inputs n={n}")
    torch.cuda.synchronize()


def test_abc_at_64x2_in_this_build(route):
    """(a) - (c) at 64 x 2 with whichever library this process loaded: the fp16 one here, the bfloat16 one in the child process below"""
    network, n_out = NETWORKS["fused-64x2"]
    for d in (20, 64):
        m, params = _module(network, d, n_out)
        x_h, dy = _inputs(256, d, m.n_output_dims(), seed=d)
        assert x_h.dtype == (torch.bfloat16 if BF16 else torch.float16)
        _check_against_fp32(route, m, x_h, params, dy, f"64x2 {d} inputs")
    torch.cuda.synchronize()


def test_misaligned_matrices(route):
    """(d) a 16-wide input (and, through the C ABI, its gradient) 8 bytes behind a 16-byte boundary: the kernels' 2-byte paths, same bits"""
    network, n_out = NETWORKS["fused-64x2"]
    m, params = _module(network, 16, n_out)
    for n in SIZES:
        x_h, dy = _inputs(n, 16, m.n_output_dims(), seed=n)
        big = torch.zeros((n * 16 + 8,), dtype=_half(), device="cuda")
        x_off = big[4:4 + n * 16].view(n, 16)
        x_off.copy_(x_h)
        assert x_off.is_contiguous() and x_off.data_ptr() % 16 == 8 and x_h.data_ptr() % 16 == 0
        aligned = _check_against_fp32(route, m, x_h, params, dy, f"aligned n={n}")
        if route == "c-abi":
            dx_big = torch.zeros((n * 16 + 8,), dtype=_half(), device="cuda")
            got = _run_abi(m, x_off, params, dy, dx_out=dx_big[4:4 + n * 16].view(n, 16))
            assert bool((dx_big[:4] == 0).all()) and bool((dx_big[-4:] == 0).all())  # nothing outside the matrix was written
        else:
            got = _run_binding(m, x_off, params, dy)
        for a, b, what in zip(got, aligned, ("inference output", "forward output", "dL_dparams", "dL_dinput")):
            assert _same_bits(a.contiguous(), b), what
    torch.cuda.synchronize()


def test_contexts_do_not_mix():
    """a context of forward_half_input goes to backward_half_input, one of forward to backward: the other pairing is TCNN_ERROR with a message"""
    C = _C()
    L, s, p = C._lib, C._stream(), C._ptr
    m, params = _module(NETWORKS["fused-64x2"][0], 16, 4)
    x_h, dy = _inputs(256, 16, m.n_output_dims(), seed=3)
    x_f = x_h.float()
    y = torch.empty((256, m.n_output_dims()), dtype=_half(), device="cuda")
    dp = torch.empty((m.n_params(),), dtype=_half(), device="cuda")
    h16, h32 = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.tcnn_module_forward_half_input(m._h, s, 256, p(x_h), p(y), p(params), 1, ctypes.byref(h16)) == 0
    assert L.tcnn_module_forward(m._h, s, 256, p(x_f), p(y), p(params), 1, ctypes.byref(h32)) == 0
    try:
        dx_f, dx_h = torch.empty_like(x_f), torch.empty_like(x_h)
        assert L.tcnn_module_backward(m._h, s, h16, 256, p(dx_f), p(dy), p(dp), p(x_f), p(y), p(params)) == 1
        assert b"tcnn_module_backward_half_input" in L.tcnn_last_error()
        assert L.tcnn_module_backward_half_input(m._h, s, h32, 256, p(dx_h), p(dy), p(dp), p(x_h), p(y), p(params)) == 1
        assert b"tcnn_module_forward" in L.tcnn_last_error()
        assert L.tcnn_module_backward_half_input(m._h, s, h16, 256, p(dx_h), p(dy), p(dp), None, p(y), p(params)) == 0  # (`input` is not read)
        assert L.tcnn_module_backward(m._h, s, h32, 256, p(dx_f), p(dy), p(dp), p(x_f), p(y), p(params)) == 0
        assert _same_bits(dx_h, dx_f.to(_half()))
    finally:
        L.tcnn_context_destroy(h16)
        L.tcnn_context_destroy(h32)
    torch.cuda.synchronize()


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    C = _C()
    if request.param == "compiled":
        assert C.EXT is not None, "the compiled binding is not built"
    else:
        monkeypatch.setattr(C, "EXT", None)
    return request.param


@pytest.mark.parametrize("create_graph", [False, True], ids=["plain", "create_graph"])
def test_encoding_into_network_keeps_16_bits(binding, create_graph):
    """(e) Encoding(Frequency) -> Network with the 16-bit tensor in between, against the same chain with .float() in between: same output, same
    parameter and input gradients, bit for bit; 300 rows, so the modules pad the batch.  The network is handed a 16-bit tensor and returns
    a 16-bit gradient for it."""
    import tinycudann as T
    enc = T.Encoding(3, {"otype": "Frequency", "n_frequencies": 4})
    net = T.Network(enc.n_output_dims, 4, NETWORKS["fused-64x2"][0])
    assert type(net.native_tcnn_module).__name__ == ("ExtModule" if binding == "compiled" else "Module")
    assert net.native_tcnn_module.supports_half_input() and not enc.native_tcnn_module.supports_half_input()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((300, 3), device="cuda", generator=g)
    w = torch.randn((300, 4), device="cuda", generator=g)
    seen = {}

    def chain(widen):
        xr = x.clone().requires_grad_(True)
        h = enc(xr)
        assert h.dtype == _half()
        h.register_hook(lambda grad: seen.__setitem__(widen, grad.dtype))
        y = net(h.float() if widen else h)
        loss = (y.float() * w).sum()
        dparams, dx = torch.autograd.grad(loss, [net.params, xr], create_graph=create_graph)
        return y.detach(), dparams.detach(), dx.detach()

    want, got = chain(True), chain(False)
    assert seen == {True: _half(), False: _half()}
    for a, b, what in zip(got, want, ("output", "parameter gradients", "input gradients")):
        assert _same_bits(a, b), what
    assert float(got[1].abs().max()) > 0.0 and float(got[2].abs().max()) > 0.0
    # the native module saw the 16-bit tensor itself, and answers with a 16-bit gradient
    hr = enc(x).detach().requires_grad_(True)
    pr = net.params.detach().to(net.dtype).requires_grad_(True)
    pad = torch.nn.functional.pad(hr, [0, 0, 0, 212])
    ctx, y = net.native_tcnn_module.fwd(pad, pr)
    dx, _ = net.native_tcnn_module.bwd(ctx, pad, pr, y, torch.ones_like(y))
    assert dx.dtype == _half() and dx.shape == pad.shape
    torch.cuda.synchronize()


def test_bf16_build_passes_the_64x2_cases():
    assert not BF16  # (the bf16 run selects test_abc_at_64x2_in_this_build alone)
    env = dict(os.environ, TCNN_PRECISION="bf16")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "--tb=short",
                        "-k", "test_abc_at_64x2_in_this_build"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "3 passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout.split("\n")[-2], tail

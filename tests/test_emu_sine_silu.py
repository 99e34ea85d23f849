"""Sine and SiLU hidden activations of the layer-by-layer network (tiny-cuda-nn_amd/csrc/mlp_general.hip) on the host SIMT emulator: the
real kernel source -- the epilogue that stores the rounded pre-activation next to the post-activation, and the backward epilogue that
takes the derivative at it -- against the numpy restatement of tests/sine_silu_reference.py.

The saved stack of such a network is [H][n][W] post-activations followed by [H][n][W] pre-activations (mlp_saved_activation_bytes), so
this file drives the emulator's emu_mlp_forward / emu_mlp_backward entry points itself with a buffer of that size.

Bars: those of tests/test_emu_mlp_general.py -- RAE p99 < 3e-3 (stacks, output, weight gradients), weight gradients p99.9 < 1.2e-2,
dL/dinput within rtol 2e-2, atol 2e-3 max|ref|; bfloat16 3e-2 / relative L2 2e-2.  tests/test_library_sine_silu.py asserts that the
restatement's two accumulation orders agree within half of each on these very cases."""
import ctypes as C

import numpy as np
import pytest

import sine_silu_reference as S
from oracle import oracle as O

emu = pytest.importorskip("emu")
if not emu.available():
    pytest.skip("ROCm clang++ not available to build the host emulator", allow_module_level=True)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def meta(c):
    IN, W, OUT, H = c.shape
    return emu.EmuMlp(IN, W, c.OUTP, H - 1, c.act, O.ACT_NONE)


def forward(c, save_hidden=True):
    """-> (post [H][n][W], pre [H][n][W], out [n][OUTP]); the stack is pre-filled with a pattern no result has (0x7E00, a NaN)"""
    IN, W, OUT, H = c.shape
    stack = np.full((2, H, c.n, W), 0x7E00, dtype=np.uint16) if save_hidden else None
    out = np.zeros((c.n, c.OUTP), dtype=np.uint16)
    m = meta(c)
    assert emu.lib().emu_mlp_forward(C.byref(m), C.c_uint32(c.n), _p(c.ph), _p(c.xs), _p(stack), _p(out)) == 0
    return (stack[0], stack[1], out) if save_hidden else (None, None, out)


def backward(c, post, pre, want_dinput=True, want_grads=True):
    IN, W, OUT, H = c.shape
    stack = np.ascontiguousarray(np.stack([post, pre]))
    dinput = np.zeros((IN, c.n), dtype=np.uint16) if want_dinput else None
    grads = np.zeros(S.n_params(*c.shape), dtype=np.uint16) if want_grads else None
    m = meta(c)
    assert emu.lib().emu_mlp_backward(C.byref(m), C.c_uint32(c.n), _p(c.ph), _p(c.xs), _p(stack), _p(c.dy), _p(dinput), _p(grads), C.c_int(0), None) == 0
    return grads, (None if dinput is None else np.ascontiguousarray(dinput.T))


@pytest.mark.parametrize("act", [S.ACT_SINE, S.ACT_SILU], ids=["Sine", "SiLU"])
@pytest.mark.parametrize("shape", S.CASES, ids=[str(c) for c in S.CASES])
def test_forward_backward(act, shape):
    c = S.case(act, shape)
    post, pre, out = forward(c)
    assert not np.any(post == 0x7E00) and not np.any(pre == 0x7E00)  # every element of both blocks was written
    _, _, out_inf = forward(c, save_hidden=False)
    assert np.array_equal(out_inf, out)  # inference (ping-pong buffers, no pre-activation store) == forward, bit for bit
    # layer by layer on shared stacks (sine_silu_reference.py): every layer's reference from this side's stored activations below it, the
    # backward pass of both sides on the restatement's stacks
    gh, dx = backward(c, c.post_ref, c.pre_ref)
    S.check(dict(post=post, pre=pre, out=out), S.forward_on(act, c.shape, c.ph, c.x, pre, post), S.BARS_FP16, label=f"emu forward {S.NAMES[act]} {shape}")
    S.check(dict(g=gh, dx=dx), c.ref["f64"], S.BARS_FP16, label=f"emu backward {S.NAMES[act]} {shape}")
    # and the chain as a whole stays near the restatement's own: a wrong layer input would show here, not above
    assert np.percentile(S.rae(O.h2f(out), O.h2f(c.out_ref)), 90) < 3e-3


def test_post_activation_is_the_activation_of_the_stored_pre_activation():
    """post = R(sin(pre)) on the ROUNDED pre-activation this side stored: bit for bit up to the last place of the fp32 sine"""
    c = S.case(S.ACT_SINE, S.CASES[0])
    post, pre, _ = forward(c)
    again = O.h2f(O.f2h(np.sin(O.h2f(pre))))
    assert np.mean(post != O.f2h(again)) < 1e-3 and np.max(np.abs(O.h2f(post) - again)) <= 2.0 ** -10


def test_without_input_gradient_and_without_weight_gradients():
    c = S.case(S.ACT_SILU, S.CASES[0])
    gh, dx = backward(c, c.post_ref, c.pre_ref)
    g_only, no_dx = backward(c, c.post_ref, c.pre_ref, want_dinput=False)
    assert no_dx is None and np.array_equal(g_only, gh)
    no_g, dx_only = backward(c, c.post_ref, c.pre_ref, want_grads=False)
    assert no_g is None and np.array_equal(dx_only, dx)


def test_output_activation_that_needs_the_pre_activation_is_refused(capfd):
    c = S.case(S.ACT_SINE, S.CASES[0])
    m = meta(c)
    m.output_activation = S.ACT_SINE
    out = np.zeros((c.n, c.OUTP), dtype=np.uint16)
    assert emu.lib().emu_mlp_forward(C.byref(m), C.c_uint32(c.n), _p(c.ph), _p(c.xs), None, _p(out)) == 1
    assert "output activation" in capfd.readouterr().err


@pytest.fixture()
def bf16():
    """The oracle's 16-bit format is a process-wide switch and emu.py calls one library at a time: both to bfloat16, restored on the way out."""
    O.set_half_format(True)
    previous = emu.set_bf16(True)
    yield
    emu.set_bf16(previous)
    O.set_half_format(False)


@pytest.mark.parametrize("act", [S.ACT_SINE, S.ACT_SILU], ids=["Sine", "SiLU"])
def test_bfloat16_build(bf16, act):
    c = S.case(act, S.CASES[1], bf16=True)
    S.band(c, S.BARS_BF16)  # the half-bar condition, evaluated in bfloat16
    post, pre, out = forward(c)
    _, _, out_inf = forward(c, save_hidden=False)
    assert np.array_equal(out_inf, out)
    gh, dx = backward(c, c.post_ref, c.pre_ref)
    S.check(dict(post=post, pre=pre, out=out), S.forward_on(act, c.shape, c.ph, c.x, pre, post), S.BARS_BF16, label=f"emu bf16 forward {S.NAMES[act]}")
    S.check(dict(g=gh, dx=dx), c.ref["f64"], S.BARS_BF16, label=f"emu bf16 backward {S.NAMES[act]}")

"""The layer-by-layer network of the widths outside 16/32/64/128 (tiny-cuda-nn_amd/csrc/mlp_general.hip: the reference's CutlassMLP) on the
host SIMT emulator against the CPU oracle.  The kernels sit behind the launchers the emulator driver already calls (mlp_forward,
mlp_backward, mlp_backward_n_partials, mlp_backward_workspace_bytes, mlp_finalize_gradients), so this runs the real kernel source: tile and
fragment bookkeeping, the two-stage K pipeline, the transpose reads and the slab layout of the weight-gradient slices (the driver fills the
slabs with a sentinel: an element no slice wrote shows in the sums).

fp16 bars: the GPU suite's own (tests/test_gpu_parity.py test_network_forward_backward) -- output RAE p99 < 3e-3, weight gradients RAE
p99 < 3e-3 and p99.9 < 1.2e-2, dL/dinput within rtol 2e-2, atol 2e-3 max|ref|.  bfloat16: outputs RAE p99 < 3e-2, weight gradients
relative L2 < 2e-2 (tests/bf16_cases.py, tests/test_emu_bf16.py)."""
import numpy as np
import pytest

from oracle import oracle as O

emu = pytest.importorskip("emu")
if not emu.available():
    pytest.skip("ROCm clang++ not available to build the host emulator", allow_module_level=True)


def rae(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (0.5 * (np.abs(a) + np.abs(b)) + np.abs(b).mean() * 1e-2 + 1e-12)


# IN, W, OUT, hidden layers, n
CASES = [
    (16, 48, 16, 1, 256),   # three blocks of 16 neurons, not a power of two
    (80, 80, 48, 3, 768),   # input wider than a fused tile, more than 16 outputs, 12 sample stages over 8 batch slices (uneven)
    (32, 272, 16, 2, 256),  # more than one workgroup tile of neurons, K longer than one LDS stage
]


class Setup:
    def __init__(self, case, activation=O.ACT_RELU, output_activation=O.ACT_NONE, scale=1.0, seed=2):
        IN, W, OUT, H, n = case
        rng = np.random.default_rng(seed)
        self.OUT, self.n = OUT, n
        self.om = O.mlp_init(IN, W, OUT, H, activation=activation, output_activation=output_activation)
        self.ph = O.f2h(O.mlp_init_params(self.om, O.pcg32(1337)) * scale)
        self.x = O.f2h(rng.random((n, IN), dtype=np.float32) * scale)
        self.xs = np.ascontiguousarray(self.x.T)
        self.hid_ref, self.out_ref = O.mlp_forward(self.om, self.ph, self.x)
        dy = np.zeros((n, self.om.padded_out), np.float32)
        dy[:, :OUT] = rng.standard_normal((n, OUT)).astype(np.float32) * 0.05
        self.dy = O.f2h(dy)
        self.gref, self.dref = O.mlp_backward(self.om, self.ph, self.x, self.hid_ref, self.out_ref, self.dy)


def check_fp16(s, out, gh, dx, gref=None):
    gref = s.gref if gref is None else gref
    if out is not None:
        e = rae(O.h2f(out), O.h2f(s.out_ref))
        print("output RAE p99", np.percentile(e, 99))
        assert np.percentile(e, 99) < 3e-3
    if gh is not None:
        e = rae(O.h2f(gh), gref)
        print("weight gradient RAE p99", np.percentile(e, 99), "p99.9", np.percentile(e, 99.9))
        assert np.percentile(e, 99) < 3e-3 and np.percentile(e, 99.9) < 1.2e-2
    if dx is not None:
        dref = O.h2f(s.dref)
        assert np.allclose(O.h2f(dx).T, dref, rtol=2e-2, atol=2e-3 * np.abs(dref).max())


@pytest.mark.parametrize("case", CASES)
def test_forward_backward(case):
    # ReLU throughout: the oracle's saved activations go into both backward passes, so a mask cannot differ between them (the linear
    # activations of tests/test_gpu_parity.py:196-199 are for stacks where each side masks with its own forward pass)
    s = Setup(case)
    hid, out = emu.mlp_forward(s.om, s.ph, s.xs)
    check_fp16(s, out, None, None)
    e = rae(O.h2f(hid), O.h2f(s.hid_ref))
    assert np.percentile(e, 99) < 3e-3
    _, out_inf = emu.mlp_forward(s.om, s.ph, s.xs, save_hidden=False)  # two ping-pong buffers instead of the saved stack
    assert np.array_equal(out_inf, out)                                # inference == forward (tests/test_common.h:160-165)
    gh, dx = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy)
    check_fp16(s, None, gh, dx)


def test_accumulate_adds_to_what_is_there():
    s = Setup(CASES[0])
    gh, _ = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy)
    gacc, dx = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy, grads_init=gh)  # GradientMode::Accumulate (fully_fused_mlp.cu:770)
    check_fp16(s, None, gacc, dx, gref=2 * s.gref)


def test_without_input_gradient_and_without_weight_gradients():
    s = Setup(CASES[0])
    gh, dx = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy)
    g_only, no_dx = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy, want_dinput=False)
    assert no_dx is None and np.array_equal(g_only, gh)
    no_g, dx_only = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy, want_grads=False)  # GradientMode::Ignore
    assert no_g is None and np.array_equal(dx_only, dx)


def test_transcendental_activations():
    """Squareplus hidden layers and a Sigmoid output: the out-of-line activation bodies in both epilogues, and the output activation's
    transfer in front of the backward pass (which needs `output`)."""
    s = Setup(CASES[1][:4] + (256,), activation=O.ACT_SQUAREPLUS, output_activation=O.ACT_SIGMOID, scale=0.5, seed=11)
    hid, out = emu.mlp_forward(s.om, s.ph, s.xs)
    check_fp16(s, out, None, None)
    assert np.percentile(rae(O.h2f(hid), O.h2f(s.hid_ref)), 99) < 3e-3
    gh, dx = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy, output=s.out_ref)
    check_fp16(s, None, gh, dx)


@pytest.fixture(scope="module")
def bf16():
    """The oracle's 16-bit format is a process-wide switch and emu.py calls one library at a time: both to bfloat16, restored on the way out."""
    O.set_half_format(True)
    previous = emu.set_bf16(True)
    yield
    emu.set_bf16(previous)
    O.set_half_format(False)


def test_bfloat16_build(bf16):
    s = Setup(CASES[1][:4] + (256,))
    hid, out = emu.mlp_forward(s.om, s.ph, s.xs)
    assert np.percentile(rae(O.h2f(out)[:, :s.OUT], O.h2f(s.out_ref)[:, :s.OUT]), 99) < 3e-2
    assert np.percentile(rae(O.h2f(hid), O.h2f(s.hid_ref)), 99) < 3e-2
    _, out_inf = emu.mlp_forward(s.om, s.ph, s.xs, save_hidden=False)
    assert np.array_equal(out_inf, out)
    gh, dx = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy)
    rel_l2 = lambda a, b: np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)  # noqa: E731
    assert rel_l2(O.h2f(gh), s.gref) < 2e-2
    assert rel_l2(O.h2f(dx).T, O.h2f(s.dref).astype(np.float64)) < 2e-2

"""Networks with more than 128 (padded) outputs, up to 1024, on the host SIMT emulator against the CPU oracle: the layer-by-layer network of
tiny-cuda-nn_amd/csrc/mlp_general.hip at every hidden width (mlp_kernels.h mlp_layer_by_layer), through the launchers tests/test_emu_mlp_general.py
calls -- the real kernel source with an output matrix of 144 / 272 / 1024 / 144-padded-from-130 rows: the tile choice of the forward product, the
K tail of a 16- and 48-wide hidden layer, the backward product's reduction over up to 1024 outputs, and the 64 x 64 weight-gradient tiles over row
counts that are no multiple of 64.  And the trimmed fp32 epilogue of the output layer (GEN_EPI_FORWARD_F32, tests/emu/emu_wide_outputs.py)
against the 16-bit output trimmed and widened in numpy, bit for bit, in both layouts of the C ABI.

fp16 bars: those of tests/test_emu_mlp_general.py -- output RAE p99 < 3e-3, weight gradients RAE p99 < 3e-3 and p99.9 < 1.2e-2, dL/dinput within
rtol 2e-2, atol 2e-3 max|ref|.  bfloat16: outputs RAE p99 < 3e-2, weight gradients and dL/dinput relative L2 < 2e-2 (tests/bf16_cases.py)."""
import numpy as np
import pytest

from oracle import oracle as O

emu = pytest.importorskip("emu")
if not emu.available():
    pytest.skip("ROCm clang++ not available to build the host emulator", allow_module_level=True)
import emu_wide_outputs as emu_wo  # noqa: E402


def rae(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (0.5 * (np.abs(a) + np.abs(b)) + np.abs(b).mean() * 1e-2 + 1e-12)


N = 256
# IN, W, OUT, hidden layers
CASES = [
    (16, 16, 144, 1),    # 9 blocks of 16 outputs: tiles of 3; K = 16 is a quarter of an LDS stage; weight-gradient tiles 64 + 64 + 16 rows x 16 columns
    (32, 64, 272, 2),    # 17 blocks: 6 tiles of 3, the last with two blocks; 4 full weight-gradient tiles and one of 16 rows
    (16, 16, 1024, 1),   # the widest: 16 tiles of 4; the backward product reduces over 16 K steps
    (32, 48, 130, 2),    # 130 outputs padded to 144; a hidden width that is no fused one; K = 48
]


class Setup:
    def __init__(self, case, n=N, seed=2):
        IN, W, OUT, H = case
        rng = np.random.default_rng(seed)
        self.OUT, self.n = OUT, n
        self.om = O.mlp_init(IN, W, OUT, H)
        self.ph = O.f2h(O.mlp_init_params(self.om, O.pcg32(1337)))
        self.x = O.f2h(rng.random((n, IN), dtype=np.float32))
        self.xs = np.ascontiguousarray(self.x.T)
        self.hid_ref, self.out_ref = O.mlp_forward(self.om, self.ph, self.x)
        dy = np.zeros((n, self.om.padded_out), np.float32)
        dy[:, :OUT] = rng.standard_normal((n, OUT)).astype(np.float32) * 0.05
        self.dy = O.f2h(dy)
        self.gref, self.dref = O.mlp_backward(self.om, self.ph, self.x, self.hid_ref, self.out_ref, self.dy)


@pytest.mark.parametrize("case", CASES)
def test_forward_backward(case):
    s = Setup(case)
    assert s.om.padded_out > 128 and s.om.padded_out % 16 == 0
    hid, out = emu.mlp_forward(s.om, s.ph, s.xs)
    e = rae(O.h2f(out), O.h2f(s.out_ref))
    print("output RAE p99", np.percentile(e, 99))
    assert np.percentile(e, 99) < 3e-3
    assert np.percentile(rae(O.h2f(hid), O.h2f(s.hid_ref)), 99) < 3e-3
    _, out_inf = emu.mlp_forward(s.om, s.ph, s.xs, save_hidden=False)
    assert np.array_equal(out_inf, out)  # inference == forward (tests/test_common.h:160-165)
    gh, dx = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy)
    e = rae(O.h2f(gh), s.gref)
    print("weight gradient RAE p99", np.percentile(e, 99), "p99.9", np.percentile(e, 99.9))
    assert np.percentile(e, 99) < 3e-3 and np.percentile(e, 99.9) < 1.2e-2
    # the output matrix on its own (it is most of the parameters at 1024 outputs, and the least of them at 144 x 16)
    n_out = s.om.padded_out * s.om.width
    e = rae(O.h2f(gh)[-n_out:], s.gref[-n_out:])
    assert np.percentile(e, 99) < 3e-3 and np.percentile(e, 99.9) < 1.2e-2
    e = rae(O.h2f(gh)[:-n_out], s.gref[:-n_out])
    print("hidden matrices: weight gradient RAE p99", np.percentile(e, 99))
    assert np.percentile(e, 99) < 3e-3
    dref = O.h2f(s.dref)
    assert np.allclose(O.h2f(dx).T, dref, rtol=2e-2, atol=2e-3 * np.abs(dref).max())


# (IN, W, n_output_dims): 130 -> rows 8-byte aligned when dense, 131 -> 4-byte aligned, 1000 -> 16-byte aligned and 8 padded columns to drop
F32_CASES = [(16, 16, 130), (16, 32, 131), (16, 16, 1000)]


@pytest.fixture(scope="module")
def f32_setups():
    """one 16-bit inference per shape, shared by every layout"""
    setups = {}
    for IN, W, OUT in F32_CASES:
        om = O.mlp_init(IN, W, OUT, 1)
        ph = O.f2h(O.mlp_init_params(om, O.pcg32(7)))
        xs = np.ascontiguousarray(O.f2h(np.random.default_rng(5).random((N, IN), dtype=np.float32) - 0.25).T)
        _, out = emu.mlp_forward(om, ph, xs, save_hidden=False)
        setups[OUT] = (om, ph, xs, O.h2f(out)[:, :OUT].astype(np.float32))
    return setups


def check_f32(result, expected, n_written):
    view, buf = result
    assert view.shape == expected.shape
    assert np.array_equal(view.view(np.uint32), expected.view(np.uint32))  # bit-equal, signed zeros included
    assert np.count_nonzero(~np.isnan(buf)) == n_written                  # and nothing outside the matrix' elements was touched


@pytest.mark.parametrize("dims", [c[2] for c in F32_CASES])
@pytest.mark.parametrize("layout", [emu_wo.COLUMN_MAJOR, emu_wo.ROW_MAJOR])
def test_fp32_epilogue_equals_trim_and_cast(f32_setups, dims, layout):
    om, ph, xs, expected = f32_setups[dims]
    assert np.abs(expected).max() > 0 and not np.isnan(expected).any()
    check_f32(emu_wo.mlp_forward_f32(om, ph, xs, dims, layout), expected, N * dims)


@pytest.mark.parametrize("dims,stride,offset", [
    (131, 132, 0),   # 16-byte stores with a tail of 3 columns: one 8-byte store and a lone column
    (130, 132, 0),   # ... with a tail of one pair
    (131, 132, 2),   # the same rows from an 8-byte aligned base: 8-byte stores and a lone column
    (131, 132, 1),   # ... from a 4-byte aligned base: column by column
    (1000, 1000, 1),
    (130, 131, 0),   # an odd stride under an even width
])
def test_fp32_epilogue_strides_and_alignment(f32_setups, dims, stride, offset):
    """column-major with a stride wider than the row and a base off the 16-byte grid: the store width follows what is aligned for every row"""
    om, ph, xs, expected = f32_setups[dims]
    check_f32(emu_wo.mlp_forward_f32(om, ph, xs, dims, emu_wo.COLUMN_MAJOR, stride=stride, offset_floats=offset), expected, N * dims)


def test_fp32_epilogue_row_major_with_a_stride():
    om = O.mlp_init(16, 16, 131, 1)
    ph = O.f2h(O.mlp_init_params(om, O.pcg32(7)))
    xs = np.ascontiguousarray(O.f2h(np.random.default_rng(5).random((N, 16), dtype=np.float32) - 0.25).T)
    _, out = emu.mlp_forward(om, ph, xs, save_hidden=False)
    check_f32(emu_wo.mlp_forward_f32(om, ph, xs, 131, emu_wo.ROW_MAJOR, stride=N + 3), O.h2f(out)[:, :131].astype(np.float32), N * 131)


def test_fp32_epilogue_serves_every_layer_by_layer_network():
    """not only the wide ones: 48 neurons and 5 outputs, with an output activation (the out-of-line activation body in front of the store)"""
    om = O.mlp_init(32, 48, 5, 2, activation=O.ACT_RELU, output_activation=O.ACT_SIGMOID)
    ph = O.f2h(O.mlp_init_params(om, O.pcg32(3)))
    xs = np.ascontiguousarray(O.f2h(np.random.default_rng(9).random((N, 32), dtype=np.float32)).T)
    _, out = emu.mlp_forward(om, ph, xs, save_hidden=False)
    expected = O.h2f(out)[:, :5].astype(np.float32)
    for layout in (emu_wo.COLUMN_MAJOR, emu_wo.ROW_MAJOR):
        check_f32(emu_wo.mlp_forward_f32(om, ph, xs, 5, layout), expected, N * 5)


@pytest.fixture(scope="module")
def bf16():
    """The oracle's 16-bit format is a process-wide switch and emu.py calls one library at a time: both to bfloat16, restored on the way out."""
    O.set_half_format(True)
    previous = emu.set_bf16(True)
    yield
    emu.set_bf16(previous)
    O.set_half_format(False)


def test_bfloat16_build(bf16):
    s = Setup(CASES[1])
    hid, out = emu.mlp_forward(s.om, s.ph, s.xs)
    assert np.percentile(rae(O.h2f(out)[:, :s.OUT], O.h2f(s.out_ref)[:, :s.OUT]), 99) < 3e-2
    assert np.percentile(rae(O.h2f(hid), O.h2f(s.hid_ref)), 99) < 3e-2
    gh, dx = emu.mlp_backward(s.om, s.ph, s.xs, s.hid_ref, s.dy)
    rel_l2 = lambda a, b: np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)  # noqa: E731
    assert rel_l2(O.h2f(gh), s.gref) < 2e-2
    assert rel_l2(O.h2f(dx).T, O.h2f(s.dref).astype(np.float64)) < 2e-2
    # the fp32 epilogue rounds to bfloat16 and widens: the 16-bit inference's bits, 272 of 272 columns and 259 of them
    _, out_inf = emu.mlp_forward(s.om, s.ph, s.xs, save_hidden=False)
    assert np.array_equal(out_inf, out)
    for dims in (272, 259):
        check_f32(emu_wo.mlp_forward_f32(s.om, s.ph, s.xs, dims, emu_wo.COLUMN_MAJOR, bf16=True), O.h2f(out_inf)[:, :dims].astype(np.float32), N * dims)

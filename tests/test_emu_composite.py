"""csrc/composite_kernels.hip on the host SIMT emulator (no GPU): the triangle-wave kernels, the fused kernels that run all nested encodings
without parameters of a Composite in one launch, and the Sum / Product reductions -- bit for bit against the numpy restatement and the
oracle's per-encoding functions (tests/composite_reference.py), at two and three granules of 256 samples (n = 256 would be one
workgroup; 768 is no power of two), in both layouts, for the 16-bit type of either build and for float.

Frequency is the one encoding that is not held to bits: the kernel calls sinf / cosf, the oracle its own libm -- the bar of the existing
stand-alone test (tests/test_gpu_parity.py::test_frequency_encoding) applies: < 0.2 % of the outputs differ, by at most 2^-10."""
import numpy as np
import pytest

import composite_reference as R
import emu_composite as E
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not E.available(), reason="no host compiler for the emulator")
SIZES = [256, 768]


@pytest.fixture(params=[False, True], ids=["fp16", "bf16"])
def bf16(request):
    O.set_half_format(request.param)
    yield request.param
    O.set_half_format(False)


def _dy(shape, seed):
    return O.f2h(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("soa", [True, False], ids=["feature-major", "sample-major"])
def test_triangle_wave_kernels(n, soa, bf16):
    x = R.kink_inputs(n, 3, seed=n)
    for fp32 in (False, True):
        got = E.triangle_wave_forward(x, 12, 48, soa=soa, fp32=fp32, bf16=bf16)
        assert np.array_equal(got, R.triangle_wave_forward(x, 12, 48, fp32=fp32)), fp32
    assert np.array_equal(got[:, 36:], np.ones((n, 12), np.float32))  # padding
    dy = _dy((n, 48), 1)
    for d in (dy, O.h2f(dy) * np.float32(1.37)):
        got = E.triangle_wave_backward(x, 12, d, soa=soa, bf16=bf16)
        assert np.array_equal(got.view(np.uint32), R.triangle_wave_backward(x, 12, d).view(np.uint32))


def test_triangle_wave_restatement_known_answers():
    """the restatement itself: x = 0.25 -> k = 0: val = 0.125, |0.125 - 0.5| * 4 - 1 = 0.5; k = 1: val = 0.5 -> -1; k = 2: val = 1.0 -> 1;
    slopes -+2^(k+1) with the sign of the half period val * 2 sits in"""
    x = np.array([[0.25]], np.float32)
    assert np.array_equal(R.triangle_wave_forward(x, 3, fp32=True), np.array([[0.5, -1.0, 1.0]], np.float32))
    dy = np.array([[1.0, 1.0, 1.0]], np.float32)
    assert R.triangle_wave_backward(x, 3, dy)[0, 0] == -2.0 + 4.0 - 8.0  # floor(0.25) = 0, floor(1.0) = 1, floor(2.0) = 2


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("soa", [True, False], ids=["feature-major", "sample-major"])
def test_nrc_parts_in_one_launch(n, soa, bf16):
    """the NRC input encoding on 14 dims, bare (62) and behind a network (64: the identity pads 6 -> 8 with ones)"""
    x = R.kink_inputs(n, 14, seed=3 * n)
    for alignment, width in ((1, 62), (16, 64)):
        parts = R.nrc_parts(14, alignment)
        got = E.parts_forward(parts, x, width, soa=soa, bf16=bf16)
        assert np.array_equal(got, R.composite_forward(parts, x, width))
        dy = _dy((n, width), 5)
        dx = E.parts_backward(parts, x, dy, soa=soa, bf16=bf16)
        ref = R.composite_backward_input(parts, x, dy, 14)
        assert np.array_equal(dx[:, :3].view(np.uint32), ref[:, :3].view(np.uint32))  # triangle wave: the restatement's summation order
        assert np.array_equal(dx[:, 8:], ref[:, 8:])  # identity
        assert np.allclose(dx[:, 3:8], ref[:, 3:8], rtol=1e-5, atol=1e-5 * np.abs(ref[:, 3:8]).max())  # one-blob: the stand-alone test's bar
    # fp32 values: the triangle-wave and identity slices are the restatement's / the input's bits
    got = E.parts_forward(R.nrc_parts(14, 1), x, 62, soa=soa, fp32=True, bf16=bf16)
    assert np.array_equal(got[:, :36], R.triangle_wave_forward(x[:, :3], 12, fp32=True)) and np.array_equal(got[:, 56:], x[:, 8:])
    assert np.abs(got[:, 36:56] - O.h2f(O.oneblob_forward(x[:, 3:8], 4))).max() <= (2.0 ** -8 if bf16 else 2.0 ** -11)


@pytest.mark.parametrize("n", SIZES)
def test_parts_with_gaps_a_frequency_part_and_rows_left_to_a_grid(n, bf16):
    """parts out of input order, a Frequency part, output rows [4, 12) that belong to somebody else (a grid) and stay untouched, input
    dims 3..5 that no part reads: their dL_dx is written as zero"""
    x = R.kink_inputs(n, 10, seed=11)
    parts = [dict(kind="Identity", begin=0, dims=3, row=0, padded=4),
             dict(kind="Frequency", begin=8, dims=2, row=12, padded=12, n_frequencies=3),
             dict(kind="TriangleWave", begin=6, dims=2, row=24, padded=8, n_frequencies=2)]
    got = E.parts_forward(parts, x, 32, bf16=bf16, fill=0x1234)
    ref = R.composite_forward(parts, x, 32)
    assert np.all(got[:, 4:12] == 0x1234)
    for p in (parts[0], parts[2]):
        assert np.array_equal(got[:, p["row"]:p["row"] + p["padded"]], ref[:, p["row"]:p["row"] + p["padded"]])
    f, fr = got[:, 12:24], ref[:, 12:24]
    assert np.mean(f != fr) < 2e-3 and np.max(np.abs(O.h2f(f) - O.h2f(fr))) <= (2.0 ** -7 if bf16 else 2.0 ** -10)  # two ulps of the 16-bit type just below 1 (the fp16 figure is the existing bar)
    dy = _dy((n, 32), 6)
    dx = E.parts_backward(parts, x, dy, bf16=bf16)
    dref = R.composite_backward_input(parts, x, dy, 10)
    assert np.array_equal(dx[:, 3:6], np.zeros((n, 3), np.float32))
    assert np.array_equal(dx[:, :3], dref[:, :3]) and np.array_equal(dx[:, 6:8].view(np.uint32), dref[:, 6:8].view(np.uint32))
    assert np.allclose(dx[:, 8:], dref[:, 8:], rtol=1e-4, atol=1e-4 * np.abs(dref[:, 8:]).max())  # test_frequency_encoding's bar


def test_part_table_is_capped():
    parts = [dict(kind="Identity", begin=i, dims=1, row=i, padded=1) for i in range(17)]
    x = np.zeros((256, 17), np.float32)
    out = np.zeros((17, 256), np.uint16)
    t = E._table(parts)
    import ctypes as C
    assert E.lib().emuc_parts_forward(C.c_uint32(17), E._p(t), C.c_uint32(256), C.c_uint32(17), C.c_uint32(17), E._p(x), E._p(out), C.c_int(1), C.c_int(0)) == 1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("product", [False, True], ids=["sum", "product"])
@pytest.mark.parametrize("soa", [True, False], ids=["feature-major", "sample-major"])
def test_reductions(n, product, soa, bf16):
    """three blocks of 16 rows (the product's backward multiplies the OTHER two, ascending), 16-bit and float"""
    rng = np.random.default_rng(n + product)
    v32 = (rng.standard_normal((n, 48)) * 1.5).astype(np.float32)
    dy32 = rng.standard_normal((n, 16)).astype(np.float32)
    for v, dy in ((O.f2h(v32), O.f2h(dy32)), (v32, dy32)):
        fp32 = v.dtype == np.float32
        assert np.array_equal(E.reduce_forward(v, 16, product, soa=soa, bf16=bf16), R.reduce_forward(v, 16, product, fp32=fp32))
        assert np.array_equal(E.reduce_backward(v, dy, 16, product, soa=soa, bf16=bf16), R.reduce_backward(v, dy, 16, 3, product, fp32=fp32))


@pytest.mark.parametrize("n", SIZES)
def test_sum_and_product_of_oneblob_and_triangle_wave(n, bf16):
    """OneBlob 4 bins on 4 dims and TriangleWave 4 frequencies on 4 other dims, width 16: parts -> reduction, reduction backward -> parts"""
    x = R.kink_inputs(n, 8, seed=17)
    parts = [dict(kind="OneBlob", begin=0, dims=4, row=0, padded=16, n_bins=4), dict(kind="TriangleWave", begin=4, dims=4, row=16, padded=16, n_frequencies=4)]
    unreduced = E.parts_forward(parts, x, 32, bf16=bf16)
    assert np.array_equal(unreduced, R.composite_forward(parts, x, 32))
    dy = _dy((n, 16), 8)
    for product in (False, True):
        assert np.array_equal(E.reduce_forward(unreduced, 16, product, bf16=bf16), R.reduce_forward(unreduced, 16, product))
        d_un = E.reduce_backward(unreduced, dy, 16, product, bf16=bf16)
        assert np.array_equal(d_un, R.reduce_backward(unreduced, dy, 16, 2, product))
        dx, ref = E.parts_backward(parts, x, d_un, bf16=bf16), R.composite_backward_input(parts, x, d_un, 8)
        assert np.array_equal(dx[:, 4:].view(np.uint32), ref[:, 4:].view(np.uint32))
        assert np.allclose(dx[:, :4], ref[:, :4], rtol=1e-5, atol=1e-5 * np.abs(ref[:, :4]).max())

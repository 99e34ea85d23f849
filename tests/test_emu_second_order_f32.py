"""The three fp32 second-order kernels of the grid encoding on the host SIMT emulator (no GPU) against the numpy restatement
(tests/grid_second_order_f32_reference.py), on the cases and under the bars of tests/second_order_f32_cases.py at N = 256, with a padded
matrix (stride = L*F + 3: the padding of dL_ddLdoutput must come back as zeros), under max_level (scalar and per sample), on positions
outside the unit cube, and in the -DTCNN_BF16 build, which must return the same bits: the kernels hold no 16-bit type."""
import numpy as np
import pytest

import emu_max_level as E16
import emu_second_order_f32 as E
import grid_domain_positions as P
import second_order_f32_cases as K
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not E.available(), reason="no host compiler for the emulator")

N = 256
PAD = 3


def _padded(dy):
    return np.concatenate([dy, np.full((dy.shape[0], PAD), np.float32(3.0))], axis=1)  # what lies in the padding of dL_doutput must not matter


def _run(og, params, pos, ddx, dy, dy_dx, scalar=1.0, array=None, bf16=False):
    return E.second_order(E.Grid(og, max_level=scalar), array, params, pos, ddx, _padded(dy), dy_dx=dy_dx, bf16=bf16)


@pytest.mark.parametrize("magnitude", K.MAGNITUDES)
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_kernels_against_the_restatement(case, magnitude):
    og = K.oracle_grid(*case)
    pos, params, dy, ddx = K.inputs(og, N, magnitude)
    ref, dy_dx = K.expected(og, params, pos, ddx, dy)
    got = _run(og, params, pos, ddx, dy, dy_dx)
    K.check(og, ref, *got, label=f"{K.case_id(case)} x{magnitude:g}")
    again = _run(og, params, pos, ddx, dy, dy_dx, bf16=True)
    assert np.array_equal(got[1].view(np.uint32), again[1].view(np.uint32)) and np.array_equal(got[2].view(np.uint32), again[2].view(np.uint32))


@pytest.mark.parametrize("pattern", ["scalar", "interleaved"])
@pytest.mark.parametrize("case", [(3, 2, "Smoothstep"), (2, 4, "Linear")], ids=K.case_id)
def test_max_level(case, pattern):
    og = K.oracle_grid(*case)
    from test_gpu_max_level import patterns  # the GPU test's own (it needs no GPU to be imported)
    scalar, array = patterns(N)[pattern]
    off = K.S.off_mask(array if array is not None else scalar, N, og.n_levels, og.n_features_per_level)
    assert off.any() and not off.all()
    pos, params, dy, ddx = K.inputs(og, N, 1.0)
    ref, dy_dx = K.expected(og, params, pos, ddx, dy, off=off)
    masked_dy_dx = dy_dx.copy()
    masked_dy_dx[K.S.feature_mask(off, og.n_features_per_level)] = 0.0  # what the forward pass stores for an off level
    K.check(og, ref, *_run(og, params, pos, ddx, dy, masked_dy_dx, scalar, array), label=f"{K.case_id(case)} max_level {pattern}")


@pytest.mark.parametrize("case", [(3, 2, "Smoothstep"), (2, 4, "Linear"), (4, 2, "Linear")], ids=K.case_id)
def test_positions_outside_the_unit_cube(case):
    og = K.oracle_grid(*case)
    pos, params, dy, ddx = K.inputs(og, N, 1.0, positions=P.for_grid(og, N, 11))
    ref, dy_dx = K.expected(og, params, pos, ddx, dy)
    K.check(og, ref, *_run(og, params, pos, ddx, dy, dy_dx), label=f"{K.case_id(case)} outside")


def test_the_16_bit_kernels_miss_these_bars():
    """What an fp32 module's second-order pass computed before it had kernels of its own: the 16-bit kernels on the parameters rounded to 16
    bits and on dL_doutput * s rounded to 16 bits, s the largest power of two <= 1024 with max |dL_doutput| * s <= 16384, the results
    divided by s.  On the (3, 2, Smoothstep) case at magnitude 1 they exceed the fp32 bars by (this test, N = 256, printed below):
    dL_dinput 40.9, dL_dparams 2707.9 times.  tests/test_gpu_second_order_f32.py asserts the same of mode 1 on the GPU."""
    og = K.oracle_grid(3, 2, "Smoothstep")
    pos, params, dy, ddx = K.inputs(og, N, 1.0)
    ref, _ = K.expected(og, params, pos, ddx, dy)
    s = min(1024.0, 2.0 ** np.floor(np.log2(16384.0 / np.abs(dy).max())))
    grad_h, dx = E16.grid_backward_backward(E16.Grid(og), None, pos, ddx, O.f2h(dy * np.float32(s)), O.f2h(params))
    r = K.ratios(og, ref, O.h2f(grad_h).astype(np.float64) / s, None, dx.astype(np.float64) / s)
    print(f"16-bit stand-ins, max |got - ref| / fp32 bar: dL_dinput {r['dL_dinput']:.1f}, dL_dparams {r['dL_dparams']:.1f}")
    assert r["dL_dinput"] > 4 and r["dL_dparams"] > 4

"""The second-order pass of a lone fp32 grid encoding through csrc/grid_second_order_f32.hip (tcnn_set_fp32_grid_second_order): dL_dparams
through the owner pass (bit 0) and dL_dinput level-major and tiled (bit 1, set here whatever its default), one straight bwd_bwd_input
call against the float64 restatement (tests/grid_second_order_f32_reference.py) under the bars of tests/second_order_f32_cases.py, which are not widened: the owners' quantum is
below 2^-44 of a value's largest term at these sizes, and the tiled dL_dinput makes the additions of the sample-major kernel in its order.

Grids: 4 levels, log2_hashmap_size 14, per_level_scale 2, so the plan (csrc/grid_backward_plan.h make_f32_backward_plan) cuts more than one
slice; slices per level at the largest slice size: (2, 1) base 64: 1, 2, 2, 2; (3, 2) base 4: 1, 1, 1, 4; (3, 4) base 4: 1, 1, 2, 8;
(4, 8) base 4: 1, 4, 16, 16.  Batches 768 (one and a half scatter tiles at D = 3) and 4352 (the first batch past 4096, where the plan halves
the slices)."""
import numpy as np
import pytest
import torch

import second_order_f32_cases as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GRIDS = {(2, 1): 64, (3, 2): 4, (3, 4): 4, (4, 8): 4}  # (D, F) -> base_resolution


def _C():
    import tinycudann
    return tinycudann._C


def make(d, f, interp):
    cfg = dict(K.config(d, f, interp), log2_hashmap_size=14, base_resolution=GRIDS[(d, f)])
    return _C().create_encoding(d, cfg, _C().Precision.Fp32), O.grid_init(d, K.N_LEVELS, f, 14, GRIDS[(d, f)], 2.0, O.GRID_HASH, K.INTERPS[interp])


def call(m, pos, params, dy, ddx, mask=3, expect=None, before=None, after=None):
    """one bwd_bwd_input call with all three results under `mask` -> dL_dparams, dL_ddLdoutput, dL_dinput on the host"""
    C = _C()
    x, p, v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pos, params, ddx))
    g = torch.zeros((pos.shape[0], m.n_output_dims()), device="cuda")
    g[:, : dy.shape[1]] = torch.from_numpy(np.ascontiguousarray(dy)).cuda()
    try:
        C.set_fp32_grid_second_order(mask)
        if before:
            before(m)
        assert expect is None or m.fp32_grid_second_order(pos.shape[0]) == expect
        ctx, _ = m.fwd(x.requires_grad_(True), p.requires_grad_(True))
        if after:
            after(m)
        d_y, d_p, d_x = m.bwd_bwd_input(ctx, x, p, v, g.requires_grad_(True))
        torch.cuda.synchronize()
    finally:
        C.set_fp32_grid_second_order(1)
        m.set_max_level_gpu(None)
        m.set_max_level(1.0)
    return d_p.cpu().numpy(), d_y.cpu().numpy(), d_x.cpu().numpy()


@pytest.mark.parametrize("n", [768, 4352])
@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
@pytest.mark.parametrize("d,f", list(GRIDS))
def test_parity(d, f, interp, n):
    m, og = make(d, f, interp)
    pos, params, dy, ddx = K.inputs(og, n, 1.0)
    ref, _ = K.expected(og, params, pos, ddx, dy)
    K.check(og, ref, *call(m, pos, params, dy, ddx, mask=3, expect=3), label=f"D{d}F{f} {interp} n={n} mask 3")
    K.check(og, ref, *call(m, pos, params, dy, ddx, mask=0, expect=0), label=f"D{d}F{f} {interp} n={n} mask 0")  # the control


@pytest.mark.parametrize("n", [768, 4352])
@pytest.mark.parametrize("d,f", [(3, 2), (4, 8)])
def test_the_order_of_the_samples_does_not_matter(d, f, n):
    m, og = make(d, f, "Smoothstep")
    pos, params, dy, ddx = K.inputs(og, n, 1.0)
    d_p, _, d_x = call(m, pos, params, dy, ddx, expect=3)
    r_p, _, r_x = call(m, pos[::-1], params, dy[::-1], ddx[::-1])
    assert d_p.any() and np.array_equal(d_p, r_p) and np.array_equal(d_p, call(m, pos, params, dy, ddx)[0])
    assert d_x.any() and np.array_equal(d_x, r_x[::-1])


@pytest.mark.parametrize("power", [13, -20])
def test_the_quantum_follows_the_magnitude(power):
    m, og = make(3, 2, "Smoothstep")
    pos, params, dy, ddx = K.inputs(og, 768, 1.0)
    s = np.float32(2.0 ** power)
    assert np.array_equal(call(m, pos, params, dy * s, ddx)[0], call(m, pos, params, dy, ddx)[0] * s)


@pytest.mark.parametrize("pattern", ["scalar", "interleaved"])
def test_max_level_as_the_forward_pass_saw_it(pattern):
    from test_gpu_max_level import patterns
    n = 768
    m, og = make(3, 2, "Smoothstep")
    scalar, array = patterns(n)[pattern]
    off = K.S.off_mask(array if array is not None else scalar, n, og.n_levels, og.n_features_per_level)
    assert off.any() and not off.all()
    pos, params, dy, ddx = K.inputs(og, n, 1.0)
    ref, _ = K.expected(og, params, pos, ddx, dy, off=off)
    values = None if array is None else torch.from_numpy(array).cuda()

    def before(m):
        m.set_max_level(scalar)
        m.set_max_level_gpu(values)

    def after(m):
        m.set_max_level_gpu(None)
        m.set_max_level(1.0 if pattern == "scalar" else 0.75)

    d_p, d_y, d_x = call(m, pos, params, dy, ddx, expect=3 if array is None else 1, before=before, after=after)
    K.check(og, ref, d_p, d_y, d_x, label=f"max_level {pattern}")
    for l in np.flatnonzero(off.all(axis=0)):
        assert not d_p[og.offsets[l] * 2:og.offsets[l + 1] * 2].any()
    assert pattern != "scalar" or off.all(axis=0).any()

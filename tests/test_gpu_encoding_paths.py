"""A grid created bare and the same grid as the only nested encoding of a Composite run the same steps on the same slices: every result
is compared bit for bit (array_equal), as a 16-bit module, as an fp32 module, and behind a 64x2 network (the feature-major path) in
GradientMode::Overwrite and then Accumulate.

The grid: D = 3, 3 levels x 2 features (6 outputs: no multiple of 16), base resolution 4, log2_hashmap_size 8 -- level 0 is dense (125
vertices), levels 1 and 2 are hashed (729 and 4913 vertices in 256 entries) -- with Linear and with Smoothstep interpolation.  Batches are
the two smallest of test_gpu_composite.py.

Where the padding is: a module made by create_encoding is not aligned, so the bare grid and the Composite of it are both 6 wide and their
sample-major outputs have no padded column to look at.  Padding exists
  * behind the network: 6 -> 16 rows of the feature-major encoded matrix, which only the network reads.  Nothing here asserts that those rows
    are 0 -- bare and nested go through the same step, so equal predictions say nothing about it; the oracle parity tests of grids behind a
    network (tests/test_gpu_parity_full.py) do;
  * sample-major, where a Composite pads a nested grid up to the next nested encoding's alignment: [the grid, a grid with 4 features per
    level] puts the first at columns 0..5, zeros at 6..7 and the second at 8.. .  Its first six columns, dL_dinput and the first grid's
    parameter gradients must equal the bare grid's; columns 6..7 must be exactly 0 (the output's memory is dirtied beforehand).

Why bit equality is the bar: the forward pass and dL_dinput are per-sample arithmetic; the 16-bit parameter gradients come from the
bucketed backward, which sums in fixed point and is order-independent.  The fp32 parameter gradients come from fp32 atomics in arbitrary
order, so their case uses inputs on which every order gives the same bits: positions on multiples of 1/4 and dL_dy in {-1, -1/2, 0, 1/2, 1}.
Such positions are not all vertices of the dense level -- only x = 1/2 is one exactly, and a batch on one vertex tests nothing: with the
scales 3, 7, 15 and the half-cell shift, x * scale + 1/2 has the fraction 1/2, 1/4, 0 or 3/4 on every level, so the weights are coarse dyadic
fractions, 0 and 1 among them.  The condition is verified from the data
(audit_exact_sums): with q the largest power of two dividing every term weight * dL_dy, every entry's sum of |terms| is below 2^24 q, so
every partial sum in any order is a multiple of q with fewer than 24 bits, i.e. an fp32 number."""
import os

import numpy as np
import pytest
import torch

import composite_reference as R
from oracle import oracle as O
from test_gpu_composite import SIZES as COMPOSITE_SIZES

pytestmark = pytest.mark.gpu
BF16 = os.environ.get("TCNN_PRECISION") == "bf16"
HALF = torch.bfloat16 if BF16 else torch.half
SIZES = sorted(COMPOSITE_SIZES)[:2]
D, L, F = 3, 3, 2
K = L * F
GRID = {"otype": "HashGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": 8, "base_resolution": 4, "per_level_scale": 2.0}
GRID_F4 = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 4, "log2_hashmap_size": 8, "base_resolution": 4, "per_level_scale": 2.0}
INTERPOLATIONS = ["Linear", "Smoothstep"]
NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}


def tcnn():
    import tinycudann
    return tinycudann


def grid_cfg(interpolation):
    return dict(GRID, interpolation=interpolation)


def nested_cfg(interpolation):
    return {"otype": "Composite", "nested": [dict(grid_cfg(interpolation), n_dims_to_encode=D)]}


def raw(t):
    """the tensor's bits on the host: 16-bit types as uint16, fp32 as uint32"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.element_size() == 2 else t.numpy().view(np.uint32)


def dirty(shape, dtype):
    """leave NaNs in the block the allocator hands to the next tensor of this shape: a column nobody writes does not read as zero"""
    junk = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    del junk


def run_module(m, x_np, params, dy):
    """forward with input gradients, backward -> (output, dL_dinput, dL_dparams)"""
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    p = params.clone().requires_grad_(True)
    dirty((x_np.shape[0], m.n_output_dims()), params.dtype)
    ctx, y = m.fwd(x, p)
    dx, dp = m.bwd(ctx, x, p, y, dy)
    return y, dx, dp


def random_case(n, n_params, width, fp32, seed):
    rng = np.random.default_rng(seed)
    dtype = torch.float32 if fp32 else HALF
    x_np = R.kink_inputs(n, D, seed=seed)
    params = torch.from_numpy(rng.uniform(-0.5, 0.5, n_params).astype(np.float32)).cuda().to(dtype)
    dy = torch.from_numpy(rng.standard_normal((n, width)).astype(np.float32)).cuda().to(dtype)
    return x_np, params, dy


def exact_case(n, n_params, seed):
    rng = np.random.default_rng(seed)
    x_np = (rng.integers(0, 4, size=(n, D)).astype(np.float32) * np.float32(0.25)).astype(np.float32)
    params = torch.from_numpy(rng.uniform(-0.5, 0.5, n_params).astype(np.float32)).cuda()
    dy_np = (rng.integers(-2, 3, size=(n, K)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    return x_np, params, dy_np


def audit_exact_sums(interpolation, x_np, dy_np):
    """the exactness condition of the fp32 parameter gradient, from the data (see the module's docstring)"""
    og = O.grid_init(D, L, F, GRID["log2_hashmap_size"], GRID["base_resolution"], GRID["per_level_scale"], O.GRID_HASH,
                     {"Linear": O.INTERP_LINEAR, "Smoothstep": O.INTERP_SMOOTHSTEP}[interpolation])
    _, w = O.grid_indices(og, x_np, with_weights=True)  # [n][L][2^D] fp32
    terms = w.astype(np.float64)[:, :, :, None] * dy_np.astype(np.float64).reshape(-1, L, 1, F)  # exact in float64: 24 x 24 bits
    assert np.array_equal(terms.astype(np.float32).astype(np.float64), terms)  # every product is an fp32 number
    lsb = next(k for k in range(64) if np.array_equal(np.rint(terms * 2.0 ** k), terms * 2.0 ** k))
    abs_sums = O.grid_backward_f32(og, x_np, np.abs(dy_np))  # float64 sums of the |terms| of every entry
    assert abs_sums.max() * 2.0 ** lsb < 2.0 ** 24, (lsb, abs_sums.max())
    assert np.count_nonzero(abs_sums) > og.n_params // 2 and np.any((w > 0) & (w < 1)) and np.any(w == 1)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
@pytest.mark.parametrize("fp32", [False, True], ids=["half", "fp32"])
def test_bare_and_nested_modules(n, interpolation, fp32):
    C = tcnn()._C
    precision = [C.Precision.Fp32] if fp32 else []
    bare = C.create_encoding(D, grid_cfg(interpolation), *precision)
    nested = C.create_encoding(D, nested_cfg(interpolation), *precision)
    assert bare.n_params() == nested.n_params() and bare.n_output_dims() >= K and nested.n_output_dims() >= K
    x_np, params, dy = random_case(n, bare.n_params(), max(bare.n_output_dims(), nested.n_output_dims()), fp32, seed=n + len(interpolation))
    yb, dxb, dpb = run_module(bare, x_np, params, dy[:, :bare.n_output_dims()].contiguous())
    yn, dxn, dpn = run_module(nested, x_np, params, dy[:, :nested.n_output_dims()].contiguous())
    assert np.array_equal(raw(yb)[:, :K], raw(yn)[:, :K]) and raw(yb)[:, :K].any()
    # padded columns are exactly 0 on both sides -- today there is none (unaligned modules, see the module's docstring): the line bites once
    # create_encoding aligns; the padding that exists is test_a_grid_padded_to_the_next_nested_one's
    assert not raw(yb)[:, K:].any() and not raw(yn)[:, K:].any()
    assert np.array_equal(raw(dxb), raw(dxn)) and raw(dxb).any()
    if not fp32:  # (fp32: atomics in arbitrary order -- test_fp32_parameter_gradients_on_exact_sums)
        assert np.array_equal(raw(dpb), raw(dpn)) and raw(dpb).any()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
def test_fp32_parameter_gradients_on_exact_sums(n, interpolation):
    C = tcnn()._C
    bare = C.create_encoding(D, grid_cfg(interpolation), C.Precision.Fp32)
    nested = C.create_encoding(D, nested_cfg(interpolation), C.Precision.Fp32)
    assert bare.n_output_dims() == K and nested.n_output_dims() == K
    x_np, params, dy_np = exact_case(n, bare.n_params(), seed=3 * n)
    audit_exact_sums(interpolation, x_np, dy_np)
    dy = torch.from_numpy(dy_np).cuda()
    yb, dxb, dpb = run_module(bare, x_np, params, dy)
    yn, dxn, dpn = run_module(nested, x_np, params, dy)
    assert np.array_equal(raw(yb), raw(yn)) and np.array_equal(raw(dxb), raw(dxn))
    assert np.array_equal(raw(dpb), raw(dpn)) and raw(dpb).any()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fp32", [False, True], ids=["half", "fp32"])
def test_a_grid_padded_to_the_next_nested_one(n, fp32):
    """[the grid, a grid with 4 features per level]: the first is padded 6 -> 8 in the sample-major output"""
    C = tcnn()._C
    precision = [C.Precision.Fp32] if fp32 else []
    bare = C.create_encoding(D, grid_cfg("Linear"), *precision)
    both = C.create_encoding(2 * D, {"otype": "Composite", "nested": [dict(grid_cfg("Linear"), n_dims_to_encode=D), dict(GRID_F4, n_dims_to_encode=D)]}, *precision)
    assert both.n_output_dims() == 16 and both.n_params() > bare.n_params()
    x_np, params, dy = random_case(n, both.n_params(), 16, fp32, seed=7 * n)
    x6 = np.ascontiguousarray(np.concatenate([x_np, x_np[::-1]], axis=1))
    if fp32:  # (order-independent sums for the atomics)
        x_np, _, dy_np = exact_case(n, both.n_params(), seed=7 * n)
        audit_exact_sums("Linear", x_np, dy_np)
        x6 = np.ascontiguousarray(np.concatenate([x_np, x_np[::-1]], axis=1))
        dy = torch.zeros((n, 16), device="cuda")
        dy[:, :K] = torch.from_numpy(dy_np).cuda()
        dy[:, 8:] = torch.from_numpy(dy_np[:, :1]).cuda()
    yb, dxb, dpb = run_module(bare, x_np, params[:bare.n_params()].contiguous(), dy[:, :K].contiguous())
    y, dx, dp = run_module(both, x6, params, dy)
    assert np.array_equal(raw(y)[:, :K], raw(yb)) and raw(yb).any()
    assert not raw(y)[:, K:8].any()
    assert np.array_equal(raw(dx)[:, :D], raw(dxb))
    assert np.array_equal(raw(dp)[:bare.n_params()], raw(dpb)) and raw(dpb).any()


@pytest.mark.parametrize("fp32", [False, True], ids=["half", "fp32"])
def test_a_pending_backward_keeps_the_scalar_max_level(fp32):
    """the slice of a lone grid's backward pass carries the scalar max_level its forward pass read, whatever set_max_level has been told
    since (tests/test_gpu_max_level.py changes the per-sample array, which wins over the scalar)"""
    C = tcnn()._C
    n = SIZES[0]
    x_np, params, dy_np = exact_case(n, C.create_encoding(D, grid_cfg("Linear")).n_params(), seed=11)
    audit_exact_sums("Linear", x_np, dy_np)  # (levels switched off only remove terms)
    dtype = torch.float32 if fp32 else HALF
    params, dy = params.to(dtype), torch.from_numpy(dy_np).cuda().to(dtype)
    got = []
    for later in (0.5, 1.0):
        m = C.create_encoding(D, grid_cfg("Linear"), *([C.Precision.Fp32] if fp32 else []))
        m.set_max_level(0.5)
        x = torch.from_numpy(x_np).cuda().requires_grad_(True)
        p = params.clone().requires_grad_(True)
        ctx, y = m.fwd(x, p)
        m.set_max_level(later)
        got.append((y,) + tuple(m.bwd(ctx, x, p, y, dy)))
    for a, b in zip(*got):
        assert np.array_equal(raw(a), raw(b)) and raw(a).any()
    m.set_max_level(1.0)
    _, _, dp_all = run_module(m, x_np, params, dy)
    assert not np.array_equal(raw(dp_all), raw(got[0][2]))  # (half of the levels were off)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
def test_behind_a_network_overwrite_then_accumulate(n, interpolation):
    T = tcnn()
    GM = T._C.GradientMode
    cfg = {"loss": {"otype": "L2"}, "optimizer": ADAM, "network": NETWORK}
    bare = T.create_from_config(D, 3, dict(cfg, encoding=grid_cfg(interpolation)), seed=5)
    nested = T.create_from_config(D, 3, dict(cfg, encoding=nested_cfg(interpolation)), seed=5)
    assert bare.n_params == nested.n_params
    w = bare.params_full_precision.cpu().numpy().copy()
    w[bare.n_mlp_params:] *= 1.0e3  # grid.h:1076-1079 initialises in U(-1e-4, 1e-4)
    bare.set_params_full_precision(torch.from_numpy(w))
    nested.set_params_full_precision(torch.from_numpy(w))
    assert np.array_equal(raw(bare.params), raw(nested.params))
    x = torch.from_numpy(R.kink_inputs(n, D, seed=n + 1)).cuda()
    t = torch.from_numpy(np.random.default_rng(n).random((n, 3), dtype=np.float32)).cuda()
    first = None
    for mode in (GM.Overwrite, GM.Accumulate):
        got = []
        for tm in (bare, nested):
            dx = torch.full((n, D), 7.0, device="cuda")
            ctx = tm.training_step(x, t, run_optimizer=False, dL_dinput=dx, gradient_mode=mode)
            got.append((raw(ctx.output), raw(dx), raw(tm.param_gradients)))
        for a, b in zip(*got):
            assert np.array_equal(a, b) and a.any()
        if first is None:
            first = got[0][2]
        else:  # Accumulate added to what Overwrite left
            assert not np.array_equal(got[0][2][bare.n_mlp_params:], first[bare.n_mlp_params:])

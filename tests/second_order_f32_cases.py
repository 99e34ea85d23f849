"""Cases, inputs and bars shared by the emulator and the GPU tests of the fp32 grid encoding's second-order pass
(tests/test_emu_second_order_f32.py, tests/test_gpu_second_order_f32.py); the expected values are tests/grid_second_order_f32_reference.py's.

Grids: 4 levels, log2_hashmap_size 10, base_resolution 4, per_level_scale 2 -- resolutions 4, 8, 16, 32: small tables that a batch of a few
hundred samples hits many times per entry, hashed (colliding) finest levels at D >= 3 -- for (D, F) in {(3, 2), (2, 4), (3, 1), (4, 2)},
Linear and Smoothstep each, and one Nearest grid.  Inputs that 16 bits cannot represent: parameters standard_normal * 0.3, ddx
standard_normal * 1e-2, dL_doutput standard_normal at magnitude 1, 1e4 or 1e-6, all fp32.

Bars, u = 2^-24, against the restatement's float64 values and its magnitudes mag_* (the same sums over absolute values).  Every constant
counts the fp32 roundings of the kernels as written (csrc/grid_second_order.hip, csrc/grid_backward.hip, csrc/grid_device.h); operands the
restatement shares with the kernels bit for bit (the fraction t, scale, ddx, dL_dy, the parameters, dy_dx) carry none.

 * dL_ddLdoutput: |got - ref| <= (D + 1) u mag_y.  k_grid_backward_backward_dLdoutput_f32 adds D rounded products to 0.0f in order: term d
   passes through its own rounding and the D - d additions after it (the first addition, to zero, is exact), at most D roundings; first-order
   (1 + u)^D - 1 < (D + 1) u.  Padded columns are exactly 0.
 * dL_dinput: |got - ref| <= K_x u mag_x with K_x = n_levels * 2^D * D + 40.  One output sums n_levels * 2^D * D terms wgt * v(c) (per level
   and corner one diagonal and D - 1 mixed terms; the diagonal ones are zero for Linear) in grad_out / out[a]: a term meets at most as many
   additions as there are terms, each contributing u times a partial sum <= mag_x.  The chain of one term, at the worst case D = 4, F = 4,
   Smoothstep: s2 = scale * scale (1); times ddx (1); S'(t_b) = 6 * t * (1 - t) (3) and its product (1), twice (8 together; the diagonal
   term's 12 * (0.5 - t) with its product is 3, every factor rounded relative to itself); the signs are exact; D - 2 = 2 weights: the
   upper one S(t) = t * t * (3 - 2t) (3: 2t is exact), the lower one S(1 - t) (the rounding of 1 - t reaches S at most doubled,
   d log S / d log x = 6 (1 - x) / (3 - 2x) <= 2, plus S's own 3: 5), and its product (1): at most 12; times v (1); v itself, F products and
   F - 1 additions of them, contributes at most 2F - 1 = 7 relative to sum_f |grid| |dL_dy|: 1 + 1 + 8 + 12 + 1 + 7 = 30, rounded up to 40
   for the second-order terms of (1 + u)^k.  K_x = 136 at D = 3, 104 at D = 2, 296 at D = 4 -- below the cap 2 * n_levels * 2^D * D + 64.
 * dL_dparams: |got - ref| <= (hits + K_w) u mag_p with K_w = 30.  An entry's value is the running fp32 sum of `hits` contributions (one
   rounding per atomic addition, each <= u times a partial sum <= mag_p).  One contribution weight * dL_dy[f], at D = 4, Smoothstep: per
   dimension d, scale * ddx (1), S'(t_d) (3) and its product (1), D - 1 = 3 weights of at most 6 roundings each as above (18): 23; the sum
   over d adds D - 1 = 3 roundings to a term; the product with dL_dy (1): 27, rounded up to 30.  Entries nothing contributes to
   (hits == 0) are exactly 0.
 * No term of these counts is a difference of rounded values: the kernels form Smoothstep's lower weight as S(1 - t), not 1 - S(t), and
   its second derivative as 12 * (0.5 - t), not 6 - 12t (csrc/grid_device.h second_order_weights_f32, csrc/grid_second_order.hip).  With
   the reference's forms the Smoothstep cases missed the dL_dparams bar 17 to 300 times over on the emulator (entries whose few
   contributions have t near 1).
 * Nearest: everything is zero (the interpolation has no second derivative and dy_dx is zero)."""
import numpy as np

import grid_second_order_f32_reference as S
from oracle import oracle as O

U = 2.0 ** -24
N_LEVELS = 4
K_W = 30
SHAPES = [(3, 2), (2, 4), (3, 1), (4, 2)]
INTERPS = {"Linear": O.INTERP_LINEAR, "Smoothstep": O.INTERP_SMOOTHSTEP, "Nearest": O.INTERP_NEAREST}
CASES = [(d, f, i) for d, f in SHAPES for i in ("Linear", "Smoothstep")] + [(3, 2, "Nearest")]
MAGNITUDES = [1.0, 1e4, 1e-6]


def case_id(c):
    return f"D{c[0]}F{c[1]}-{c[2]}"


def k_x(d):
    k = N_LEVELS * (1 << d) * d + 40
    assert k <= 2 * N_LEVELS * (1 << d) * d + 64
    return k


def config(d, f, interp):
    return {"otype": "HashGrid", "n_levels": N_LEVELS, "n_features_per_level": f, "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 2.0,
            "interpolation": interp}


def oracle_grid(d, f, interp):
    return O.grid_init(d, N_LEVELS, f, 10, 4, 2.0, O.GRID_HASH, INTERPS[interp])


def inputs(og, n, magnitude, seed=7, positions=None):
    """-> pos [n, D], params [n_params], dy [n, L*F], ddx [n, D], all float32"""
    d, k = og.n_dims, og.n_levels * og.n_features_per_level
    r = np.random.default_rng([seed, d, og.n_features_per_level, n])
    pos = O.generate_random_uniform(O.pcg32(seed + n), n * d, 0.0, 1.0).reshape(n, d) if positions is None else positions
    params = (r.standard_normal(og.n_params) * 0.3).astype(np.float32)
    dy = (r.standard_normal((n, k)) * magnitude).astype(np.float32)
    ddx = (r.standard_normal((n, d)) * 1e-2).astype(np.float32)
    for a in (params, dy):  # 16 bits cannot represent them
        assert np.mean(O.h2f(O.f2h(a)) != a) > 0.9
    return pos, params, dy, ddx


def expected(og, params, pos, ddx, dy, off=None):
    """the restatement on the dy_dx the fp32 forward pass stores (the oracle's, which that pass equals bit for bit: tests/test_gpu_parity.py)"""
    _, dy_dx = O.grid_forward_f32(og, params, pos, want_dy_dx=True)
    return S.second_order(og, params, pos, ddx, dy, off=off, dy_dx=dy_dx), dy_dx


def ratios(og, ref, d_p, d_y, d_x):
    """largest |got - ref| / bar of each result (0 / 0 counts as 0, a non-zero value over a zero bar as inf); None for a result not given"""
    def worst(err, bar):
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bar)
        return float(np.max(q))

    k = og.n_levels * og.n_features_per_level
    out = {}
    if d_p is not None:
        out["dL_dparams"] = worst(np.abs(np.asarray(d_p, np.float64) - ref.dL_dparams), (ref.hits + K_W) * U * ref.mag_p)
    if d_y is not None:
        out["dL_ddLdoutput"] = worst(np.abs(np.asarray(d_y, np.float64)[:, :k] - ref.dL_ddLdoutput), (og.n_dims + 1) * U * ref.mag_y)
    if d_x is not None:
        out["dL_dinput"] = worst(np.abs(np.asarray(d_x, np.float64) - ref.dL_dinput), k_x(og.n_dims) * U * ref.mag_x)
    return out


def check(og, ref, d_p, d_y, d_x, label=""):
    """prints each figure, then asserts the bars of the module docstring"""
    k = og.n_levels * og.n_features_per_level
    r = ratios(og, ref, d_p, d_y, d_x)
    print(f"{label} max |got - ref| / bar: " + ", ".join(f"{name} {v:.4f}" for name, v in r.items()))
    if og.interpolation == O.INTERP_NEAREST:
        assert not np.asarray(d_x).any() and not np.asarray(d_p).any() and (d_y is None or not np.asarray(d_y).any())
        return r
    assert np.abs(ref.dL_dparams).max() > 0 and np.abs(ref.dL_dinput).max() > 0 and np.abs(ref.dL_ddLdoutput).max() > 0
    assert not np.asarray(d_p)[ref.hits == 0].any()
    if d_y is not None:
        assert not np.asarray(d_y)[:, k:].any()
    assert all(v <= 1.0 for v in r.values()), r
    return r

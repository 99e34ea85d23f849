"""Reference for the Composite / TriangleWave tests (host emulator and GPU): a numpy-fp32 restatement of the triangle-wave encoding
(reference encodings/triangle_wave.h:46-108) and of the Sum / Product reductions (encodings/composite.h:47-133), operation by operation,
and the composition of a Composite out of the oracle's per-encoding functions laid out by composite.h:188-211 / 362-400.
Plain numpy over the oracle; nothing here touches the emulator or the GPU library.

A "part" is a dict: kind ("TriangleWave" | "OneBlob" | "Frequency" | "Identity" | "Grid"), begin (first input dim), dims, row (first output
row), padded (padded width), and n_frequencies / n_bins / grid (oracle Grid) / params_offset as the kind needs.  Values are 16-bit
patterns (uint16, the oracle's current half format) or float32."""
import numpy as np

from oracle import oracle as O

f32 = np.float32


def _round(y, fp32):
    return y.astype(f32) if fp32 else O.f2h(y.astype(f32))


def _widen(v):
    return v.astype(f32) if v.dtype == np.float32 else O.h2f(v)


# ---------------------------------------------------------------------------------------------- triangle wave
def triangle_wave_phase(x, n_frequencies):
    """val of triangle_wave.h:70-73 for every (sample, dim, k): fp32, one rounding per step"""
    x = np.asarray(x, dtype=f32)
    k = np.arange(n_frequencies, dtype=np.int32)
    scaled = np.ldexp(x[:, :, None], k[None, None, :] - 1).astype(f32)  # scalbnf(in, k - 1): exact
    return (scaled + (k.astype(f32) * f32(0.25))[None, None, :]).astype(f32)


def triangle_wave_forward(x, n_frequencies, padded=None, fp32=False):
    """[n, d] fp32 -> [n, padded]: fabsf(val - floorf(val) - 0.5f) * 4 - 1 (:74), padding 1 (:64-65)"""
    n, d = x.shape
    val = triangle_wave_phase(x, n_frequencies)
    t = (val - np.floor(val)).astype(f32)
    t = (t - f32(0.5)).astype(f32)
    y = ((np.abs(t) * f32(4)).astype(f32) - f32(1)).astype(f32)
    out = np.ones((n, padded or d * n_frequencies), dtype=f32)
    out[:, :d * n_frequencies] = y.reshape(n, d * n_frequencies)
    return _round(out, fp32)


def triangle_wave_backward(x, n_frequencies, dL_dy):
    """dL_dx[i, j] = sum_k dL_dy[i, j F + k] * scalbnf((int)floorf(val * 2) % 2 == 0 ? -1 : 1, k + 1) (:78, :103-107), fp32, ascending k"""
    n, d = x.shape
    val = triangle_wave_phase(x, n_frequencies)
    even = np.fmod(np.floor((val * f32(2)).astype(f32)).astype(np.int64), 2) == 0  # C's %: the sign of the dividend, zero for even either way
    k = np.arange(n_frequencies, dtype=np.int32)
    dy_dx = np.ldexp(np.where(even, f32(-1), f32(1)).astype(f32), k[None, None, :] + 1).astype(f32)
    dy = _widen(np.asarray(dL_dy)[:, :d * n_frequencies]).reshape(n, d, n_frequencies)
    result = np.zeros((n, d), dtype=f32)
    for kk in range(n_frequencies):
        result = (result + (dy[:, :, kk] * dy_dx[:, :, kk]).astype(f32)).astype(f32)
    return result


# ---------------------------------------------------------------------------------------------- reductions (composite.h:47-133)
def reduce_forward(to_reduce, width, product, fp32=False):
    """[n, width * K] -> [n, width]: fp32 accumulation in nested order from 0 (sum) / 1 (product), rounded at the store"""
    v = _widen(to_reduce)
    K = v.shape[1] // width
    result = np.full((v.shape[0], width), 1.0 if product else 0.0, dtype=f32)
    for k in range(K):
        blk = v[:, k * width:(k + 1) * width]
        result = (result * blk).astype(f32) if product else (result + blk).astype(f32)
    return _round(result, fp32)


def reduce_backward(to_reduce, dL_dreduced, width, K, product, fp32=False):
    """-> dL_dunreduced [n, width * K]; the product: dL_dreduced times all OTHER nested values, ascending (:119-130)"""
    if not product:
        return np.tile(np.asarray(dL_dreduced), (1, K))
    v, dy = _widen(to_reduce), _widen(dL_dreduced)
    out = np.empty((v.shape[0], width * K), dtype=f32)
    for k in range(K):
        result = dy.copy()
        for l in range(K - 1):
            o = l if l < k else l + 1
            result = (result * v[:, o * width:(o + 1) * width]).astype(f32)
        out[:, k * width:(k + 1) * width] = result
    return _round(out, fp32)


# ---------------------------------------------------------------------------------------------- composition
def nrc_parts(n_dims=14, alignment=1, n_frequencies=12, n_bins=4):
    """encoding.cu:93-115 laid out by composite.h:188-198 (every required alignment is 1) and set_alignment (the last part takes the padding)"""
    w = [3 * n_frequencies, 5 * n_bins, n_dims - 8]
    total = sum(w)
    w[2] += -total % alignment
    return [dict(kind="TriangleWave", begin=0, dims=3, row=0, padded=w[0], n_frequencies=n_frequencies),
            dict(kind="OneBlob", begin=3, dims=5, row=w[0], padded=w[1], n_bins=n_bins),
            dict(kind="Identity", begin=8, dims=n_dims - 8, row=w[0] + w[1], padded=w[2])]


def part_forward(part, x, params=None, fp32=False, want_dy_dx=False):
    """one part on its slice of the input -> [n, padded] in the value type"""
    xs = np.ascontiguousarray(x[:, part["begin"]:part["begin"] + part["dims"]], dtype=f32)
    kind, padded = part["kind"], part["padded"]
    if kind == "TriangleWave":
        return triangle_wave_forward(xs, part["n_frequencies"], padded, fp32)
    if kind == "Grid":
        g = part["grid"]
        p = params[part["params_offset"]:part["params_offset"] + g.n_params]
        k = g.n_levels * g.n_features_per_level
        fwd = O.grid_forward_f32 if fp32 else O.grid_forward
        r = fwd(g, p, xs, out_stride=padded, want_dy_dx=want_dy_dx)
        out = r[0] if want_dy_dx else r
        out[:, k:] = 0  # grid.h:757-766: padded dims are zero
        return (out, r[1]) if want_dy_dx else out
    assert not fp32, "the oracle's element-wise encodings are 16-bit"
    if kind == "OneBlob":
        return O.oneblob_forward(xs, part["n_bins"], padded)
    if kind == "Frequency":
        return O.frequency_forward(xs, part["n_frequencies"], padded)
    return O.identity_forward(xs, padded)


def composite_forward(parts, x, width, params=None, fp32=False):
    """Concatenation: [n, width]; for a reduction pass the unreduced width and reduce_forward the result"""
    out = np.zeros((x.shape[0], width), dtype=f32 if fp32 else np.uint16)
    for p in parts:
        out[:, p["row"]:p["row"] + p["padded"]] = part_forward(p, x, params, fp32)
    return out


def part_backward_input(part, x, dL_dy, params=None):
    """dL_dx [n, dims] of one part from its rows of dL_dy ([n, >= row + padded], 16-bit)"""
    xs = np.ascontiguousarray(x[:, part["begin"]:part["begin"] + part["dims"]], dtype=f32)
    dy = np.ascontiguousarray(dL_dy[:, part["row"]:part["row"] + part["padded"]])
    kind = part["kind"]
    if kind == "TriangleWave":
        return triangle_wave_backward(xs, part["n_frequencies"], dy)
    if kind == "OneBlob":
        return O.oneblob_backward(xs, part["n_bins"], dy)
    if kind == "Frequency":
        return O.frequency_backward(xs, part["n_frequencies"], dy)
    if kind == "Grid":
        g = part["grid"]
        p = params[part["params_offset"]:part["params_offset"] + g.n_params]
        if dy.dtype == np.float32:
            _, dy_dx = O.grid_forward_f32(g, p, xs, want_dy_dx=True)
            return O.grid_backward_input_f32(g, dy, dy_dx)
        _, dy_dx = O.grid_forward(g, p, xs, want_dy_dx=True)
        return O.grid_backward_input(g, dy, dy_dx)
    # identity.h:83 with scale 1: (T)((float)dL_dy * 1), widened
    return _widen(dy[:, :part["dims"]])


def composite_backward_input(parts, x, dL_dy, n_dims, params=None):
    """dims no part reads get zero"""
    dx = np.zeros((x.shape[0], n_dims), dtype=f32)
    for p in parts:
        dx[:, p["begin"]:p["begin"] + p["dims"]] = part_backward_input(p, x, dL_dy, params)
    return dx


def kink_inputs(n, d, seed):
    """uniform [0, 1) inputs with a block of exact multiples of 2^-13 and the values 0, 0.25, 0.5, 1 - 2^-24: these sit on the kinks of the
    triangle waves (and on the one-blob bin boundaries)"""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d), dtype=f32)
    m = n // 4
    x[:m] = (rng.integers(0, 1 << 13, size=(m, d)).astype(f32) * f32(2.0 ** -13)).astype(f32)
    special = np.array([0.0, 0.25, 0.5, 1.0 - 2.0 ** -24], dtype=f32)
    x[m:m + 4 * d] = special[(np.arange(4 * d)[:, None] + np.arange(d)[None, :]) % 4]
    return x

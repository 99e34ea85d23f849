"""numpy restatement of a layer-by-layer network whose hidden activation needs the PRE-activation for its derivative: Sine (SIREN) and SiLU.
The CPU oracle knows neither, so the tests of these activations (tests/test_library_sine_silu.py, test_emu_sine_silu.py,
test_gpu_sine_silu.py) compare with this module; it is pinned itself against a float64 torch network in the first of them.

Arithmetic (what the reference's layer-by-layer network computes, networks/cutlass_mlp: a product, then an element-wise pass over 16-bit
matrices), with every rounding to the 16-bit type written as R():
  forward, per hidden layer     pre  = R(W x)                      post = R(f(pre))  with f evaluated in fp32 on the ROUNDED pre
  output layer                  out  = R(W_out post)               (no output activation: Sine / SiLU are refused there)
  backward, per hidden layer    d    = R( R(W^T d_above) * R(f'(pre)) )          -- a 16-bit times 16-bit product, one rounding
  weight gradients              dW   = sum_samples d[out] * a[in]   a = the network input / the post-activations below
  Sine: f = sin, f' = cos.      SiLU: f = x * l, f' = l + x * (l * (1 - l)),  l = 1 / (1 + exp(-x)).
R() is the oracle's conversion, so `oracle.set_half_format(True)` turns this module to bfloat16 with it.

Two accumulation modes for the products, the band idea of oracle/tcnn_oracle.h:41-43: "f32" sums the (exact) fp32 products in k order in
fp32, "f64" sums them in float64.  MFMA hardware sums in neither order; a comparison is only meaningful where the two modes agree far
inside the bar it uses (band(), asserted in tests/test_library_sine_silu.py for the shared cases below).

Comparisons are made LAYER BY LAYER ON SHARED STACKS: the reference of a layer is computed from the stored activations of the side under
test (forward_on()), and the backward pass of both sides reads the same stacks.  Two sides that each run their own chain differ by more
than rounding in a deep, wide network: a sum that lands near a rounding boundary of the 16-bit pre-activation flips it by one place, the
flips of a layer move every sum of the next one, and the rate grows about eightfold per layer -- at (80, 272, 40, 3, 768) 2.4 % (Sine) /
3.4 % (SiLU) of the third layer's pre-activations differ between the two accumulation modes of THIS module, which alone puts their weight
gradients 4.2e-3 / 3.0e-3 (RAE p99) and 1.4e-2 / 1.1e-2 (p99.9) apart: past the bars, whatever the kernel does.  On shared stacks the two
modes stay within 7.6e-4 / 3.7e-3 there, and the bars measure the layer under test.

The SIREN initialisation (gpu_matrix.h:343-377, cutlass_mlp.cu:362-371): one rng, matrices in layer order, the first with
s = scale * (30 / fan_in), every other one (the output matrix too) with s = scale * sqrt(6 / fan_in), element = next_float * 2 * s - s
evaluated left to right in fp32."""
import ctypes as C

import numpy as np

from oracle import oracle as O

ACT_SILU, ACT_SINE = 8, 9  # Activation::SiLU / Sine of activation_device.h (0-7 are the oracle's ORC_ACT_*)
NAMES = {ACT_SILU: "SiLU", ACT_SINE: "Sine"}

# IN, W, OUT, hidden layers, n -- the shapes the emulator and GPU tests share
CASES = [
    (16, 48, 3, 1, 256),     # one partial block of neurons
    (32, 64, 4, 2, 256),     # a fused width on the layer-by-layer path, K exactly one LDS stage
    (80, 272, 40, 3, 768),   # several neuron tiles, K over several stages with a ragged last one, > 16 outputs, 12 sample stages over uneven slices
]


def R(x):
    """round to the 16-bit type and back"""
    return O.h2f(O.f2h(np.asarray(x, np.float32)))


def rae(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (0.5 * (np.abs(a) + np.abs(b)) + np.abs(b).mean() * 1e-2 + 1e-12)


def layer_shapes(IN, W, OUT, H):
    """(rows, cols) of every weight matrix in parameter order; the output matrix is padded to 16 rows"""
    return [(W, IN)] + [(W, W)] * (H - 1) + [((OUT + 15) // 16 * 16, W)]


def n_params(IN, W, OUT, H):
    return sum(r * c for r, c in layer_shapes(IN, W, OUT, H))


def split(params, IN, W, OUT, H):
    out, at = [], 0
    for r, c in layer_shapes(IN, W, OUT, H):
        out.append(np.asarray(params[at:at + r * c]).reshape(r, c))
        at += r * c
    return out


def next_floats(rng, count):
    fn = O.lib().orc_pcg32_next_float
    return np.array([fn(C.byref(rng)) for _ in range(count)], dtype=np.float32)


def siren_init_params(IN, W, OUT, H, rng, scale=1.0):
    """fp32 parameters of a Sine network, advancing `rng` (oracle.pcg32) as the library does"""
    out = []
    for i, (rows, cols) in enumerate(layer_shapes(IN, W, OUT, H)):
        if i == 0:
            s = np.float32(scale) * (np.float32(30.0) / np.float32(cols))
        else:
            s = np.float32(scale) * np.sqrt(np.float32(6.0) / np.float32(cols))
        t = next_floats(rng, rows * cols) * np.float32(2.0)
        t = t * s
        out.append(t - s)
    return np.concatenate(out).astype(np.float32)


def init_params(act, IN, W, OUT, H, seed=1337):
    """what Model::initialize_params draws for this activation: SIREN for Sine, Xavier (the oracle's) otherwise"""
    if act == ACT_SINE:
        return siren_init_params(IN, W, OUT, H, O.pcg32(seed))
    return O.mlp_init_params(O.mlp_init(IN, W, OUT, H), O.pcg32(seed))


def _f(act, x):
    x = x.astype(np.float32)
    if act == ACT_SINE:
        return np.sin(x)
    one = np.float32(1.0)
    return x * (one / (one + np.exp(-x)))


def _df(act, x):
    x = x.astype(np.float32)
    if act == ACT_SINE:
        return np.cos(x)
    one = np.float32(1.0)
    l = one / (one + np.exp(-x))
    return l + x * (l * (one - l))


def _product(a, b, mode):
    """a [n][K] . b [M][K]^T -> [n][M] fp32; the fp32 products of 16-bit values are exact, the modes differ in how they are summed"""
    if mode == "f64":
        return (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[None, :, k]
    return acc


def _outer_sum(d, a, mode):
    """sum over samples of d[s][o] a[s][i] -> [O][I], float64 out"""
    if mode == "f64":
        return d.astype(np.float64).T @ a.astype(np.float64)
    acc = np.zeros((d.shape[1], a.shape[1]), np.float32)
    for s in range(d.shape[0]):
        acc += d[s, :, None] * a[s, None, :]
    return acc.astype(np.float64)


def forward(act, shape, params_h, x_h, mode="f64"):
    """params_h: 16-bit patterns [n_params]; x_h: [n][IN] patterns.  Returns (pre [H][n][W], post [H][n][W], out [n][OUTP]) as patterns."""
    IN, W, OUT, H = shape
    mats = [O.h2f(m) for m in split(params_h, IN, W, OUT, H)]
    a = O.h2f(x_h)
    pre, post = [], []
    for Wl in mats[:-1]:
        p = R(_product(a, Wl, mode))
        a = R(_f(act, p))
        pre.append(p)
        post.append(a)
    out = _product(a, mats[-1], mode)
    return O.f2h(np.stack(pre)), O.f2h(np.stack(post)), O.f2h(out)


def backward(act, shape, params_h, x_h, pre_h, post_h, dy_h, mode="f64"):
    """dy_h: dL/doutput [n][OUTP] patterns.  Returns (weight gradients float64 [n_params], dL/dinput [n][IN] patterns)."""
    IN, W, OUT, H = shape
    mats = [O.h2f(m) for m in split(params_h, IN, W, OUT, H)]
    x, pre, post = O.h2f(x_h), O.h2f(pre_h), O.h2f(post_h)
    d = O.h2f(dy_h)
    grads = [None] * (H + 1)
    grads[H] = _outer_sum(d, post[H - 1], mode)
    for j in range(H - 1, -1, -1):
        back = R(_product(d, np.ascontiguousarray(mats[j + 1].T), mode))
        d = R(back * R(_df(act, pre[j])))
        grads[j] = _outer_sum(d, post[j - 1] if j > 0 else x, mode)
    dx = _product(d, np.ascontiguousarray(mats[0].T), mode)
    return np.concatenate([g.reshape(-1) for g in grads]), O.f2h(dx)


def forward_on(act, shape, params_h, x_h, pre_h, post_h, mode="f64"):
    """The forward reference of every layer from the OTHER side's stored activations (see the module text): pre[l] from its post[l - 1],
    post[l] from its pre[l], the output from its last post.  Same form as forward()'s result."""
    IN, W, OUT, H = shape
    mats = [O.h2f(m) for m in split(params_h, IN, W, OUT, H)]
    below = [O.h2f(x_h)] + [O.h2f(post_h[l]) for l in range(H)]
    pre = [_product(below[l], mats[l], mode) for l in range(H)]
    post = [_f(act, O.h2f(pre_h[l])) for l in range(H)]
    return dict(pre=O.f2h(np.stack(pre)), post=O.f2h(np.stack(post)), out=O.f2h(_product(below[H], mats[H], mode)))


class Case:
    """One shared test case, fixed on the CPU: inputs uniform in [0, 1), the library's own initialisation at seed 1337 (SIREN / Xavier),
    dL/doutput = 0.05 N(0, 1) on the real outputs; the restatement's own chain in float64 mode (ref["f64"]) and, on its stacks, the float32
    mode (ref["f32"]), computed once."""

    def __init__(self, act, case, seed=2):
        IN, W, OUT, H, n = case
        self.act, self.case, self.shape, self.n = act, case, (IN, W, OUT, H), n
        self.OUT, self.OUTP = OUT, (OUT + 15) // 16 * 16
        rng = np.random.default_rng(seed)
        self.p32 = init_params(act, IN, W, OUT, H)
        self.ph = O.f2h(self.p32)
        self.x = O.f2h(rng.random((n, IN), dtype=np.float32))
        self.xs = np.ascontiguousarray(self.x.T)  # feature-major, what the network kernels read
        dy = np.zeros((n, self.OUTP), np.float32)
        dy[:, :OUT] = rng.standard_normal((n, OUT)).astype(np.float32) * 0.05
        self.dy = O.f2h(dy)
        pre, post, out = forward(act, self.shape, self.ph, self.x, "f64")
        g, dx = backward(act, self.shape, self.ph, self.x, pre, post, self.dy, "f64")
        self.ref = {"f64": dict(pre=pre, post=post, out=out, g=g, dx=dx)}
        # the other accumulation mode ON THE SAME STACKS, layer by layer: what band() holds against the first
        self.ref["f32"] = forward_on(act, self.shape, self.ph, self.x, pre, post, "f32")
        self.ref["f32"]["g"], self.ref["f32"]["dx"] = backward(act, self.shape, self.ph, self.x, pre, post, self.dy, "f32")
        for k, v in self.ref["f64"].items():
            setattr(self, k + "_ref", v)

    def reference_on(self, pre_h, post_h):
        """the float64-mode reference for a side whose stacks are pre_h / post_h: dict(pre, post, out, g, dx)"""
        r = forward_on(self.act, self.shape, self.ph, self.x, pre_h, post_h, "f64")
        r["g"], r["dx"] = backward(self.act, self.shape, self.ph, self.x, pre_h, post_h, self.dy, "f64")
        return r


_cases = {}


def case(act, shape_case, bf16=False):
    """the shared Case, computed once per process (and per 16-bit format: the caller has switched the oracle)"""
    key = (act, tuple(shape_case), bool(bf16))
    if key not in _cases:
        _cases[key] = Case(act, shape_case)
    return _cases[key]


def figures(got, ref):
    """the figures the bars are set on, of `got` = dict(post, pre, out, g, dx) against `ref` of the same form (entries may be missing)"""
    f = {}
    for k in ("post", "pre", "out"):
        if got.get(k) is not None:
            f[k + "_p99"] = float(np.percentile(rae(O.h2f(got[k]), O.h2f(ref[k])), 99))
    if got.get("g") is not None:
        g = got["g"] if got["g"].dtype != np.uint16 else O.h2f(got["g"])
        e = rae(g, ref["g"])
        f["g_p99"], f["g_p999"] = float(np.percentile(e, 99)), float(np.percentile(e, 99.9))
        f["g_rel_l2"] = float(np.linalg.norm(np.asarray(g, np.float64) - ref["g"]) / np.linalg.norm(ref["g"]))
    if got.get("dx") is not None:
        a, b = O.h2f(got["dx"]).astype(np.float64), O.h2f(ref["dx"]).astype(np.float64)
        # allclose(rtol 2e-2, atol 2e-3 max|ref|) as one number: the largest |a - b| / (2e-2 |b| + 2e-3 max|b|); passes where <= 1
        f["dx_allclose"] = float(np.max(np.abs(a - b) / (2e-2 * np.abs(b) + 2e-3 * np.abs(b).max())))
        f["dx_rel_l2"] = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    return f


# the bars of tests/test_emu_mlp_general.py / tests/test_gpu_general_mlp.py, as upper bounds on figures()
BARS_FP16 = {"post_p99": 3e-3, "pre_p99": 3e-3, "out_p99": 3e-3, "g_p99": 3e-3, "g_p999": 1.2e-2, "dx_allclose": 1.0}
BARS_BF16 = {"post_p99": 3e-2, "pre_p99": 3e-2, "out_p99": 3e-2, "g_rel_l2": 2e-2, "dx_rel_l2": 2e-2}


def check(got, ref, bars, fraction=1.0, label=""):
    f = figures(got, ref)
    print(label, {k: f"{v:.3g}" for k, v in f.items()})
    for k, bar in bars.items():
        if k in f:
            assert f[k] < bar * fraction or (k == "dx_allclose" and f[k] <= bar * fraction), (label, k, f[k], bar * fraction)
    return f


def band(c, bars):
    """the two accumulation modes of the restatement against each other: must stay within HALF of every bar used with this case"""
    return check(c.ref["f32"], c.ref["f64"], bars, fraction=0.5, label=f"band {NAMES[c.act]} {c.case}")

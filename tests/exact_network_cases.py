"""Exact-arithmetic cases for the network kernels: inputs on which the order of summation cannot matter.

Every value is a small dyadic rational, chosen so that every fp32 accumulation -- a pre-activation, a backward product, a weight-gradient
entry summed over the batch, a slab of it -- is exact in ANY association order.  Each value a kernel stores in 16 bits is then the rounding
of an exactly known number, and prediction, dL/dinput, weight gradients and (trainer paths) the loss gradient must equal the float64
restatement below in every bit.  Only ReLU / None hidden activations with a None output activation qualify.

This module is a helper, not a test:
  * CASES            one row per kernel path: shape, batch, activation, weight recipe, and (as a comment) the kernels the row reaches;
  * generate()       seeded parameters in the project's layout ([W][IN] | (H-1) x [W][W] | [OUTP][W], row-major), inputs, dL/doutput, targets;
  * restate()        float64 numpy forward / L2 loss gradient / backward / weight gradients, rounding through round16() exactly where the
                     reference rounds: hidden activations, output, loss gradient, every backward activation gradient, dL/dinput, and the
                     weight gradients after the fp32 sum;
  * audit()          the figures of the exactness conditions:
      C1  for every accumulated sum, with g the largest power of two dividing every term of THAT sum (from the data): sum|terms| / g < 2^24.
          A slab is a sub-sum of a weight-gradient entry's terms, so that entry's figure bounds every slab and the sum of the slabs.
      C2  every nonzero value stored in 16 bits is a normal number of the type, before and after rounding.
      C3  in every compared tensor at least 10 % of the nonzero entries are not representable before rounding; at least 90 % of the
          dL/dinput entries and of the weight-gradient entries are nonzero.  (The rows of the output matrix beyond OUT are zero and so is
          dL/doutput there, so their gradients are exact zeros whatever the kernel does right: the share is taken over the other rows,
          and the zero rows are compared like everything else.)

Targets of the in-kernel L2 loss: t = p - delta with p the restated prediction and delta dyadic, so that the loss gradient
2 * loss_scale / (n * OUT) * (p - t) is a coarse dyadic number times (1 - 2^-13) or (1 + 2^-12) in half of the entries: not
representable in 16 bits, rounded to the coarse number by nearest-even (and to its neighbour by a truncating conversion), which keeps
the lattice of everything behind it as coarse as with an external dL/doutput.  p - t is exact in fp32 (audited).
"""
from dataclasses import dataclass, field, replace

import numpy as np


@dataclass(frozen=True)
class Fmt:
    name: str
    p: int      # significant bits
    emin: int   # exponent of the smallest normal number
    emax: int


FP16 = Fmt("fp16", 11, -14, 15)
BF16 = Fmt("bf16", 8, -126, 127)
LOSS_SCALE = 128.0


def round16(v, fmt=FP16, mode="nearest-even"):
    """float64 -> the values of the 16-bit type (as float64).  THE rounding of the restatement: `mode` is "nearest-even" (the reference)
    or "toward-zero" (a sensitivity check)."""
    v = np.asarray(v, np.float64)
    _, e = np.frexp(v)  # |v| in [2^(e-1), 2^e)
    q = np.exp2((np.maximum(e - 1, fmt.emin) - (fmt.p - 1)).astype(np.float64))  # the type's spacing at v
    k = v / q  # exact: a power of two
    k = np.rint(k) if mode == "nearest-even" else np.trunc(k)
    r = k * q
    r = np.where(np.abs(r) >= np.exp2(fmt.emax + 1.0), np.copysign(np.inf, r), r)
    return r + 0.0  # (-0 -> +0: an fp32 sum that starts at +0 never ends at -0)


def to_bits(v, fmt=FP16):
    """values of the 16-bit type -> their uint16 bit patterns"""
    v = np.ascontiguousarray(v, np.float64)
    if fmt is FP16:
        return v.astype(np.float16).view(np.uint16)
    return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b, fmt=FP16):
    b = np.ascontiguousarray(b, np.uint16)
    if fmt is FP16:
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@dataclass(frozen=True)
class Case:
    name: str
    IN: int
    W: int
    OUT: int
    H: int
    n: int = 256
    act: str = "ReLU"
    otype: str = "FullyFusedMLP"
    hidden: tuple = ((0.125, 0.25), 1.0)   # (magnitudes, density) of the input and hidden matrices
    out: tuple = (0.5, 1.0)                # magnitudes of the output matrix, rows < OUT
    dy: tuple = tuple(k / 64.0 for k in range(1, 65))  # magnitudes of the external dL/doutput (and 0), columns < OUT
    trainer: bool = False                  # in-kernel L2 loss: targets instead of dL/doutput
    seed: int = 1

    @property
    def OUTP(self):
        return (self.OUT + 15) // 16 * 16

    @property
    def n_params(self):
        return self.W * self.IN + (self.H - 1) * self.W * self.W + self.OUTP * self.W

    def at(self, n):
        return replace(self, n=n, name=f"{self.name}-n{n}")

    def network(self):
        return {"otype": self.otype, "activation": self.act, "output_activation": "None", "n_neurons": self.W, "n_hidden_layers": self.H}


def _k(denominator, most=None):
    return tuple(k / denominator for k in range(1, (most or denominator) + 1))


D64, D128, D256, D528 = ((0.125, 0.25), 1.0), ((0.125, 0.25), 0.5), ((0.125, 0.25), 0.5), ((0.125, 0.25), 0.25)
DEEP = ((0.5,), 0.125)
# one hidden layer: two matrix products in a row are too few for a sum to outgrow 11 bits on the recipe above, so the values are finer
ONE = dict(hidden=(_k(16), 1.0), out=_k(128), dy=_k(64))
TWO = dict(out=_k(16), dy=_k(8))  # two hidden layers: a finer output matrix, so that the prediction outgrows 11 bits as well
COARSE_DY = dict(dy=(0.5, 1.0))  # three and more hidden layers: every layer refines the lattice of the backward pass by itself

# Module forward / backward through create_network (Identity encoding, nothing to pad).  Each row runs with single-kernel network passes
# on (forward without saved activations, backward = the training kernel with an external dL/doutput, recomputing the activations) and off
# (k_mlp_forward<W, save> -> k_mlp_backward / the layer-by-layer backward); inference takes mlp_forward(hidden == nullptr).
MODULE_CASES = [
    # k_mlp_forward<16>; on: k_mlp_train<16, 0>; off: k_mlp_backward<16, 0>
    Case("fused-16x1", 16, 16, 3, 1, seed=11, **ONE),
    # k_mlp_forward<32>; on: k_mlp_train<32, 2> (48 inputs: no register-resident instance); off: k_mlp_backward<32, 2>
    Case("fused-32x3", 48, 32, 16, 3, hidden=D64, seed=12, **COARSE_DY),
    # inference: k_mlp_infer_wave<64, 32, 1> (fp32 input read by the kernel); forward: k_mlp_forward<64>; on: k_mlp_train_wave<64, 32, 1, external>;
    # off: k_mlp_backward<64, 1>
    Case("fused-64x2", 32, 64, 4, 2, hidden=D64, seed=13, **TWO),
    # inference: k_mlp_infer_wave<64, 64, 1>; on: k_mlp_train_wave<64, 64, 1, external> (one wave per SIMD); off: k_mlp_backward<64, 1>
    Case("fused-64x2-in64", 64, 64, 16, 2, hidden=D64, seed=14, **TWO),
    # the workgroup-tiled instances: k_mlp_forward<64>; on: k_mlp_train<64, 3>; off: k_mlp_backward<64, 3>
    Case("fused-64x4", 32, 64, 4, 4, hidden=D128, seed=15, **COARSE_DY),
    # k_mlp_forward<128>; on: k_mlp_train_wide<3> (weights resident in LDS, transpose reads); off: k_mlp_backward<128, 3>
    Case("fused-128x4", 32, 128, 16, 4, hidden=D128, seed=16, **COARSE_DY),
    # 128 inputs: k_mlp_forward<64>; on: k_mlp_train<64, 1>; off: k_mlp_backward<64, 1>
    Case("fused-64x2-in128", 128, 64, 5, 2, hidden=D128, seed=17, **TWO),
    # deeper than the register-resident kernels, on and off: k_mlp_forward<W, save> -> k_mlp_backward_chain<W> + k_mlp_weight_gradient<W> per matrix
    Case("deep-64x6", 32, 64, 4, 6, act="None", hidden=DEEP, seed=18, **COARSE_DY),
    Case("deep-128x8", 32, 128, 8, 8, act="None", hidden=((0.5,), 0.0625), seed=19, **COARSE_DY),
]

# The layer-by-layer network (mlp_general.hip): one k_general_layer launch per layer and direction, the weight gradients in batch-sliced
# slabs summed in fixed order.  n = 768: more than one slab, and the slab count does not divide the stages evenly.
GENERAL_SHAPES = [
    Case("general-48x1", 16, 48, 3, 1, otype="CutlassMLP", seed=21, **ONE),
    Case("general-96x3", 80, 96, 40, 3, otype="CutlassMLP", hidden=D128, seed=22, **COARSE_DY),
    Case("general-256x2", 32, 256, 4, 2, otype="CutlassMLP", hidden=D256, seed=23, **TWO),
    Case("general-528x2", 64, 528, 4, 2, otype="CutlassMLP", hidden=D528, seed=24, **TWO),
    Case("general-64x2-130-outputs", 32, 64, 130, 2, otype="CutlassMLP", hidden=D64, seed=25, **TWO),  # more than 128 outputs: layer by layer at a fused width
]
GENERAL_CASES = [c.at(n) for c in GENERAL_SHAPES for n in (256, 768)]

# Trainer paths with the in-kernel L2 loss (create_from_config with an Identity encoding, training_step(run_optimizer=False, dL_dinput=...)),
# each with the network kernel reading the fp32 input itself (set_fused_identity_input) and behind the encoding kernel; n = 1024: several
# tiles per workgroup, several workgroups.
TRAINER_SHAPES = [
    # k_mlp_train_wave<64, 32, 1> (32 inputs: always behind the encoding kernel); forward() + backward(): k_mlp_forward<64> -> k_loss -> k_mlp_train_wave<.., external>
    Case("trainer-64x2", 32, 64, 4, 2, hidden=D64, trainer=True, seed=31, **TWO),
    # k_mlp_train_wave<64, 64, 1, .., f32 input> (one wave per SIMD) / the same kernel on the encoded matrix
    Case("trainer-64x2-in64", 64, 64, 4, 2, hidden=D64, trainer=True, seed=32, **TWO),
    # k_mlp_train_wave<64, 64, 0, .., f32 input>, 16 outputs: the instance with a loss over all output columns
    Case("trainer-64x1-in64", 64, 64, 16, 1, trainer=True, seed=33, **ONE),
    # k_mlp_train_wide<3> / k_mlp_train_wide<0>: the LDS-resident kernel
    Case("trainer-128x4", 32, 128, 16, 4, hidden=D128, trainer=True, seed=34, **COARSE_DY),
    Case("trainer-128x1", 64, 128, 4, 1, trainer=True, seed=35, **ONE),
]
TRAINER_CASES = [c.at(n) for c in TRAINER_SHAPES for n in (256, 1024)]
# the fused training kernels behind a module's backward at n = 1024
MODULE_CASES_1024 = [c.at(1024) for c in MODULE_CASES if c.name in ("fused-64x2", "fused-64x2-in64", "fused-64x4", "fused-128x4")]
# the bfloat16 build: module forward / backward of 64 x 2 and 128 x 4
BF16_CASES = [c for c in MODULE_CASES if c.name in ("fused-64x2", "fused-128x4")]

CASES = MODULE_CASES + MODULE_CASES_1024 + GENERAL_CASES + TRAINER_CASES


def by_name(name):
    return next(c for c in CASES if c.name == name)


def _draw(rng, shape, magnitudes, density=1.0):
    v = rng.choice(np.asarray(magnitudes, np.float64), size=shape) * rng.choice([-1.0, 1.0], size=shape)
    return v * (rng.random(shape) < density)


@dataclass
class Data:
    params: np.ndarray            # float64 [n_params]
    x: np.ndarray                 # float64 [n][IN]
    dy: np.ndarray = None         # float64 [n][OUTP], module cases
    wanted_dout: np.ndarray = None  # float64 [n][OUT], trainer cases: the loss gradient before its rounding
    targets: np.ndarray = None    # float32 [n][OUT], trainer cases (filled by with_targets)


def matrices(case, params):
    """the weight matrices as views of the flat parameter vector, input matrix first"""
    IN, W, H = case.IN, case.W, case.H
    mats, off = [], 0
    for rows, cols in [(W, IN)] + [(W, W)] * (H - 1) + [(case.OUTP, W)]:
        mats.append(params[off:off + rows * cols].reshape(rows, cols))
        off += rows * cols
    return mats


def generate(case, fmt=FP16, x=None):
    rng = np.random.default_rng(case.seed * 7919 + case.n)
    params = np.zeros(case.n_params)
    mats = matrices(case, params)
    for m in mats[:-1]:
        m[...] = _draw(rng, m.shape, *case.hidden)
    mats[-1][:case.OUT] = _draw(rng, (case.OUT, case.W), case.out)
    if x is None:
        x = rng.integers(-1, 2, size=(case.n, case.IN)).astype(np.float64)
    d = Data(params, np.asarray(x, np.float64))
    if case.trainer:
        coarse = _draw(rng, (case.n, case.OUT), case.dy, 0.9)
        tilt = rng.choice([1.0, 1.0 - 2.0 ** -13, 1.0 + 2.0 ** -12], p=[0.5, 0.35, 0.15], size=coarse.shape)
        d.wanted_dout = coarse * tilt
        p = restate(case, d, fmt, forward_only=True).out[:, :case.OUT]
        factor = 2.0 * LOSS_SCALE / (case.n * case.OUT)
        assert np.log2(factor) == np.rint(np.log2(factor)), "n * OUT must be a power of two"
        t = p - d.wanted_dout / factor
        d.targets = t.astype(np.float32)
        assert np.array_equal(d.targets.astype(np.float64), t), "targets are fp32 numbers"
    else:
        d.dy = np.zeros((case.n, case.OUTP))
        d.dy[:, :case.OUT] = _draw(rng, (case.n, case.OUT), case.dy, 0.9)
    return d


@dataclass
class Result:
    out: np.ndarray = None
    hidden: list = field(default_factory=list)
    dout: np.ndarray = None
    dinput: np.ndarray = None
    grads: np.ndarray = None
    stored: list = field(default_factory=list)   # (name, before rounding, after): everything that is stored in 16 bits
    sums: list = field(default_factory=list)     # (name, A, B): the sums S[i][o] = sum_k A[i][k] * B[o][k]
    f32: list = field(default_factory=list)      # values that must be fp32 numbers (the loss gradient's arithmetic)

    def compared(self, case):
        names = ["out", "dinput", "grads"] + (["dout"] if case.trainer else [])
        return {k: getattr(self, k) for k in names}


def restate(case, data, fmt=FP16, mode="nearest-even", drop_last=0, swap=None, forward_only=False):
    """The reference's network in float64.  drop_last: leave the last samples out of the weight-gradient sums; swap = (matrix, k0, k1): two K
    indices of a weight matrix exchanged (sensitivity checks)."""
    r16 = lambda v: round16(v, fmt, mode)  # noqa: E731
    res = Result()
    params = data.params
    if swap is not None:
        params = params.copy()
        m = matrices(case, params)[swap[0]]
        m[:, [swap[1], swap[2]]] = m[:, [swap[2], swap[1]]]
    mats = matrices(case, params)
    relu = case.act == "ReLU"
    a = data.x
    acts = [a]
    for l in range(case.H):
        res.sums.append((f"pre-activation {l}", a, mats[l]))
        pre = a @ mats[l].T
        pre = np.maximum(pre, 0.0) if relu else pre
        a = r16(pre)
        res.stored.append((f"hidden {l}", pre, a))
        acts.append(a)
    res.hidden = acts[1:]
    res.sums.append(("output", a, mats[-1]))
    pre = a @ mats[-1].T
    res.out = r16(pre)
    res.stored.append(("out", pre, res.out))
    if forward_only:
        return res
    if case.trainer:  # l2.h: gradient = 2 * (p - t); dL/doutput = (T)(loss_scale * gradient / n_total), zero in the padded columns
        diff = res.out[:, :case.OUT] - data.targets.astype(np.float64)
        g = LOSS_SCALE * (2.0 * diff) / (case.n * case.OUT)
        res.f32 += [diff, g]
        res.dout = np.zeros((case.n, case.OUTP))
        res.dout[:, :case.OUT] = r16(g)
        res.stored.append(("dout", g, res.dout[:, :case.OUT]))
    else:
        res.dout = data.dy
    keep = case.n - drop_last
    d = res.dout
    grads = [None] * len(mats)
    for l in range(case.H, -1, -1):  # matrix l maps acts[l] to layer l
        res.sums.append((f"weight gradient {l}", d[:keep].T, acts[l][:keep].T))
        grads[l] = d[:keep].T @ acts[l][:keep]
        res.sums.append((f"backward product {l}", d, mats[l].T))
        back = d @ mats[l]
        if l > 0:
            back = np.where(acts[l] > 0.0, back, 0.0) if relu else back
            d = r16(back)
            res.stored.append((f"dL/dhidden {l - 1}", back, d))
        else:
            res.dinput = r16(back)
            res.stored.append(("dinput", back, res.dinput))
    pre = np.concatenate([g.reshape(-1) for g in grads])
    res.grads = r16(pre)
    res.stored.append(("grads", pre, res.grads))
    return res


def _valuation(a):
    """exponent of the lowest set bit of every entry (entries that are zero: meaningless, masked by the caller)"""
    m, e = np.frexp(np.abs(a))
    mant = (m * 2.0 ** 53).astype(np.int64)
    low = mant & -mant
    return (e - 53 + np.rint(np.log2(np.maximum(low, 1).astype(np.float64)))).astype(np.int64)


def c1_figure(A, B):
    """worst sum|terms| / g over the sums S[i][o] = sum_k A[i][k] * B[o][k], g = the largest power of two dividing every term of the sum"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    total = np.abs(A) @ np.abs(B).T
    va, vb = _valuation(A), _valuation(B)
    g = np.full(total.shape, np.iinfo(np.int64).max)
    for p in np.unique(va[A != 0]):
        ia = ((va == p) & (A != 0)).astype(np.float32)
        for q in np.unique(vb[B != 0]):
            ib = ((vb == q) & (B != 0)).astype(np.float32)
            g = np.where(ia @ ib.T > 0, np.minimum(g, p + q), g)  # some k has a term whose lowest bit is 2^(p+q)
    some = total > 0
    if not some.any():
        return 0.0
    return float(np.max(total[some] / np.exp2(g[some].astype(np.float64))))


def audit(case, data, fmt=FP16, res=None):
    """the C1 - C3 figures of a case (on the restatement alone)"""
    res = res or restate(case, data, fmt)
    fig = {"c1": {}, "c3_rounded": {}, "c3_nonzero": {}}
    for name, A, B in res.sums:
        key = name.rstrip(" 0123456789")
        fig["c1"][key] = max(fig["c1"].get(key, 0.0), c1_figure(A, B))
    fig["c1_log2"] = float(np.log2(max(fig["c1"].values())))
    lo, hi = 2.0 ** fmt.emin, 2.0 ** (fmt.emax + 1)
    tensors = [("params", data.params, data.params), ("x", data.x, data.x)] + res.stored
    if data.dy is not None:
        tensors.append(("dy", data.dy, data.dy))
    fig["c2"] = all(np.all((v == 0) | ((np.abs(v) >= lo) & (np.abs(v) < hi))) for _, pre, post in tensors for v in (pre, post))
    fig["inputs_are_16_bit"] = all(np.array_equal(round16(v, fmt), v) for v in (data.params, data.x) + (() if data.dy is None else (data.dy,)))
    fig["f32_exact"] = all(np.array_equal(v.astype(np.float32).astype(np.float64), v) for v in res.f32)
    before = {name: pre for name, pre, _ in res.stored}
    live = np.ones(case.n_params, bool)
    live[case.n_params - (case.OUTP - case.OUT) * case.W:] = False  # the zero rows of the output matrix
    for name in res.compared(case):
        pre = before[name]
        nz = pre != 0
        fig["c3_rounded"][name] = float(np.mean(round16(pre[nz], fmt) != pre[nz])) if nz.any() else 0.0
    fig["c3_nonzero"]["dinput"] = float(np.mean(res.dinput != 0))
    fig["c3_nonzero"]["grads"] = float(np.mean(res.grads[live] != 0))
    fig["padding_gradients_zero"] = bool(np.all(res.grads[~live] == 0)) and bool(np.all(res.out[:, case.OUT:] == 0))
    return fig


def audit_passes(fig):
    return (fig["c1_log2"] < 24 and fig["c2"] and fig["inputs_are_16_bit"] and fig["f32_exact"] and fig["padding_gradients_zero"]
            and min(fig["c3_rounded"].values()) >= 0.10 and min(fig["c3_nonzero"].values()) >= 0.90)


def describe(case, fig):
    r = ", ".join(f"{k} {100 * v:.0f} %" for k, v in fig["c3_rounded"].items())
    return f"{case.name}: C1 2^{fig['c1_log2']:.1f}, rounded: {r}, nonzero: dinput {100 * fig['c3_nonzero']['dinput']:.0f} %, grads {100 * fig['c3_nonzero']['grads']:.0f} %"


def mismatch(name, got_bits, want_bits):
    """'' if the two uint16 (or uint32) arrays are equal, else the tensor, the number of differing entries and the first few (index, got, want)"""
    got_bits, want_bits = np.asarray(got_bits), np.asarray(want_bits)
    if got_bits.shape != want_bits.shape:
        return f"{name}: shape {got_bits.shape} != {want_bits.shape}"
    if np.array_equal(got_bits, want_bits):
        return ""
    idx = np.argwhere(got_bits != want_bits)
    first = "; ".join(f"{tuple(int(j) for j in i)}: got 0x{int(got_bits[tuple(i)]):04x} want 0x{int(want_bits[tuple(i)]):04x}" for i in idx[:8])
    return f"{name}: {len(idx)} of {got_bits.size} entries differ; first: {first}"

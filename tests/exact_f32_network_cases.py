"""Exact-arithmetic cases for the fp32 network kernels (csrc/mlp_general_fp32.hip), after the method of tests/exact_network_cases.py.

Every weight, input and output gradient is a small dyadic rational, chosen so that EVERY product and EVERY partial sum of the passes -- a
pre-activation, a backward product, a weight-gradient entry summed over the batch, any slab of it, the sum of the slabs -- is an fp32 number
in any association order.  An fp32 network rounds nowhere else (no 16-bit store between the layers), so prediction, dL/dinput and the
weight gradients must equal the float64 evaluation below, cast to float32, in every bit.  Only ReLU / None hidden activations with a None
output activation qualify.

Helper, not a test:
  * CASES       the shapes: the smallest at which a tile, a K stage or a slab can go missing.  The layer kernel stages K in steps of
                Gen<float>::BK = 32 floats and tiles m in blocks of 16 * {1..4}; the weight-gradient kernel works on 64 x 64 tiles and stages of 32
                samples.  Hidden width 16: a single tile; 48: not a power of two, one and a half K stages; 272: eight full K stages plus a
                ragged one (272 = 8 * 32 + 16), m tiles of 48 with a ragged last one, four full weight-gradient tiles and a ragged fifth.
                Inputs 16 and 80 (two and a half K stages), outputs 3 (padded to 16) and 144 (> 128, three weight-gradient tiles), 1 and 3
                hidden layers, n = 256 and 768 (more than one batch slice, an odd number of 128-sample workgroup rows).
  * generate()  seeded parameters in the project's layout, inputs, dL/doutput (exact_network_cases.generate)
  * restate()   the network in float64, nothing rounded
  * audit()     per case, from the data:
      C1  for every accumulated sum, with g the largest power of two dividing every term of THAT sum: sum|terms| / g < 2^24 -- every
          partial sum in any order is then a multiple of g below 2^24 g, an fp32 number.  A slab is a sub-sum of a weight-gradient entry's
          terms, so the entry's figure bounds every slab and the sum of the slabs.  Accumulate adds the buffer as one more term.
      C2  every input, every stored activation and every compared value is an fp32 number (float64 -> float32 -> float64 is the identity)
          and a normal one or zero.
      C3  at least 90 % of the dL/dinput entries and of the weight-gradient entries (outside the zero rows of the output matrix) are
          nonzero, and in every compared tensor at least 10 % of the nonzero entries are NOT fp16 numbers: bits a 16-bit path would lose.
"""
from dataclasses import replace

import numpy as np

import exact_network_cases as E

Case, matrices, mismatch = E.Case, E.matrices, E.mismatch

_F = dict(otype="CutlassMLP")
# magnitudes / densities: one hidden layer can afford fine values; with three, every layer refines the lattice by itself and multiplies
# the magnitudes, so the hidden weights are +-1/4, +-1/2 and +-1, sparse in the wide matrices, and the output side is coarser
FINE = dict(hidden=(E._k(16), 1.0), out=E._k(128), dy=E._k(64))
WIDE_ONE = dict(hidden=((0.125, 0.25, 0.5), 0.5), out=E._k(64), dy=E._k(64))
DEEP_48 = dict(hidden=((0.25, 0.5, 1.0), 0.25), out=E._k(8), dy=E._k(4))
DEEP_272 = dict(hidden=((0.25, 0.5, 1.0), 0.0625), out=E._k(16), dy=E._k(16))

SHAPES = [
    Case("f32-16x1", 16, 16, 3, 1, seed=41, **_F, **FINE),
    Case("f32-48x3", 80, 48, 144, 3, seed=42, **_F, **DEEP_48),
    Case("f32-272x1-linear", 16, 272, 144, 1, act="None", seed=43, **_F, **WIDE_ONE),
    Case("f32-272x3", 80, 272, 3, 3, seed=44, **_F, **DEEP_272),
]
CASES = [c.at(n) for c in SHAPES for n in (256, 768)]
CASES_256 = [c for c in CASES if c.n == 256]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def generate(case):
    """parameters, inputs in {-1, 0, 1} and dL/doutput of the case (exact_network_cases.generate: the padded output rows and columns zero),
    plus a non-zero dyadic buffer to accumulate the weight gradients into"""
    data = E.generate(case)
    rng = np.random.default_rng(case.seed * 104729 + case.n)
    data.grads_init = rng.integers(-8, 9, size=case.n_params).astype(np.float64) / 4.0
    return data


def restate(case, data, forward_only=False):
    """float64, nothing rounded -> E.Result with out [n][OUTP], hidden, dinput [n][IN], grads [n_params] and the sums the audit figures"""
    res = E.Result()
    mats = matrices(case, data.params)
    relu = case.act == "ReLU"
    a = data.x
    acts = [a]
    for l in range(case.H):
        res.sums.append((f"pre-activation {l}", a, mats[l]))
        pre = a @ mats[l].T
        a = np.maximum(pre, 0.0) + 0.0 if relu else pre
        res.stored.append((f"hidden {l}", pre, a))
        acts.append(a)
    res.hidden = acts[1:]
    res.sums.append(("output", a, mats[-1]))
    res.out = a @ mats[-1].T
    res.stored.append(("out", res.out, res.out))
    if forward_only:
        return res
    d = res.dout = data.dy
    grads = [None] * len(mats)
    for l in range(case.H, -1, -1):  # matrix l maps acts[l] to layer l
        res.sums.append((f"weight gradient {l}", d.T, acts[l].T))
        grads[l] = d.T @ acts[l]
        res.sums.append((f"backward product {l}", d, mats[l].T))
        back = d @ mats[l]
        if l > 0:
            d = np.where(acts[l] > 0.0, back, 0.0) if relu else back
            res.stored.append((f"dL/dhidden {l - 1}", back, d))
        else:
            res.dinput = back
            res.stored.append(("dinput", back, back))
    res.grads = np.concatenate([g.reshape(-1) for g in grads])
    res.stored.append(("grads", res.grads, res.grads))
    res.grads_accumulated = data.grads_init + res.grads
    res.stored.append(("grads accumulated", res.grads_accumulated, res.grads_accumulated))
    return res


def _is_f32(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        back = v.astype(np.float32).astype(np.float64)
    return bool(np.array_equal(back, v)) and bool(np.all((v == 0) | (np.abs(v) >= 2.0 ** -126)))


def _not_fp16_share(v):
    v = np.asarray(v, np.float64)
    nz = v[v != 0]
    if nz.size == 0:
        return 0.0
    with np.errstate(over="ignore"):
        return float(np.mean(nz.astype(np.float16).astype(np.float64) != nz))


def audit(case, data, res=None):
    res = res or restate(case, data)
    fig = {"c1": {}}
    for name, A, B in res.sums:
        key = name.rstrip(" 0123456789")
        fig["c1"][key] = max(fig["c1"].get(key, 0.0), E.c1_figure(A, B))
    # Accumulate: the buffer is one more term of every weight-gradient sum (its lowest bit is 2^-2 or coarser, every entry at most 2)
    g = res.grads
    terms = np.abs(g) + np.abs(data.grads_init)
    unit = np.exp2(np.minimum(E._valuation(np.where(g != 0, g, 1.0)), -2).astype(np.float64))
    fig["c1"]["accumulate"] = float(np.max(terms / unit))
    fig["c1_log2"] = float(np.log2(max(fig["c1"].values())))
    tensors = [data.params, data.x, data.dy, data.grads_init] + [v for _, pre, post in res.stored for v in (pre, post)]
    fig["c2"] = all(_is_f32(v) for v in tensors)
    live = np.ones(case.n_params, bool)
    live[case.n_params - (case.OUTP - case.OUT) * case.W:] = False  # the zero rows of the output matrix
    fig["c3_nonzero"] = {"dinput": float(np.mean(res.dinput != 0)), "grads": float(np.mean(res.grads[live] != 0))}
    fig["c3_not_fp16"] = {"out": _not_fp16_share(res.out), "dinput": _not_fp16_share(res.dinput), "grads": _not_fp16_share(res.grads)}
    fig["padding_zero"] = bool(np.all(res.grads[~live] == 0)) and bool(np.all(res.out[:, case.OUT:] == 0))
    return fig


def audit_passes(fig):
    return (fig["c1_log2"] < 24 and fig["c2"] and fig["padding_zero"] and min(fig["c3_nonzero"].values()) >= 0.90
            and min(fig["c3_not_fp16"].values()) >= 0.10)


def describe(case, fig):
    return (f"{case.name}: C1 2^{fig['c1_log2']:.1f} ({', '.join(f'{k} 2^{np.log2(max(v, 1)):.1f}' for k, v in fig['c1'].items())}), "
            f"nonzero {fig['c3_nonzero']}, not fp16 {fig['c3_not_fp16']}")


def bits32(v):
    """float64 values that are fp32 numbers -> their uint32 bit patterns (-0 never occurs: sums that start at +0)"""
    return np.ascontiguousarray(np.asarray(v, np.float64) + 0.0).astype(np.float32).view(np.uint32)


def with_n(case, n):
    return replace(case, n=n)

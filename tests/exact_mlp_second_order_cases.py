"""Exact-arithmetic cases for the second-order pass of the fp32 network (csrc/mlp_general_fp32.hip mlp_f32_backward_backward), after
tests/exact_f32_network_cases.py: the same shapes, parameters, inputs and dL/doutput, plus v = dL/d(dL/dinput) with dyadic entries in
{-1, -1/2, 0, 1/2, 1}.  With ReLU / None hidden activations and no output activation nothing curves: the pass is the tangent pass, the
first-order recomputation and the d (x) u weight-gradient products, dL/dinput is zero, and every sum is an fp32 number in any association
order -- so dL/d(dL/doutput) and the weight gradients must equal the float64 restatement, cast to float32, in every bit.

Helper, not a test:
  * CASES      exact_f32_network_cases.CASES (16 / 48 / 272 wide, 3 and 144 outputs, n = 256 and 768: ragged tiles, several slabs)
  * generate() that module's data plus v
  * restate()  tests/second_order_mlp_reference.second_order in float64 -> the three results and every sum the audit figures
  * audit()    C1 - C3 as in that module, over the NEW sums: every t (tangent product), every e (backward product of the recomputation) and
               every d (x) u weight-gradient entry; C2 over v and everything stored; C3 over dL/d(dL/doutput) and the weight gradients.
"""
import numpy as np

import exact_f32_network_cases as F
import exact_network_cases as E
import second_order_mlp_reference as R

CASES, CASES_256 = F.CASES, F.CASES_256
matrices, mismatch, bits32, by_name = F.matrices, F.mismatch, F.bits32, F.by_name


def generate(case):
    data = F.generate(case)
    rng = np.random.default_rng(case.seed * 15485863 + case.n)
    data.v = rng.integers(-2, 3, size=(case.n, case.IN)).astype(np.float64) / 2.0
    return data


class Result:
    pass


def restate(case, data):
    """float64, nothing rounded"""
    mats = matrices(case, data.params)
    res = Result()
    res.ddy, res.dinput, res.grads, p = R.second_order(np.float64, mats, data.x, data.dy, data.v, case.act, "None")
    H = case.H
    res.sums, res.stored = [], [("v", data.v)]
    for j in range(H):
        res.sums.append((f"tangent product {j}", p["u"][j - 1] if j > 0 else data.v, mats[j]))
        res.sums.append((f"backward product {j}", p["d"][j + 1] if j + 1 < H else p["g"], mats[j + 1].T))
        res.sums.append((f"weight gradient {j}", p["d"][j].T, (p["u"][j - 1] if j > 0 else data.v).T))
        res.stored += [(f"t {j}", p["t"][j]), (f"u {j}", p["u"][j]), (f"e {j}", p["e"][j]), (f"d {j}", p["d"][j])]
    res.sums.append(("tangent product out", p["u"][H - 1], mats[H]))
    res.sums.append((f"weight gradient {H}", p["g"].T, p["u"][H - 1].T))
    res.stored += [("dL/d(dL/doutput)", res.ddy), ("weight gradients", res.grads), ("dL/dinput", res.dinput)]
    res.curvature_is_zero = all(float(np.abs(c).max()) == 0.0 for c in p["c"] + [p["c_out"]])
    return res


def audit(case, data, res=None):
    res = res or restate(case, data)
    fig = {"c1": {}}
    for name, A, B in res.sums:
        key = name.rstrip(" 0123456789").replace(" out", "")
        fig["c1"][key] = max(fig["c1"].get(key, 0.0), E.c1_figure(A, B))
    fig["c1_log2"] = float(np.log2(max(fig["c1"].values())))
    fig["c2"] = all(F._is_f32(v) for _, v in res.stored)
    live = np.ones(case.n_params, bool)
    live[case.n_params - (case.OUTP - case.OUT) * case.W:] = False  # the zero rows of the output matrix
    fig["c3_nonzero"] = {"ddy": float(np.mean(res.ddy[:, :case.OUT] != 0)), "grads": float(np.mean(res.grads[live] != 0))}
    fig["c3_not_fp16"] = {"ddy": F._not_fp16_share(res.ddy), "grads": F._not_fp16_share(res.grads)}
    fig["padding_zero"] = bool(np.all(res.grads[~live] == 0)) and bool(np.all(res.ddy[:, case.OUT:] == 0))
    fig["no_curvature"] = res.curvature_is_zero and bool(np.all(res.dinput == 0))
    return fig


def audit_passes(fig):
    return (fig["c1_log2"] < 24 and fig["c2"] and fig["padding_zero"] and fig["no_curvature"] and min(fig["c3_nonzero"].values()) >= 0.90
            and min(fig["c3_not_fp16"].values()) >= 0.10)


def describe(case, fig):
    return (f"{case.name}: C1 2^{fig['c1_log2']:.1f} ({', '.join(f'{k} 2^{np.log2(max(v, 1)):.1f}' for k, v in fig['c1'].items())}), "
            f"nonzero {fig['c3_nonzero']}, not fp16 {fig['c3_not_fp16']}")

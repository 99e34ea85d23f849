"""The second-order pass of the fp32 network (csrc/mlp_general_fp32.hip mlp_f32_backward_backward) on the host SIMT emulator, no GPU.
  * The audit that makes the bit comparison legitimate, for every case of tests/exact_mlp_second_order_cases.py including the n = 768
    ones that only the GPU runs.
  * The exact cases at n = 256: dL/d(dL/doutput) and the weight gradients np.array_equal on bit patterns to the float64 restatement cast to
    float32, dL/dinput all zeros; and with single results asked for, the same bits.
  * The smooth activations (Tanh, Softplus, Sine, SiLU; Tanh also under a Sigmoid output) at 16 -> 48 x 2 -> 3, n = 256, where the
    curvature launches run: under the rule of tests/test_gpu_f32_network.py -- the emulator may exceed the CPU float32 restatement's own
    error against float64 on the same inputs by FACTOR = 8."""
import numpy as np
import pytest

import exact_mlp_second_order_cases as X
import second_order_mlp_reference as R

emu_so = pytest.importorskip("emu_mlp_second_order")
pytestmark = pytest.mark.skipif(not emu_so.available(), reason="no host compiler for the emulator")

ACT = {"None": 0, "ReLU": 1, "LeakyReLU": 2, "Exponential": 3, "Sigmoid": 4, "Squareplus": 5, "Softplus": 6, "Tanh": 7, "SiLU": 8, "Sine": 9}
FACTOR = 8.0


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(case):
        if case.name not in cache:
            data = X.generate(case)
            cache[case.name] = (data, X.restate(case, data))
        return cache[case.name]
    return get


@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_every_new_sum_of_the_case_is_exact_in_fp32(built, case):
    data, res = built(case)
    fig = X.audit(case, data, res)
    assert X.audit_passes(fig), X.describe(case, fig)


def test_the_audit_notices_an_inexact_sum(built):
    """sensitivity: the same case with a fine v fails C1"""
    case = X.by_name("f32-48x3-n768")
    data = X.generate(case)
    data.v = data.v + np.random.default_rng(1).integers(1, 4096, size=data.v.shape) / 4096.0
    assert not X.audit_passes(X.audit(case, data))


def check(*pairs):
    report = [X.mismatch(name, got, want) for name, got, want in pairs]
    assert not any(report), "\n".join(r for r in report if r)


@pytest.mark.parametrize("case", X.CASES_256, ids=[c.name for c in X.CASES_256])
def test_exact_cases_on_the_emulator(built, case):
    data, res = built(case)
    m = emu_so.meta(case.IN, case.W, case.OUTP, case.H, ACT[case.act])
    assert not emu_so.has_curvature(m)
    params, x_fm, v_fm, dy = data.params.astype(np.float32), np.ascontiguousarray(data.x.T, np.float32), np.ascontiguousarray(data.v.T, np.float32), data.dy.astype(np.float32)
    hidden, _ = emu_so.forward(m, params, x_fm)
    ddy, dinput, grads = emu_so.backward_backward(m, params, x_fm, hidden, v_fm, dy)
    check(("dL/d(dL/doutput)", ddy.view(np.uint32), X.bits32(res.ddy)), ("weight gradients", grads.view(np.uint32), X.bits32(res.grads)))
    assert not dinput.view(np.uint32).any(), "dL/dinput of a network without curvature is +0 everywhere"
    # single results: only the launches they need, the same bits
    only_ddy, _, _ = emu_so.backward_backward(m, params, x_fm, hidden, v_fm, None, want_dinput=False, want_grads=False)
    _, only_dinput, _ = emu_so.backward_backward(m, params, x_fm, hidden, v_fm, dy, want_ddy=False, want_grads=False)
    _, _, only_grads = emu_so.backward_backward(m, params, x_fm, hidden, v_fm, dy, want_ddy=False, want_dinput=False)
    check(("dL/d(dL/doutput) alone", only_ddy.view(np.uint32), X.bits32(res.ddy)), ("weight gradients alone", only_grads.view(np.uint32), X.bits32(res.grads)))
    assert not only_dinput.view(np.uint32).any()


def test_workspace_per_sample():
    """floats per sample: 2 (u, d) or 4 (t, e as well) matrices per hidden layer, 2 or 3 output-wide ones"""
    assert emu_so.workspace_floats(emu_so.meta(16, 48, 16, 2, ACT["ReLU"]), 256) == 256 * (2 * 2 * 48 + 2 * 16)
    assert emu_so.workspace_floats(emu_so.meta(16, 48, 16, 2, ACT["Tanh"]), 256) == 256 * (4 * 2 * 48 + 3 * 16)
    assert emu_so.workspace_floats(emu_so.meta(16, 48, 16, 2, ACT["ReLU"], ACT["Sigmoid"]), 256) == 256 * (4 * 2 * 48 + 3 * 16)


SMOOTH = [("Tanh", "None"), ("Softplus", "None"), ("Sine", "None"), ("SiLU", "None"), ("Tanh", "Sigmoid"), ("ReLU", "Sigmoid")]


@pytest.mark.parametrize("hidden_act,output_act", SMOOTH, ids=[f"{h}-{o}" for h, o in SMOOTH])
def test_smooth_activations_on_the_emulator(hidden_act, output_act):
    IN, W, H, OUT, OUTP, n = 16, 48, 2, 3, 16, 256
    rng = np.random.default_rng(2026)
    mats = []
    for rows, cols in [(W, IN)] + [(W, W)] * (H - 1) + [(OUTP, W)]:
        s = np.sqrt(6.0 / (rows + cols))
        mats.append(rng.uniform(-s, s, size=(rows, cols)).astype(np.float32))
    mats[-1][OUT:] = 0
    x = rng.uniform(-1, 1, size=(n, IN)).astype(np.float32)
    dy = np.zeros((n, OUTP), np.float32)
    dy[:, :OUT] = rng.uniform(-1, 1, size=(n, OUT))
    v = rng.uniform(-1, 1, size=(n, IN)).astype(np.float32)
    ref, cpu_error = R.errors(mats, x, dy, v, hidden_act, output_act)
    m = emu_so.meta(IN, W, OUTP, H, ACT[hidden_act], ACT[output_act])
    assert emu_so.has_curvature(m)
    params, x_fm, v_fm = np.concatenate([a.reshape(-1) for a in mats]), np.ascontiguousarray(x.T), np.ascontiguousarray(v.T)
    hidden, _ = emu_so.forward(m, params, x_fm)
    ddy, dinput_fm, grads = emu_so.backward_backward(m, params, x_fm, hidden, v_fm, dy)
    report = []
    for name, got, want, e in zip(("dL/d(dL/doutput)", "dL/dinput", "parameter gradients"), (ddy, dinput_fm.T, grads), ref, cpu_error):
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{hidden_act}/{output_act} {name}: emulator max error {err:.3e}, CPU float32 {e:.3e}, bar {FACTOR * e:.3e}, max |reference| {np.abs(want).max():.3e}")
        assert np.isfinite(got).all()
        if not err <= FACTOR * e:
            report.append(f"{name}: emulator max error {err:.3e} exceeds {FACTOR} x the CPU float32 error {e:.3e}")
    assert not report, "; ".join(report)
    # asked for alone, each result has the same bits
    only_dinput = emu_so.backward_backward(m, params, x_fm, hidden, v_fm, dy, want_ddy=False, want_grads=False)[1]
    only_grads = emu_so.backward_backward(m, params, x_fm, hidden, v_fm, dy, want_ddy=False, want_dinput=False)[2]
    assert np.array_equal(only_dinput.view(np.uint32), dinput_fm.view(np.uint32)) and np.array_equal(only_grads.view(np.uint32), grads.view(np.uint32))

"""The fused fp32 network kernels (csrc/mlp_f32_fused.hip, mlp_f32_fused_backward.hip, mlp_f32_fused_device.h,
mlp_f32_fused_second_order.hip) on the host SIMT emulator, no GPU.  The emulator's build has two persistent workgroups
(-DTCNN_F32F_MAX_BLOCKS=2), so batches of three and five sample tiles run the tile loop in uneven shares.

  a. The exact cases of tests/exact_f32_fused_cases.py, every one audited first (C1 - C3 of tests/exact_f32_network_cases.py, and of
     tests/exact_mlp_second_order_cases.py for the second-order pass: every float64 result is an fp32 number): inference, the saving
     forward pass with its whole stack, trimmed inference in both layouts, dL/dinput, weight gradients (Overwrite, Accumulate), each result
     asked for alone, dL/d(dL/doutput) and the second-order weight gradients -- np.array_equal on bit patterns against the float64
     restatement cast to float32, and against the emulated layer-by-layer kernels on the same arguments.
  b. Staged weights: 128 -> 64 x 6 -> 16 does not fit the resident LDS budget in the forward pass and in the backward chain WITH dL/dinput,
     and fits in the chain without it; at n = 768 workgroup 0 stages every matrix a second time for its second tile.  Held to the bar of
     tests/test_gpu_f32_network.py (FACTOR x the error of a numpy float32 restatement against float64 on the same data), plus: the rows of
     that second tile equal, bit for bit, the same rows run as a batch of their own.
  c. Every hidden activation x output None / Sigmoid through forward, backward and second order under the same bar.  The emulator runs the
     host's libm, so this holds the PLUMBING -- which block a derivative is taken at (SiLU / Sine read the pre-activation block behind the
     post-activations), the GENERAL / simple kernel instance chosen -- not the device's expf / tanhf / sinf, which only the GPU tests see.
  d. The slab count of the weight gradients."""
import numpy as np
import pytest

import exact_f32_fused_cases as X
import exact_f32_network_cases as F
import exact_mlp_second_order_cases as S
import second_order_mlp_reference as R
from test_gpu_f32_fused_network import FACTOR, HIDDEN, case as drawn  # (numpy only: the data, the float64 reference and the bars)

fused = pytest.importorskip("emu_mlp_f32_fused")
pytestmark = pytest.mark.skipif(not fused.available(), reason="no host compiler for the emulator")
import emu_mlp_f32 as plain  # noqa: E402  (the layer-by-layer kernels, same signatures)
import emu_mlp_second_order as plain_so  # noqa: E402

ACT = {"None": 0, "ReLU": 1, "LeakyReLU": 2, "Exponential": 3, "Sigmoid": 4, "Squareplus": 5, "Softplus": 6, "Tanh": 7, "SiLU": 8, "Sine": 9}
IDS = [c.name for c in X.CASES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(*pairs):
    report = [F.mismatch(name, got, want) for name, got, want in pairs]
    assert not any(report), "\n".join(r for r in report if r)


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(case):
        if case.name not in cache:
            data = S.generate(case)  # (exact_f32_network_cases.generate plus v)
            cache[case.name] = (data, F.restate(case, data), S.restate(case, data))
        return cache[case.name]
    return get


# ---- a. exact sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_every_sum_of_the_case_is_exact_in_fp32(built, case):
    data, res, _ = built(case)
    fig = F.audit(case, data, res)
    assert F.audit_passes(fig), F.describe(case, fig)


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_every_second_order_sum_of_the_case_is_exact_in_fp32(built, case):
    data, _, res = built(case)
    fig = S.audit(case, data, res)
    assert fig["c2"], "a float64 result of the second-order restatement is not an fp32 number"
    assert S.audit_passes(fig), S.describe(case, fig)


def test_the_sweep_is_the_one_it_claims_to_be():
    shapes = {(c.W, c.IN, c.OUTP, c.H, c.n, c.act) for c in X.CASES}
    assert len(shapes) == len(X.CASES)
    assert {(W, IN, OUTP, 2, 256, "ReLU") for W in (16, 32, 64) for IN in range(16, 129, 16) for OUTP in (16, 32, 48, 64)} <= shapes
    assert {(W, IN, OUTP, H, 768, "ReLU") for W in (16, 32, 64) for H in (1, 3) for IN in (48, 128) for OUTP in (16, 48)} <= shapes
    assert {(64, IN, OUTP, H, 1280, "ReLU") for H in (1, 3) for IN in (48, 128) for OUTP in (16, 48)} <= shapes  # (five tiles: at width 64 only, for the time they take)
    assert any(c.act == "None" for c in X.CASES)
    assert fused.max_blocks() == 2  # 768: workgroup 0 takes tiles 0 and 2, workgroup 1 tile 1
    assert all(fused.supported(fused.meta(c.IN, c.W, c.OUTP, c.H), c.n) for c in X.CASES)


def arguments(case, data):
    m = fused.meta(case.IN, case.W, case.OUTP, case.H, ACT[case.act])
    return m, data.params.astype(np.float32), np.ascontiguousarray(data.x.T, np.float32), data.dy.astype(np.float32)


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_exact_cases_on_the_emulator(built, case):
    data, res, _ = built(case)
    m, params, x_fm, dy = arguments(case, data)
    hidden, out = fused.forward(m, params, x_fm)
    _, out_inference = fused.forward(m, params, x_fm, save=False)
    grads, dinput = fused.backward(m, params, x_fm, hidden, dy)
    accumulated, none = fused.backward(m, params, x_fm, hidden, dy, grads_init=data.grads_init.astype(np.float32), want_dinput=False)  # the weight gradients alone
    assert none is None
    none, dinput_alone = fused.backward(m, params, x_fm, hidden, dy, want_grads=False)
    assert none is None
    check(("prediction", bits(out), F.bits32(res.out)), ("inference", bits(out_inference), F.bits32(res.out)),
          ("saved activations", bits(hidden), F.bits32(np.stack(res.hidden).reshape(-1))),
          ("dL/dinput", bits(dinput.T), F.bits32(res.dinput)), ("dL/dinput alone", bits(dinput_alone.T), F.bits32(res.dinput)),
          ("weight gradients", bits(grads), F.bits32(res.grads)),
          ("weight gradients alone, accumulated", bits(accumulated), F.bits32(res.grads_accumulated)))
    for row_major in (False, True):
        view, buf, mask = fused.inference_trimmed(m, params, x_fm, case.OUT, row_major=row_major)
        check((f"trimmed inference (row-major {row_major})", bits(view), F.bits32(res.out[:, :case.OUT])))
        assert np.isnan(buf[~mask]).all(), "the trimmed inference wrote outside the caller's matrix"
    # the layer-by-layer kernels on the same arguments
    hidden_plain, out_plain = plain.forward(m, params, x_fm)
    grads_plain, dinput_plain = plain.backward(m, params, x_fm, hidden_plain, dy)
    check(("prediction, layer by layer", bits(out_plain), bits(out)), ("saved activations, layer by layer", bits(hidden_plain), bits(hidden)),
          ("dL/dinput, layer by layer", bits(dinput_plain), bits(dinput)), ("weight gradients, layer by layer", bits(grads_plain), bits(grads)))


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_exact_second_order_on_the_emulator(built, case):
    data, first, res = built(case)
    m, params, x_fm, dy = arguments(case, data)
    v_fm = np.ascontiguousarray(data.v.T, np.float32)
    hidden = np.stack(first.hidden).reshape(-1).astype(np.float32)  # the stack test_exact_cases_on_the_emulator holds the forward pass to
    assert all(F._is_f32(r) for r in (res.ddy, res.dinput, res.grads)) and not res.dinput.any()
    ddy, dinput, grads = fused.backward_backward(m, params, x_fm, hidden, v_fm, dy)
    only_ddy, _, _ = fused.backward_backward(m, params, x_fm, hidden, v_fm, None, want_dinput=False, want_grads=False)
    _, only_dinput, _ = fused.backward_backward(m, params, x_fm, hidden, v_fm, dy, want_ddy=False, want_grads=False)
    _, _, only_grads = fused.backward_backward(m, params, x_fm, hidden, v_fm, dy, want_ddy=False, want_dinput=False)
    check(("dL/d(dL/doutput)", bits(ddy), F.bits32(res.ddy)), ("weight gradients", bits(grads), F.bits32(res.grads)),
          ("dL/d(dL/doutput) alone", bits(only_ddy), F.bits32(res.ddy)), ("weight gradients alone", bits(only_grads), F.bits32(res.grads)))
    assert not bits(dinput).any() and not bits(only_dinput).any(), "dL/dinput of a network without curvature is +0 everywhere"
    ddy_plain, dinput_plain, grads_plain = plain_so.backward_backward(m, params, x_fm, hidden, v_fm, dy)
    check(("dL/d(dL/doutput), layer by layer", bits(ddy_plain), bits(ddy)), ("weight gradients, layer by layer", bits(grads_plain), bits(grads)))
    assert not bits(dinput_plain).any()


# ---- b. c. under the bar of tests/test_gpu_f32_network.py ---------------------------------------------------------------------------------
def held(report, name, got, ref, bar):
    got = np.asarray(got, np.float64)
    err = float(np.abs(got - ref).max())
    print(f"{name}: emulator max error {err:.3e}, CPU float32 {bar / FACTOR:.3e}, bar {bar:.3e}, max |reference| {np.abs(ref).max():.3e}")
    if not (np.isfinite(got).all() and err <= bar):
        report.append(f"{name}: emulator max error {err:.3e} exceeds the bar {bar:.3e}")


def all_passes(IN, W, H, OUT, n, hidden_act, output_act):
    """forward, backward and second order of the fused kernels on the data of test_gpu_f32_fused_network.case, each result held to its bar
    -> the results, for further comparisons"""
    mats, x, dy, ref, bars = drawn(IN, W, H, OUT, n, hidden_act, output_act, away_from_kinks=True)
    v = np.random.default_rng(99).uniform(-1, 1, size=x.shape).astype(np.float32)
    ref_so, cpu_error = R.errors(mats, x, dy, v, hidden_act, output_act)
    m = fused.meta(IN, W, dy.shape[1], H, ACT[hidden_act], ACT[output_act])
    params, x_fm, v_fm = np.concatenate([a.reshape(-1) for a in mats]), np.ascontiguousarray(x.T), np.ascontiguousarray(v.T)
    hidden, out = fused.forward(m, params, x_fm)
    _, out_inference = fused.forward(m, params, x_fm, save=False)
    assert np.array_equal(bits(out), bits(out_inference))
    grads, dinput = fused.backward(m, params, x_fm, hidden, dy, output=out)
    ddy, dinput_so, grads_so = fused.backward_backward(m, params, x_fm, hidden, v_fm, dy)
    report, tag = [], f"{hidden_act}/{output_act}"
    for name, got, r, bar in zip(("prediction", "dL/dinput", "parameter gradients"), (out, dinput.T, grads), ref, bars):
        held(report, f"{tag} {name}", got, r, bar)
    for name, got, r, e in zip(("dL/d(dL/doutput)", "second-order dL/dinput", "second-order parameter gradients"), (ddy, dinput_so.T, grads_so), ref_so, cpu_error):
        held(report, f"{tag} {name}", got, r, FACTOR * e)
    assert not report, "; ".join(report)
    return dict(m=m, params=params, x_fm=x_fm, v_fm=v_fm, dy=dy, hidden=hidden, out=out, dinput=dinput, grads=grads, ddy=ddy, dinput_so=dinput_so, grads_so=grads_so)


STAGED = dict(IN=128, W=64, H=6, OUT=13, n=768)


def test_the_staged_shape_is_staged_where_it_claims():
    m = fused.meta(STAGED["IN"], STAGED["W"], 16, STAGED["H"])
    limit = fused.lds_floats(m, fused.RESIDENT_LIMIT)
    assert limit == 32768
    assert fused.lds_floats(m, fused.RESIDENT_FORWARD) == 32896 > limit                      # the forward pass and the tangent chain: staged
    # f32b_resident_floats: 64 * (16 + 8) + (5 * 64 [+ 128]) * (64 + 8)
    assert fused.lds_floats(m, fused.RESIDENT_BACKWARD_WITH_DINPUT) == 33792 > limit         # the chain with dL/dinput: staged
    assert fused.lds_floats(m, fused.RESIDENT_BACKWARD_WITHOUT_DINPUT) == 24576 <= limit     # without it: resident


@pytest.mark.parametrize("hidden_act", ["ReLU", "Tanh"])  # (Tanh: the curvature chain, staged as well)
def test_staged_weights_through_the_persistent_loop(hidden_act):
    r = all_passes(hidden_act=hidden_act, output_act="None", **STAGED)
    m, params, x_fm, v_fm, dy, hidden = (r[k] for k in ("m", "params", "x_fm", "v_fm", "dy", "hidden"))
    # the second tile of workgroup 0, after it staged every matrix once already: a sample's prediction, dL/dinput and dL/d(dL/doutput) depend
    # on no other sample, so the same 256 rows as a batch of their own (one tile, staged once) give the same bits
    rows = slice(512, 768)
    x_t, v_t, dy_t = np.ascontiguousarray(x_fm[:, rows]), np.ascontiguousarray(v_fm[:, rows]), np.ascontiguousarray(dy[rows])
    hidden_t, out_t = fused.forward(m, params, x_t)
    _, dinput_t = fused.backward(m, params, x_t, hidden_t, dy_t, want_grads=False)
    ddy_t, dinput_so_t, _ = fused.backward_backward(m, params, x_t, hidden_t, v_t, dy_t, want_grads=False)
    L = STAGED["H"]
    check(("prediction of tile 2", bits(r["out"][rows]), bits(out_t)),
          ("saved activations of tile 2", bits(hidden.reshape(L, STAGED["n"], STAGED["W"])[:, rows]), bits(hidden_t.reshape(L, 256, STAGED["W"]))),
          ("dL/dinput of tile 2", bits(r["dinput"][:, rows]), bits(dinput_t)),
          ("dL/d(dL/doutput) of tile 2", bits(r["ddy"][rows]), bits(ddy_t)),
          ("second-order dL/dinput of tile 2", bits(r["dinput_so"][:, rows]), bits(dinput_so_t)))
    # one result alone: the chain without dL/dinput keeps its matrices resident, with it it stages them -- the same bits either way
    none, dinput_alone = fused.backward(m, params, x_fm, hidden, dy, want_grads=False)
    grads_alone, none_ = fused.backward(m, params, x_fm, hidden, dy, want_dinput=False)
    assert none is None and none_ is None
    check(("dL/dinput without weight gradients", bits(dinput_alone), bits(r["dinput"])), ("weight gradients without dL/dinput (resident chain)", bits(grads_alone), bits(r["grads"])))
    if hidden_act == "Tanh":
        _, dinput_so_alone, _ = fused.backward_backward(m, params, x_fm, hidden, v_fm, dy, want_ddy=False, want_grads=False)
        _, _, grads_so_alone = fused.backward_backward(m, params, x_fm, hidden, v_fm, dy, want_ddy=False, want_dinput=False)
        check(("second-order dL/dinput alone", bits(dinput_so_alone), bits(r["dinput_so"])),
              ("second-order weight gradients alone (resident chain)", bits(grads_so_alone), bits(r["grads_so"])))


@pytest.mark.parametrize("output_act", ["None", "Sigmoid"])
@pytest.mark.parametrize("hidden_act", HIDDEN)
def test_activations(hidden_act, output_act):
    all_passes(32, 32, 2, 4, 256, hidden_act, output_act)


# ---- d. ---------------------------------------------------------------------------------------------------------------------------------
def test_slab_count_is_a_function_of_network_and_batch():
    """1, 2, 4, 4 slabs for one, three, five and seven sample tiles: a power of two, at most the tiles -- with the emulator's two persistent
    workgroups exactly as with the library's 512 (the count is a function of the network and n alone)"""
    for W in (16, 32, 64):
        m = fused.meta(48, W, 16, 2)
        assert [fused.n_partials(m, n) for n in (256, 768, 1280, 1792)] == [1, 2, 4, 4]

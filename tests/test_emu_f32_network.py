"""The fp32 network kernels (csrc/mlp_general_fp32.hip) on the host SIMT emulator, no GPU: the exact cases of
tests/exact_f32_network_cases.py at n = 256 -- prediction, dL/dinput, weight gradients (Overwrite, and Accumulate into a non-zero dyadic
buffer) and inference into a trimmed matrix in both layouts, all np.array_equal on bit patterns against the float64 evaluation cast to
float32 -- and, first, the audit that makes that comparison legitimate, for every case including the n = 768 ones the GPU runs."""
import numpy as np
import pytest

import exact_f32_network_cases as F

emu_f32 = pytest.importorskip("emu_mlp_f32")
pytestmark = pytest.mark.skipif(not emu_f32.available(), reason="no host compiler for the emulator")

ACT = {"None": 0, "ReLU": 1}


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(case):
        if case.name not in cache:
            data = F.generate(case)
            cache[case.name] = (data, F.restate(case, data))
        return cache[case.name]
    return get


@pytest.mark.parametrize("case", F.CASES, ids=[c.name for c in F.CASES])
def test_every_sum_of_the_case_is_exact_in_fp32(built, case):
    data, res = built(case)
    fig = F.audit(case, data, res)
    assert F.audit_passes(fig), F.describe(case, fig)


def test_the_restatement_is_an_fp32_network_in_disguise(built):
    """the float64 restatement against a plain float32 evaluation of the same network: equal, since nothing rounds"""
    case = F.by_name("f32-48x3-n256")
    data, res = built(case)
    a = data.x.astype(np.float32)
    mats = [m.astype(np.float32) for m in F.matrices(case, data.params)]
    for m in mats[:-1]:
        a = np.maximum(a @ m.T, np.float32(0))
    assert np.array_equal((a @ mats[-1].T).astype(np.float64), res.out)


def test_the_audit_notices_an_inexact_sum(built):
    """sensitivity: the same case with finer output gradients fails C1"""
    from dataclasses import replace
    case = replace(F.by_name("f32-48x3-n768"), dy=tuple(k / 4096.0 for k in range(1, 4097)))
    data = F.generate(case)
    assert not F.audit_passes(F.audit(case, data))


def check(*pairs):
    report = [F.mismatch(name, got, want) for name, got, want in pairs]
    assert not any(report), "\n".join(r for r in report if r)


@pytest.mark.parametrize("case", F.CASES_256, ids=[c.name for c in F.CASES_256])
def test_exact_cases_on_the_emulator(built, case):
    data, res = built(case)
    m = emu_f32.meta(case.IN, case.W, case.OUTP, case.H, ACT[case.act])
    params, x_fm, dy = data.params.astype(np.float32), np.ascontiguousarray(data.x.T, np.float32), data.dy.astype(np.float32)
    hidden, out = emu_f32.forward(m, params, x_fm)
    _, out_inference = emu_f32.forward(m, params, x_fm, save=False)
    grads, dinput = emu_f32.backward(m, params, x_fm, hidden, dy)
    accumulated, _ = emu_f32.backward(m, params, x_fm, hidden, dy, grads_init=data.grads_init.astype(np.float32), want_dinput=False)
    check(("prediction", out.view(np.uint32), F.bits32(res.out)), ("inference", out_inference.view(np.uint32), F.bits32(res.out)),
          ("saved activations", hidden.view(np.uint32), F.bits32(np.stack(res.hidden).reshape(-1))),
          ("dL/dinput", np.ascontiguousarray(dinput.T).view(np.uint32), F.bits32(res.dinput)),
          ("weight gradients", grads.view(np.uint32), F.bits32(res.grads)),
          ("weight gradients, accumulated", accumulated.view(np.uint32), F.bits32(res.grads_accumulated)))
    for row_major in (False, True):
        view, buf, mask = emu_f32.inference_trimmed(m, params, x_fm, case.OUT, row_major=row_major)
        check((f"trimmed inference (row-major {row_major})", np.ascontiguousarray(view).view(np.uint32), F.bits32(res.out[:, :case.OUT])))
        assert np.isnan(buf[~mask]).all(), "the trimmed inference wrote outside the caller's matrix"


def test_slab_count_is_a_function_of_network_and_batch():
    m = emu_f32.meta(80, 272, 16, 3)
    assert emu_f32.n_partials(m, 256) == 8 and emu_f32.n_partials(m, 768) == 16  # 25 tiles -> 32 wanted, one stage of 32 samples per slab at least
    assert emu_f32.n_partials(emu_f32.meta(16, 16, 16, 1), 768) == 16

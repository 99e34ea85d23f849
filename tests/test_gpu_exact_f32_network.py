"""Bit-exact parity of the fp32 network (csrc/mlp_general_fp32.hip) on a real MI355X, entry by entry, on inputs where the order of summation
cannot matter (tests/exact_f32_network_cases.py; the audit of every case runs on the CPU in tests/test_emu_f32_network.py).  Through the
module entry points: prediction with its padded columns, inference, dL/dinput, the whole parameter gradient with GradientMode Overwrite and
Accumulate (into a non-zero dyadic buffer), and inference into the caller's trimmed fp32 matrix in both layouts.  Every comparison is
np.array_equal on float32 bit patterns against the float64 evaluation cast to float32."""
import numpy as np
import pytest
import torch

import exact_f32_network_cases as F

pytestmark = pytest.mark.gpu


def _C():
    import tinycudann
    return tinycudann._C


def f_t(values):
    return torch.from_numpy(np.ascontiguousarray(values, np.float64).astype(np.float32)).cuda()


def bits(t):
    assert t.dtype == torch.float32
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def check(*pairs):
    report = [F.mismatch(name, got, want) for name, got, want in pairs]
    assert not any(report), "\n".join(r for r in report if r)


@pytest.fixture(scope="module")
def built():
    """inputs and expected values once per case, shared and left unchanged"""
    cache = {}

    def get(case):
        if case.name not in cache:
            data = F.generate(case)
            cache[case.name] = (data, F.restate(case, data))
        return cache[case.name]
    return get


def module_for(case):
    C = _C()
    m = C.create_network_precision(case.IN, case.OUT, case.network(), C.Precision.Fp32)
    assert m.n_params() == case.n_params and m.n_output_dims() == case.OUTP and m.param_precision() == C.Precision.Fp32
    assert m.hyperparams()["network"]["otype"] == "CutlassMLP"
    return m


@pytest.mark.parametrize("case", F.CASES, ids=[c.name for c in F.CASES])
def test_forward_backward_and_inference(built, case):
    C = _C()
    data, res = built(case)
    m = module_for(case)
    x, p, dy = f_t(data.x).requires_grad_(True), f_t(data.params).requires_grad_(True), f_t(data.dy)
    ctx, y = m.fwd(x, p)
    _, y_inf = m.fwd(x.detach(), p.detach())
    dx, dp = m.bwd(ctx, x, p, y, dy)
    accumulated = f_t(data.grads_init)
    m.bwd_into(ctx, x, p, y, dy, accumulated, C.GradientMode.Accumulate, want_dL_dinput=False)
    overwritten = torch.full_like(accumulated, float("nan"))
    dx2 = m.bwd_into(ctx, x, p, y, dy, overwritten, C.GradientMode.Overwrite)
    untouched = torch.full_like(accumulated, 3.0)
    m.bwd_into(ctx, x, p, y, dy, untouched, C.GradientMode.Ignore)
    torch.cuda.synchronize()
    assert y.dtype == dx.dtype == dp.dtype == torch.float32
    assert y.shape == (case.n, case.OUTP) and dx.shape == (case.n, case.IN) and dp.shape == (case.n_params,)
    check(("prediction", bits(y), F.bits32(res.out)), ("inference", bits(y_inf), F.bits32(res.out)), ("dL/dinput", bits(dx), F.bits32(res.dinput)),
          ("parameter gradients", bits(dp), F.bits32(res.grads)), ("parameter gradients, Overwrite into the caller's buffer", bits(overwritten), F.bits32(res.grads)),
          ("dL/dinput, second backward pass of the context", bits(dx2), F.bits32(res.dinput)),
          ("parameter gradients, Accumulate", bits(accumulated), F.bits32(res.grads_accumulated)))
    assert bool((untouched == 3.0).all())


@pytest.mark.parametrize("layout", ["sample-major", "feature-major"])
@pytest.mark.parametrize("case", F.CASES, ids=[c.name for c in F.CASES])
def test_inference_into_a_trimmed_matrix(built, case, layout):
    """the caller's fp32 matrix of OUT (unpadded) columns, with a stride above its leading dimension: every element of the matrix, nothing else"""
    data, res = built(case)
    m = module_for(case)
    x, p = f_t(data.x), f_t(data.params)
    if layout == "sample-major":
        buf = torch.full((case.n, case.OUT + 3), float("nan"), device="cuda")
        out = buf[:, :case.OUT]
        got = lambda: out  # noqa: E731
    else:
        buf = torch.full((case.OUT, case.n + 5), float("nan"), device="cuda")
        out = buf[:, :case.n]
        got = lambda: out.t()  # noqa: E731
    m.inference_into(x, p, out)
    torch.cuda.synchronize()
    check((f"inference into a trimmed {layout} matrix", bits(got()), F.bits32(res.out[:, :case.OUT])))
    mask = torch.ones_like(buf, dtype=torch.bool)
    (mask[:, :case.OUT] if layout == "sample-major" else mask[:, :case.n])[...] = False
    assert bool(torch.isnan(buf[mask]).all()), "the trimmed inference wrote outside the caller's matrix"

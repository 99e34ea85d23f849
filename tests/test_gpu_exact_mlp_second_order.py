"""Bit-exact parity of the fp32 network's second-order pass (tcnn_module_backward_backward_input on the modules of
tcnn_create_network_precision) on a real MI355X, on inputs where the order of summation cannot matter (tests/exact_mlp_second_order_cases.py;
the audit of every case runs on the CPU in tests/test_emu_mlp_second_order.py): dL/d(dL/doutput) and the whole parameter gradient
np.array_equal on float32 bit patterns to the float64 restatement cast to float32, dL/dinput all zeros (ReLU / None hidden activations
have no curvature)."""
import numpy as np
import pytest
import torch

import exact_mlp_second_order_cases as X

pytestmark = pytest.mark.gpu


def f_t(values):
    return torch.from_numpy(np.ascontiguousarray(values, np.float64).astype(np.float32)).cuda()


def bits(t):
    assert t.dtype == torch.float32
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_second_order_pass(case):
    import tinycudann
    C = tinycudann._C
    data = X.generate(case)
    res = X.restate(case, data)
    m = C.create_network_precision(case.IN, case.OUT, case.network(), C.Precision.Fp32)
    x, p, dy, v = f_t(data.x).requires_grad_(True), f_t(data.params).requires_grad_(True), f_t(data.dy).requires_grad_(True), f_t(data.v)
    ctx, _ = m.fwd(x, p)
    ddy, dp, dx = m.bwd_bwd_input(ctx, x, p, v, dy)
    torch.cuda.synchronize()
    assert ddy.shape == (case.n, case.OUTP) and dp.shape == (case.n_params,) and dx.shape == (case.n, case.IN)
    report = [X.mismatch(name, got, want) for name, got, want in (("dL/d(dL/doutput)", bits(ddy), X.bits32(res.ddy)), ("parameter gradients", bits(dp), X.bits32(res.grads)))]
    assert not any(report), "\n".join(r for r in report if r)
    assert not bits(dx).any(), "dL/dinput of a network without curvature is +0 everywhere"

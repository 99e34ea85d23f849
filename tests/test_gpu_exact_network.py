"""Bit-exact parity of the network kernels on a real MI355X, entry by entry, on inputs where the order of summation cannot matter
(tests/exact_network_cases.py: small dyadic values, every fp32 accumulation exact in any association order; the conditions and the
restatement are checked on the CPU by tests/test_exact_network_reference.py).  Every comparison is np.array_equal on bit patterns: the
prediction with its padded columns, dL/dinput, the whole network parameter gradient and, on trainer paths, the loss gradient.  A mismatch
names the tensor, the number of differing entries and the first few (index, got, want), which points at a tile or a lane."""
import numpy as np
import pytest
import torch

import exact_network_cases as E

pytestmark = pytest.mark.gpu


def tcnn():
    import tinycudann
    return tinycudann


def bits16(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def bits32(t):
    assert t.dtype == torch.float32
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def want32(v):
    return np.ascontiguousarray(v, np.float64).astype(np.float32).view(np.uint32)


def h_t(values):
    return torch.from_numpy(E.to_bits(values).view(np.int16)).view(torch.half).cuda()


def f_t(values):
    return torch.from_numpy(np.ascontiguousarray(values, np.float64).astype(np.float32)).cuda()


def check(*pairs):
    report = [E.mismatch(name, got, want) for name, got, want in pairs]
    assert not any(report), "\n".join(r for r in report if r)


@pytest.fixture(scope="module")
def built():
    """inputs and expected bits once per case, shared and left unchanged"""
    cache = {}

    def get(case):
        if case.name not in cache:
            data = E.generate(case)
            cache[case.name] = (data, E.restate(case, data))
        return cache[case.name]
    return get


class switches:
    """process-wide switches of the library, restored on the way out"""

    def __init__(self, fused_passes=True, fused_identity=True):
        self.values = (fused_passes, fused_identity)

    def __enter__(self):
        C = tcnn()._C
        C.set_fused_network_passes(self.values[0])
        C.set_fused_identity_input(self.values[1])

    def __exit__(self, *exc):
        C = tcnn()._C
        C.set_fused_network_passes(True)
        C.set_fused_identity_input(True)


def module_for(case):
    C = tcnn()._C
    m = C.create_network(case.IN, case.OUT, case.network())
    assert m.n_params() == case.n_params and m.n_output_dims() == case.OUTP
    assert m.hyperparams()["network"]["otype"] == case.otype
    return m


def run_module(case, data, res, half_input=False):
    m = module_for(case)
    x = (h_t(data.x) if half_input else f_t(data.x)).requires_grad_(True)
    p = h_t(data.params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    _, y_inf = m.fwd(x.detach(), p.detach())
    dx, dp = m.bwd(ctx, x, p, y, h_t(data.dy))
    torch.cuda.synchronize()
    assert y.shape == (case.n, case.OUTP) and dx.shape == (case.n, case.IN) and dp.shape == (case.n_params,)
    dinput = ("dL/dinput", bits16(dx), E.to_bits(res.dinput)) if half_input else ("dL/dinput", bits32(dx), want32(res.dinput))
    check(("prediction", bits16(y), E.to_bits(res.out)), ("inference", bits16(y_inf), E.to_bits(res.out)), dinput,
          ("parameter gradients", bits16(dp), E.to_bits(res.grads)))
    assert torch.equal(y, y_inf)  # forward == inference


FUSED = E.MODULE_CASES + E.MODULE_CASES_1024


@pytest.mark.parametrize("fused_passes", [True, False], ids=["single-kernel", "saved-activations"])
@pytest.mark.parametrize("case", FUSED, ids=[c.name for c in FUSED])
def test_module_forward_backward(built, case, fused_passes):
    with switches(fused_passes=fused_passes):
        run_module(case, *built(case))


@pytest.mark.parametrize("case", E.GENERAL_CASES, ids=[c.name for c in E.GENERAL_CASES])
def test_layer_by_layer_network(built, case):
    """mlp_general.hip; at 768 samples the weight gradients come in more than one batch slab, and the slabs are not equally long"""
    run_module(case, *built(case))


@pytest.mark.parametrize("name", ["fused-64x2", "general-256x2-n256"])
def test_half_input_entries(built, name):
    """the *_half_input entries: the same expected bits, and a 16-bit dL/dinput"""
    case = E.by_name(name)
    run_module(case, *built(case), half_input=True)


def trainer_for(case, data):
    T = tcnn()
    cfg = {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6},
           "encoding": {"otype": "Identity"}, "network": case.network()}
    tm = T.create_from_config(case.IN, case.OUT, cfg, seed=1)
    assert tm.n_params == tm.n_mlp_params == case.n_params and tm.padded_output_width == case.OUTP
    tm.set_params_full_precision(f_t(data.params))
    check(("parameters", bits16(tm.params_view), E.to_bits(data.params)))
    return tm


@pytest.mark.parametrize("fused_identity", [True, False], ids=["fp32-input-in-kernel", "encoding-kernel"])
@pytest.mark.parametrize("name", ["fused-64x2", "fused-64x2-in64", "general-256x2-n256", "general-64x2-130-outputs-n256"])
def test_inference_into_fp32(built, name, fused_identity):
    """the fp32 output epilogue (the register-resident inference kernel; the output layer of a layer-by-layer network): the values are
    exact 16-bit numbers widened, so float32 bits"""
    case = E.by_name(name)
    data, res = built(case)
    with switches(fused_identity=fused_identity):
        tm = trainer_for(case, data)
        guard = torch.full((case.n * case.OUT + 64,), float("nan"), device="cuda")
        result = guard[:case.n * case.OUT].view(case.n, case.OUT)
        tm.inference(f_t(data.x), result)
        torch.cuda.synchronize()
    check(("inference into fp32", bits32(result), want32(res.out[:, :case.OUT])))
    assert torch.isnan(guard[case.n * case.OUT:]).all()


@pytest.mark.parametrize("fused_identity", [True, False], ids=["fp32-input-in-kernel", "encoding-kernel"])
@pytest.mark.parametrize("case", E.TRAINER_CASES, ids=[c.name for c in E.TRAINER_CASES])
def test_training_step_with_the_loss_in_the_kernel(built, case, fused_identity):
    """training_step(run_optimizer=False, dL_dinput=...) with the L2 loss evaluated inside the network kernel, and forward() + backward() with
    and without single-kernel network passes: the same bits, all of them the restatement's"""
    data, res = built(case)
    x, t = f_t(data.x), torch.from_numpy(data.targets).cuda()
    want = [("prediction", E.to_bits(res.out)), ("loss gradient", E.to_bits(res.dout)), ("parameter gradients", E.to_bits(res.grads)),
            ("dL/dinput", want32(res.dinput))]

    def compare(label, ctx, tm, dx):
        torch.cuda.synchronize()
        got = [bits16(ctx.output), bits16(ctx.dL_doutput), bits16(tm.param_gradients), bits32(dx)]
        check(*[(f"{label}: {name}", g, w) for (name, w), g in zip(want, got)])

    with switches(fused_identity=fused_identity):
        tm = trainer_for(case, data)
        dx = torch.zeros((case.n, case.IN), device="cuda")
        ctx = tm.training_step(x, t, run_optimizer=False, dL_dinput=dx)
        compare("training_step", ctx, tm, dx)
    for fused_passes in (True, False):
        with switches(fused_passes=fused_passes, fused_identity=fused_identity):
            dx = torch.zeros((case.n, case.IN), device="cuda")
            ctx = tm.forward(x, t, loss_scale=E.LOSS_SCALE, prepare_input_gradients=True)
            tm.backward(ctx, x, dL_dinput=dx)
            compare(f"forward + backward (single-kernel passes {fused_passes})", ctx, tm, dx)

"""The library's optimizers and losses in a torch loop: tinycudann.optim.Optimizer (a torch.optim.Optimizer over the modules' fp32 params,
stepping them with the native fp32 optimizer chains) and tinycudann.Loss (the native loss kernels behind a torch.autograd.Function).

Optimizer, on a 2-D HashGrid (4 levels, T = 2^12) + 64x1 module at batch 256: three steps equal three native.Optimizer fp32 steps fed
the same params.grad, bit for bit; inference_params of an Ema chain is the native weights_ema; a module without grad is skipped;
state_dict round-trips.  Loss, L2 and RelativeL2 on fp32 predictions [300, 3] (ragged: the width is padded to 8, n is no multiple of
anything): values and prediction.grad within 4 ulps of fp32 per element of the same loss written in torch in fp32 (a short chain of
single-rounding operations; a division and a square differ by at most one rounding each between the two formulations); with a 16-bit
prediction the result equals tcnn_loss_evaluate's.  End to end: 200 steps of an fp32 NetworkWithInputEncoding with tinycudann.Loss("L2")
and tinycudann.optim Adam at batch 1024 bring the loss below a tenth of its first value (a deliberately slack bound: it catches a dead
loop)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.5}
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}


def _tcnn():
    import tinycudann as tcnn
    return tcnn


def _module(seed=7, hidden_layers=1, dtype=None):
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": hidden_layers}
    kw = {} if dtype is None else {"dtype": dtype}
    return _tcnn().NetworkWithInputEncoding(2, 3, GRID, net, seed=seed, **kw).cuda()


def _batch(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 2), dtype=np.float32)
    y = np.stack([0.5 + 0.4 * np.sin(3.0 * (c + 1) * x[:, 0]) * np.cos(2.0 * x[:, 1]) for c in range(3)], 1).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def _backward(model, x, y):
    model.zero_grad()
    ((model(x).float() - y) ** 2).mean().backward()


def test_three_steps_equal_the_native_fp32_optimizer():
    tcnn = _tcnn()
    from tinycudann import _C, native
    model = _module()
    cfg = {"otype": "Ema", "decay": 0.9, "nested": ADAM}
    opt = tcnn.optim.Optimizer(model, cfg)
    assert isinstance(opt, torch.optim.Optimizer)
    layers = model.native_tcnn_module.network_layers()
    assert sum(r * c for r, c in layers) < model.params.numel()  # the grid's parameters are non-matrix parameters
    twin = native.Optimizer(cfg, model.params.numel(), layer_sizes=layers, precision=_C.Precision.Fp32)
    w = model.params.data.clone()
    for k in range(3):
        x, y = _batch(256, k)
        _backward(model, x, y)
        twin.step(w, None, model.params.grad.clone(), 1.0)
        opt.step()
        torch.cuda.synchronize()
        assert opt.step_count(model) == twin.step_count == k + 1
        assert torch.equal(model.params.data.view(torch.int32), w.view(torch.int32)), k
    ema = opt.inference_params(model)
    assert ema.dtype == torch.float32 and ema.data_ptr() == opt.native_optimizer(model).state_named("weights_ema").data_ptr()
    assert torch.equal(ema.view(torch.int32), twin.state_named("weights_ema").view(torch.int32))
    assert opt.hyperparams()["nested"]["learning_rate"] == pytest.approx(1e-2)
    opt.update_hyperparams({"nested": {"learning_rate": 0.5}})
    assert opt.hyperparams()["nested"]["learning_rate"] == 0.5
    opt.zero_grad()
    assert model.params.grad is None or not model.params.grad.any()


def test_a_module_without_grad_is_skipped_and_plain_chains_have_no_custom_weights():
    tcnn = _tcnn()
    a, b = _module(1), _module(2)
    opt = tcnn.optim.Optimizer([a, b], ADAM)
    x, y = _batch(256, 0)
    _backward(a, x, y)
    before = b.params.data.clone()
    assert b.params.grad is None
    opt.step()
    torch.cuda.synchronize()
    assert opt.step_count(a) == 1 and opt.step_count(b) == 0
    assert torch.equal(b.params.data, before)
    assert opt.inference_params(a) is a.params
    with pytest.raises(RuntimeError, match="float32"):
        a.params.grad = None
        a.params.data = a.params.data.half()
        tcnn.optim.Optimizer(a, ADAM)


def test_state_dict_round_trips():
    tcnn = _tcnn()
    cfg = {"otype": "Ema", "decay": 0.9, "nested": ADAM}
    model, twin_model = _module(3), _module(3)
    opt, twin = tcnn.optim.Optimizer(model, cfg), tcnn.optim.Optimizer(twin_model, cfg)
    for k in range(2):
        x, y = _batch(256, k)
        _backward(model, x, y)
        opt.step()
    opt.update_hyperparams({"nested": {"learning_rate": 5e-3}})
    twin_model.load_state_dict(model.state_dict())
    twin.load_state_dict(opt.state_dict())
    assert twin.hyperparams() == opt.hyperparams() and twin.step_count(twin_model) == 2
    x, y = _batch(256, 9)
    for m, o in ((model, opt), (twin_model, twin)):
        _backward(m, x, y)
        o.step()
    torch.cuda.synchronize()
    assert torch.equal(model.params.data.view(torch.int32), twin_model.params.data.view(torch.int32))
    assert torch.equal(opt.inference_params(model).view(torch.int32), twin.inference_params(twin_model).view(torch.int32))
    for name in ("first_moments", "second_moments", "param_steps"):
        assert torch.equal(opt.native_optimizer(model).state_named(name), twin.native_optimizer(twin_model).state_named(name)), name


def _torch_loss_values(otype, p, t):
    d = p - t
    if otype == "L2":
        return d * d / 1.0 / p.numel()
    return d * d / (p * p + 0.01).detach() / 1.0 / p.numel()  # (relative_l2.h:70-80: the denominator is not differentiated)


def _within_ulps(a, b, ulps=4):
    return bool((np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))).all())


@pytest.mark.parametrize("otype", ["L2", "RelativeL2"])
def test_loss_against_torch_fp32(otype):
    tcnn = _tcnn()
    rng = np.random.default_rng(11)
    p_np = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    t = torch.from_numpy(rng.uniform(0.0, 1.0, (300, 3)).astype(np.float32)).cuda()
    p = torch.from_numpy(p_np).cuda().requires_grad_(True)
    loss = tcnn.Loss(otype)
    value = loss(p, t)
    assert value.shape == () and value.dtype == torch.float32
    (2.0 * value).backward()  # (the incoming scalar: a power of two scales both sides exactly)
    q = torch.from_numpy(p_np).cuda().requires_grad_(True)
    ref_values = _torch_loss_values(otype, q, t)
    (2.0 * ref_values.sum()).backward()
    values = loss.values(p.detach(), t)
    torch.cuda.synchronize()
    assert values.shape == (300, 3)
    assert _within_ulps(values.cpu().numpy(), ref_values.detach().cpu().numpy())
    assert _within_ulps(p.grad.cpu().numpy(), q.grad.cpu().numpy())
    assert float(value.detach()) == pytest.approx(float(ref_values.detach().sum()), rel=1e-5)
    assert t.grad is None


def test_loss_with_a_16_bit_prediction_is_loss_evaluate():
    tcnn = _tcnn()
    from tinycudann import _C
    dtype = _C.TORCH_DTYPE[_C.preferred_precision()]
    rng = np.random.default_rng(12)
    p = torch.from_numpy(rng.uniform(0.1, 1.0, (300, 3)).astype(np.float32)).cuda().to(dtype)
    t = torch.from_numpy(rng.uniform(0.0, 1.0, (300, 3)).astype(np.float32)).cuda()
    pdf = torch.from_numpy(rng.uniform(0.5, 1.5, (300, 3)).astype(np.float32)).cuda()
    padded = torch.nn.functional.pad(p, (0, 5))
    values, grads = _C.loss_evaluate("RelativeL2", padded, t, 1.0, pdf)
    q = p.clone().requires_grad_(True)
    loss = tcnn.Loss("RelativeL2")
    loss(q, t, pdf).backward()
    torch.cuda.synchronize()
    assert q.grad.dtype == dtype and torch.equal(q.grad.view(torch.int16), grads[:, :3].contiguous().view(torch.int16))
    assert torch.equal(loss.values(p, t, pdf), values[:, :3])
    assert not values[:, 3:].any()


def test_end_to_end_fp32_loop_learns():
    """first run on an MI355X: first loss 3.338e-01, loss after 200 steps 2.373e-05"""
    tcnn = _tcnn()
    model = _module(5, hidden_layers=2, dtype=torch.float32)
    assert model.params.dtype == torch.float32
    opt = tcnn.optim.Optimizer(model, ADAM)
    loss = tcnn.Loss("L2")
    first = last = None
    for k in range(200):
        x, y = _batch(1024, 100 + k)
        opt.zero_grad()
        value = loss(model(x), y)
        value.backward()
        opt.step()
        if k == 0:
            first = float(value.detach())
        last = float(value.detach())
    print(f"end-to-end fp32 loop: first loss {first:.3e}, loss after 200 steps {last:.3e}")
    assert np.isfinite(last) and last < 0.1 * first

"""Networks of widths outside 16/32/64/128 (the layer-by-layer network of tiny-cuda-nn_amd/csrc/mlp_general.hip, the reference's
CutlassMLP) on a real MI355X, through the three surfaces: the module C ABI (tcnn_create_network*), the trainer (tcnn_create_from_config,
training_step, tcnn_network_inference, snapshots) and the tinycudann torch modules.  Bars: those of tests/test_gpu_parity.py for the
same comparisons on the fused widths -- output RAE p99 < 3e-3, weight gradients RAE p99 < 3e-3 and p99.9 < 1.2e-2, dL/dinput within
rtol 2e-2, atol 2e-3 max|ref|."""
import numpy as np
import pytest
import torch

from conftest import ADAM_HASH, HASH_ENCODING_SMALL
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def tcnn():
    import tinycudann
    return tinycudann


def h_np(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def h_t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.half).cuda()


def rae(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (0.5 * (np.abs(a) + np.abs(b)) + np.abs(b).mean() * 1e-2 + 1e-12)


def positions(n, d, seed=1337):
    rng = O.pcg32(seed)
    return O.generate_random_uniform(rng, n * d, 0.0, 1.0).reshape(n, d)


def targets_for(pos, out):
    return np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c + 1) * pos[:, 0]) * np.cos(2 * np.pi * pos[:, 1]) for c in range(out)], 1).astype(np.float32)


def network(width, hidden_layers, **more):
    return dict({"otype": "MLP", "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden_layers}, **more)


def config(width, hidden_layers, loss):
    return {"loss": {"otype": loss}, "optimizer": dict(ADAM_HASH), "encoding": dict(HASH_ENCODING_SMALL), "network": network(width, hidden_layers)}


@pytest.mark.parametrize("IN,W,OUT,H,n", [(16, 48, 3, 1, 1024), (80, 96, 40, 3, 1024), (32, 256, 4, 2, 1024), (32, 256, 4, 2, 768), (64, 528, 4, 2, 1024)])
def test_network_forward_backward(IN, W, OUT, H, n):
    """test_network_forward_backward of tests/test_gpu_parity.py on the layer-by-layer widths: tcnn.Network == identity encoding (padded
    with 1) + the network, against the oracle; 768 samples are 12 stages of the weight-gradient pass over 8 batch slices (uneven)."""
    C = tcnn()._C
    n_in = IN - 3  # exercises the padding of the identity encoding
    m = C.create_network(n_in, OUT, network(W, H))
    om = O.mlp_init(IN, W, OUT, H)
    assert m.n_params() == om.n_params and m.n_output_dims() == om.padded_out == (OUT + 15) // 16 * 16
    assert m.hyperparams()["network"]["otype"] == "CutlassMLP"
    p32 = m.initial_params(1337).cpu().numpy()
    assert np.array_equal(p32, O.mlp_init_params(om, O.pcg32(1337)))  # Xavier draw order, gpu_matrix.h:292-307
    ph = O.f2h(p32)
    rng = np.random.default_rng(3)
    xin = rng.random((n, n_in), dtype=np.float32)
    x = torch.from_numpy(xin).cuda().requires_grad_(True)
    p = h_t(ph).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    _, y_inf = m.fwd(x.detach(), p.detach())
    torch.cuda.synchronize()
    enc = O.identity_forward(xin, IN)
    hid_ref, out_ref = O.mlp_forward(om, ph, enc)
    assert torch.equal(y, y_inf)                                       # inference == forward (test_common.h:160-165)
    e = rae(O.h2f(h_np(y)), O.h2f(out_ref))
    print("output RAE p99", np.percentile(e, 99))
    assert np.percentile(e, 99) < 3e-3
    assert np.max(np.abs(O.h2f(h_np(y)) - O.h2f(out_ref))) < 2e-2 * max(1.0, np.abs(O.h2f(out_ref)).max())

    dy = np.zeros((n, om.padded_out), np.float32)
    dy[:, :OUT] = rng.standard_normal((n, OUT)).astype(np.float32) * 0.05
    dyh = O.f2h(dy)
    dx, dp = m.bwd(ctx, x, p, y, h_t(dyh))
    torch.cuda.synchronize()
    gref, dref = O.mlp_backward(om, ph, enc, hid_ref, out_ref, dyh)
    g = dp.float().cpu().numpy()
    dx_ref = O.h2f(dref)[:, :n_in]
    e = rae(g, gref)
    print("weight gradient RAE p99", np.percentile(e, 99), "p99.9", np.percentile(e, 99.9))
    assert np.percentile(e, 99.9) < 1.2e-2
    assert np.percentile(e, 99) < 3e-3
    assert np.allclose(dx.cpu().numpy(), dx_ref, rtol=2e-2, atol=2e-3 * np.abs(dx_ref).max())


@pytest.mark.parametrize("width,hidden_layers,loss", [(256, 2, "RelativeL2"), (48, 3, "L1")])
def test_training_step_matches_oracle(width, hidden_layers, loss):
    """test_training_step_matches_oracle of tests/test_gpu_parity.py: create_from_config -> training_step -> loss -> inference against the
    oracle's whole-step restatement from identical fp32 master parameters.  These widths have no single-kernel training pass: the step is
    forward (saved activations) -> loss -> backward."""
    T = tcnn()
    cfg = config(width, hidden_layers, loss)
    tm = T.create_from_config(3, 4, cfg, seed=1337)
    og = O.grid_init(3, 16, 2, 15, 16, 1.5)
    adam = O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=1e-6)
    md = O.model_init(3, 4, og, width, hidden_layers, O.LOSS_NAMES.index(loss), adam)
    rng = O.pcg32(O.seed_seq_first(1337))  # Trainer seed path: std::seed_seq{1337} -> pcg32 (trainer.h:53-56)
    init = np.concatenate([O.mlp_init_params(md.mlp, rng), O.generate_random_uniform(rng, md.grid.n_params, -1e-4, 1e-4)])
    assert np.array_equal(tm.params_full_precision.cpu().numpy(), init)
    init[md.mlp.n_params:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))
    st = O.TrainState(md, init)
    n = 1024
    pos = positions(n, 3, seed=21)
    tgt = targets_for(pos, 4)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()

    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-3 * abs(loss_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(pred_ref)), 99) < 3e-3
    _, g_ref = O.loss(md.loss_type, h_np(ctx.output), tgt, 4)
    assert np.array_equal(h_np(ctx.dL_doutput), g_ref)                 # loss gradient: bit-exact on the GPU's own prediction
    g = tm.param_gradients.float().cpu().numpy()
    gref = O.h2f(st.grads)
    nm = md.mlp.n_params
    assert np.percentile(rae(g[:nm], gref[:nm]), 99) < 5e-3
    big = np.abs(gref[nm:]) > 1e-2 * np.abs(gref[nm:]).max()
    assert np.percentile(rae(g[nm:][big], gref[nm:][big]), 99) < 3e-2

    losses, losses_ref = [], []
    for _ in range(3):
        ctx = tm.training_step(x, t)
        losses.append(tm.loss(ctx))
        losses_ref.append(O.training_step(st, pos, tgt))
    assert tm.optimizer_step_count == 3
    assert np.allclose(losses, losses_ref, rtol=2e-2)
    assert losses[-1] < losses[0]
    w = tm.params_full_precision.cpu().numpy()
    assert np.mean(np.abs(w - st.w32) > 1e-2) < 2e-3
    # network->inference: the oracle's to that test's bar, and the bits of a step's prediction on the same batch and parameters
    out = tm.inference(x).cpu().numpy()
    ref = O.inference(md, pos, st.w16)
    assert out.shape == (n, 4)
    assert np.percentile(np.abs(out - ref), 99) < 5e-2
    ctx = tm.training_step(x, t, run_optimizer=False)
    assert np.array_equal(out, ctx.output.float().cpu().numpy()[:, :4])


def test_backward_is_deterministic():
    """two identical backward passes: bit-identical gradient buffers (fixed slices, slabs summed in fixed order, no floating-point atomics)"""
    C = tcnn()._C
    m = C.create_network(32, 4, network(256, 2))
    n = 1024
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.random((n, 32), dtype=np.float32)).cuda().requires_grad_(True)
    p = m.initial_params(7).half().requires_grad_(True)
    dy = torch.zeros((n, 16), dtype=torch.half, device="cuda")
    dy[:, :4] = torch.from_numpy(rng.standard_normal((n, 4)).astype(np.float32) * 0.05).cuda().half()
    results = []
    for _ in range(2):
        ctx, y = m.fwd(x, p)
        dx, dp = m.bwd(ctx, x, p, y, dy)
        torch.cuda.synchronize()
        results.append((h_np(y), dx.cpu().numpy(), h_np(dp)))
    assert np.abs(O.h2f(results[0][2])).max() > 0
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes()


def test_torch_network_module_autograd_and_padding():
    """tinycudann.Network at 256 neurons through autograd: a batch that is no multiple of 256 is padded and sliced, and the gradients are
    those of the module C ABI on the padded batch (parameter gradients divided by the loss scale in fp16, modules.py)."""
    T = tcnn()
    net = T.Network(5, 3, {"n_neurons": 256, "n_hidden_layers": 2}, seed=1337)  # `otype` left alone
    assert net.native_tcnn_module.hyperparams()["network"]["otype"] == "CutlassMLP"
    n, npad = 1000, 1024
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.random((n, 5), dtype=np.float32)).cuda().requires_grad_(True)
    y = net(x)
    assert y.shape == (n, 3) and y.dtype == torch.half and torch.equal(y, net(x))
    tgt = torch.from_numpy(rng.random((n, 3), dtype=np.float32)).cuda()
    ((y.float() - tgt) ** 2).mean().backward()
    g = net.params.grad
    assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all() and g.abs().sum() > 0

    m = T._C.create_network(5, 3, {"n_neurons": 256, "n_hidden_layers": 2})
    xp = torch.zeros((npad, 5), device="cuda")
    xp[:n] = x.detach()
    xp.requires_grad_(True)
    p = net.params.detach().half().requires_grad_(True)
    ctx, yp = m.fwd(xp, p)
    assert torch.equal(yp[:n, :3], y)
    dy = torch.zeros((npad, 16), device="cuda")
    dy[:n, :3] = 2.0 * (y.detach().float() - tgt) / (n * 3) * 128.0
    dx, dp = m.bwd(ctx, xp, p, yp, dy.half())
    ref = dp.float().cpu().numpy() / 128.0
    assert np.abs(ref).max() > 1e-6
    assert np.all(np.abs(g.cpu().numpy() - ref) <= 1.2e-7 + 1e-2 * np.abs(ref))
    dx_ref = dx[:n].cpu().numpy() / 128.0
    assert np.allclose(x.grad.cpu().numpy(), dx_ref, rtol=1e-2, atol=1e-3 * np.abs(dx_ref).max())


def test_snapshot_round_trip_resumes_training_bit_exactly():
    """test_snapshot_round_trip_resumes_training_bit_exactly of tests/test_gpu_parity.py with a 256-wide network"""
    T = tcnn()
    cfg = config(256, 2, "RelativeL2")
    cfg["encoding"]["log2_hashmap_size"] = 14
    n = 1024
    pos = positions(n, 3, seed=11)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()
    a = T.create_from_config(3, 4, cfg, seed=7)
    for _ in range(5):
        a.training_step(x, t, want_context=False)
    blob = a.serialize(serialize_optimizer=True)
    b = T.create_from_config(3, 4, cfg, seed=99)  # different init, then restored
    b.deserialize(blob)
    assert b.optimizer_step_count == 5 and torch.equal(a.params, b.params)
    a.deserialize(blob)  # the fp16 snapshot drops the fp32 master's low bits: align a with it
    for _ in range(3):
        a.training_step(x, t, want_context=False)
        b.training_step(x, t, want_context=False)
    assert torch.equal(a.params_full_precision, b.params_full_precision)
    assert torch.equal(a.inference(x), b.inference(x))

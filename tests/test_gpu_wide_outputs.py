"""Networks with more than 128 (padded) outputs, up to 1024, on a real MI355X: layer-by-layer networks at every hidden width
(tiny-cuda-nn_amd/csrc/mlp_general.hip, mlp_kernels.h mlp_layer_by_layer), through the module C ABI, the trainer (create_from_config,
training_step, inference into fp32, snapshots) and the tinycudann torch modules.  Bars: those of tests/test_gpu_general_mlp.py for the
same comparisons -- output RAE p99 < 3e-3, weight gradients RAE p99 < 3e-3 and p99.9 < 1.2e-2, dL/dinput within rtol 2e-2, atol 2e-3
max|ref|, and that file's test_training_step_matches_oracle bars for a training step.  Every figure is printed before it is asserted."""
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
    return np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c % 7 + 1) * pos[:, 0]) * np.cos(2 * np.pi * (c // 7 + 1) * pos[:, 1]) for c in range(out)], 1).astype(np.float32)


def network(otype, width, hidden_layers):
    return {"otype": otype, "activation": "ReLU", "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden_layers}


def config(width, hidden_layers, loss, otype="FullyFusedMLP"):
    return {"loss": {"otype": loss}, "optimizer": dict(ADAM_HASH), "encoding": dict(HASH_ENCODING_SMALL), "network": network(otype, width, hidden_layers)}


@pytest.mark.parametrize("IN,W,OUT,H,n", [
    (16, 16, 144, 1, 256),     # 9 blocks of outputs over a 16-wide hidden layer: K is a quarter of an LDS stage
    (32, 64, 272, 2, 768),     # 17 blocks; 768 samples are 12 stages of the weight-gradient pass over 8 batch slices (uneven)
    (64, 128, 1000, 2, 512),   # 1000 outputs padded to 1008: 63 blocks, weight-gradient tiles 15 x 64 + 48 rows
    (32, 256, 520, 2, 512),    # a width outside the fused ones under 528 padded outputs
])
def test_network_forward_backward(IN, W, OUT, H, n):
    """test_network_forward_backward of tests/test_gpu_general_mlp.py with more than 128 outputs: tcnn.Network == identity encoding (padded
    with 1) + the network, against the oracle.  The fused widths are asked for as FullyFusedMLP, the reference's spelling for them."""
    C = tcnn()._C
    n_in = IN - 3
    m = C.create_network(n_in, OUT, network("FullyFusedMLP" if W in (16, 32, 64, 128) else "MLP", W, H))
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
    assert y.shape == (n, om.padded_out)
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
    print("dL/dinput max |difference|", np.abs(dx.cpu().numpy() - dx_ref).max(), "max |ref|", np.abs(dx_ref).max())
    assert np.allclose(dx.cpu().numpy(), dx_ref, rtol=2e-2, atol=2e-3 * np.abs(dx_ref).max())


@pytest.mark.parametrize("loss", ["RelativeL2", "L1"])
def test_training_step_matches_oracle(loss):
    """test_training_step_matches_oracle of tests/test_gpu_general_mlp.py: a hash grid in front of 64 neurons x 2 and 144 outputs"""
    T = tcnn()
    width, hidden_layers, out = 64, 2, 144
    tm = T.create_from_config(3, out, config(width, hidden_layers, loss), seed=1337)
    assert tm.padded_output_width == 144
    og = O.grid_init(3, 16, 2, 15, 16, 1.5)
    adam = O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=1e-6)
    md = O.model_init(3, out, og, width, hidden_layers, O.LOSS_NAMES.index(loss), adam)
    rng = O.pcg32(O.seed_seq_first(1337))  # Trainer seed path: std::seed_seq{1337} -> pcg32 (trainer.h:53-56)
    init = np.concatenate([O.mlp_init_params(md.mlp, rng), O.generate_random_uniform(rng, md.grid.n_params, -1e-4, 1e-4)])
    assert np.array_equal(tm.params_full_precision.cpu().numpy(), init)
    init[md.mlp.n_params:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))
    st = O.TrainState(md, init)
    n = 1024
    pos = positions(n, 3, seed=21)
    tgt = targets_for(pos, out)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()

    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    print("loss", tm.loss(ctx), "oracle", loss_ref)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-3 * abs(loss_ref)
    assert ctx.output.shape == (n, 144)
    e = np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(pred_ref)), 99)
    print("prediction RAE p99", e)
    assert e < 3e-3
    _, g_ref = O.loss(md.loss_type, h_np(ctx.output), tgt, out)
    assert np.array_equal(h_np(ctx.dL_doutput), g_ref)                 # loss gradient: bit-exact on the GPU's own prediction
    g = tm.param_gradients.float().cpu().numpy()
    gref = O.h2f(st.grads)
    nm = md.mlp.n_params
    e = np.percentile(rae(g[:nm], gref[:nm]), 99)
    print("network gradient RAE p99", e)
    assert e < 5e-3
    big = np.abs(gref[nm:]) > 1e-2 * np.abs(gref[nm:]).max()
    e = np.percentile(rae(g[nm:][big], gref[nm:][big]), 99)
    print("grid gradient RAE p99", e)
    assert e < 3e-2

    losses, losses_ref = [], []
    for _ in range(3):
        ctx = tm.training_step(x, t)
        losses.append(tm.loss(ctx))
        losses_ref.append(O.training_step(st, pos, tgt))
    print("losses", losses, "oracle", losses_ref)
    assert tm.optimizer_step_count == 3
    assert np.allclose(losses, losses_ref, rtol=2e-2)
    assert losses[-1] < losses[0]
    w = tm.params_full_precision.cpu().numpy()
    print("weights off by more than 1e-2:", np.mean(np.abs(w - st.w32) > 1e-2))
    assert np.mean(np.abs(w - st.w32) > 1e-2) < 2e-3


@pytest.mark.parametrize("out,width", [(130, 16), (131, 32), (1000, 64)])
def test_inference_into_fp32(out, width):
    """network->inference of a layer-by-layer network: the output layer's kernel stores the trimmed fp32 matrix itself.  Rows of 130 floats
    start 8-byte aligned, of 131 floats 4-byte aligned, of 1000 floats 16-byte aligned: a store width each.  The bits are those of a step's
    padded 16-bit prediction on the same batch and parameters, trimmed and widened."""
    T = tcnn()
    tm = T.create_from_config(3, out, config(width, 1, "L2"), seed=5)
    w = tm.params_full_precision.cpu().numpy()
    w[tm.n_mlp_params:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(w))
    n = 512
    pos = positions(n, 3, seed=9)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, out)).cuda()
    guard = torch.full((n * out + 64,), float("nan"), device="cuda")
    result = guard[:n * out].view(n, out)
    tm.inference(x, result)
    assert result.shape == (n, out) and result.dtype == torch.float32
    ctx = tm.training_step(x, t, run_optimizer=False)
    expected = ctx.output.float()[:, :out].contiguous()
    assert ctx.output.shape == (n, (out + 15) // 16 * 16)
    assert expected.abs().max() > 0
    assert torch.equal(result.view(torch.int32), expected.view(torch.int32))
    assert torch.isnan(guard[n * out:]).all()                              # nothing behind the last row
    assert torch.equal(tm.inference(x).view(torch.int32), result.view(torch.int32))  # a fresh matrix: the same bits again


def test_snapshot_round_trip_resumes_training_bit_exactly():
    """test_snapshot_round_trip_resumes_training_bit_exactly of tests/test_gpu_general_mlp.py with 272 outputs behind 64 neurons, built from
    the FullyFusedMLP spelling"""
    T = tcnn()
    out = 272
    cfg = config(64, 2, "RelativeL2")
    cfg["encoding"]["log2_hashmap_size"] = 14
    n = 1024
    pos = positions(n, 3, seed=11)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, out)).cuda()
    a = T.create_from_config(3, out, cfg, seed=7)
    assert a.padded_output_width == 272
    for _ in range(5):
        a.training_step(x, t, want_context=False)
    blob = a.serialize(serialize_optimizer=True)
    b = T.create_from_config(3, out, cfg, seed=99)  # different init, then restored
    b.deserialize(blob)
    assert b.optimizer_step_count == 5 and torch.equal(a.params, b.params)
    a.deserialize(blob)  # the fp16 snapshot drops the fp32 master's low bits: align a with it
    for _ in range(3):
        a.training_step(x, t, want_context=False)
        b.training_step(x, t, want_context=False)
    assert torch.equal(a.params_full_precision, b.params_full_precision)
    assert torch.equal(a.inference(x), b.inference(x))


def test_torch_network_with_256_outputs_over_changing_batch_sizes():
    """The network of the reference's scripts/test_random_input.py -- tcnn.Network(3 -> 256, FullyFusedMLP, 128 neurons x 8 hidden layers) --
    through autograd at a fixed list of row counts, multiples of 256 and not, with the temporary memory freed in between.  One pass over
    the list; then the first row count once more on its original input, which must give the first pass's bits."""
    T = tcnn()
    net = T.Network(3, 256, network("FullyFusedMLP", 128, 8), seed=42)
    assert net.native_tcnn_module.hyperparams()["network"]["otype"] == "CutlassMLP"
    om = O.mlp_init(16, 128, 256, 8)
    assert net.params.numel() == om.n_params
    rng = np.random.default_rng(8)
    xin = y = first = None
    for rows in (200, 1000, 257, 1024, 999, 256, 513, 768):
        net.params.grad = None
        xin = rng.random((rows, 3), dtype=np.float32)
        x = torch.from_numpy(xin).cuda()
        y = net(x)
        assert y.shape == (rows, 256) and y.dtype == torch.half
        y.mean().backward()
        g = net.params.grad
        assert g is not None and g.shape == net.params.shape and torch.isfinite(g).all() and g.abs().sum() > 0
        if first is None:
            first = (xin, h_np(y).copy(), g.detach().cpu().numpy().copy())
        T.free_temporary_memory()
    # the first row count once more, on its original input, after the seven other row counts: the kernels are deterministic
    # (test_backward_is_deterministic), so the same bits (histories on recycled blocks: tests/test_gpu_call_history.py)
    net.params.grad = None
    again = net(torch.from_numpy(first[0]).cuda())
    again.mean().backward()
    g_again = net.params.grad.detach().cpu().numpy()
    raw = lambda a: a.view(np.uint32 if a.dtype == np.float32 else np.uint16)  # noqa: E731  (the array's bits)
    differing = int(np.count_nonzero(h_np(again) != first[1])), int(np.count_nonzero(raw(g_again) != raw(first[2])))
    assert differing == (0, 0), f"200 rows again after the other row counts: {differing[0]} output entries and {differing[1]} parameter gradient entries differ"
    ph = O.f2h(net.params.detach().float().cpu().numpy())
    n_pad = (xin.shape[0] + 255) // 256 * 256
    xp = np.zeros((n_pad, 3), np.float32)
    xp[:xin.shape[0]] = xin
    _, out_ref = O.mlp_forward(om, ph, O.identity_forward(xp, 16))
    e = rae(O.h2f(h_np(y)), O.h2f(out_ref)[:xin.shape[0], :256])
    print("output RAE p99", np.percentile(e, 99))
    assert np.percentile(e, 99) < 3e-3

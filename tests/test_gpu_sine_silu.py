"""Sine (SIREN) and SiLU hidden activations on a real MI355X, through the three surfaces: the module C ABI, the trainer and the tinycudann
torch modules.  Such a network runs layer by layer at every width (tiny-cuda-nn_amd/csrc/mlp_general.hip) and saves the pre-activations
next to the post-activations.  The reference values are the numpy restatement of tests/sine_silu_reference.py (the CPU oracle knows
neither activation); bars: those of tests/test_gpu_general_mlp.py -- RAE p99 < 3e-3 (output, weight gradients), weight gradients p99.9 <
1.2e-2, dL/dinput within rtol 2e-2, atol 2e-3 max|ref|; tests/test_library_sine_silu.py asserts that the restatement's two accumulation
orders agree within half of each on these cases."""
import numpy as np
import pytest
import torch

import sine_silu_reference as S
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


def network(act, width, hidden_layers, **more):
    return dict({"otype": "MLP", "activation": S.NAMES[act], "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden_layers}, **more)


def gpu_stacks(c):
    """The GPU's own saved stacks (post, pre), [H][n][W] each, which no interface hands out -- read through networks that do.  A network whose
    output matrix has a single 1.0 per row copies neurons to its outputs exactly, 128 at a time.  post[l]: the first l + 1 hidden layers of
    the network under test in front of such a matrix.  pre[l]: ONE hidden layer with weights W_l and activation None on the input post[l - 1]
    (the network input for l = 0): its post-activation is the rounded accumulator, which is the pre-activation."""
    C = tcnn()._C
    IN, W, OUT, H = c.shape
    mats = S.split(c.ph, IN, W, OUT, H)
    one = O.f2h(np.float32(1.0)).item()

    def neurons(cfg, x_h, hidden_mats):
        out = np.zeros((c.n, W), np.uint16)
        for first in range(0, W, 128):
            rows = min(128, W - first)
            select = np.zeros((rows, W), np.uint16)
            select[np.arange(rows), first + np.arange(rows)] = one
            m = C.create_network(x_h.shape[1], rows, cfg)
            p = h_t(np.concatenate([a.reshape(-1) for a in hidden_mats] + [select.reshape(-1)]))
            assert m.n_params() == p.numel()
            _, y = m.fwd(torch.from_numpy(O.h2f(x_h)).cuda(), p)
            out[:, first:first + rows] = h_np(y)[:, :rows]
        return out

    post, pre = [], []
    for l in range(H):
        post.append(neurons(network(c.act, W, l + 1), c.x, mats[:l + 1]))
        pre.append(neurons(dict(network(c.act, W, 1), activation="None"), c.x if l == 0 else post[l - 1], [mats[l]]))
    return np.stack(post), np.stack(pre)


@pytest.mark.parametrize("act", [S.ACT_SINE, S.ACT_SILU], ids=["Sine", "SiLU"])
@pytest.mark.parametrize("shape", S.CASES, ids=[str(c) for c in S.CASES])
def test_network_forward_backward(act, shape):
    """create_network with IN inputs (an identity encoding that pads nothing) on the shared cases: initial parameters bit for bit, forward,
    inference == forward, backward, and two identical backward passes giving identical bytes.  Compared layer by layer on this side's own
    stacks (sine_silu_reference.py says why; gpu_stacks() gets them)."""
    IN, W, OUT, H, n = shape
    c = S.case(act, shape)
    m = tcnn()._C.create_network(IN, OUT, network(act, W, H))
    assert m.n_params() == c.p32.size and m.hyperparams()["network"]["otype"] == "CutlassMLP"
    p32 = m.initial_params(1337).cpu().numpy()
    assert np.array_equal(p32, c.p32)  # Sine: the SIREN draw (gpu_matrix.h:343-377); SiLU: the oracle's Xavier draw
    x = torch.from_numpy(O.h2f(c.x)).cuda().requires_grad_(True)  # fp16 values: the identity encoding's cast is exact
    p = h_t(c.ph).requires_grad_(True)
    _, y_inf = m.fwd(x.detach(), p.detach())
    results = []
    for _ in range(2):
        ctx, y = m.fwd(x, p)
        dx, dp = m.bwd(ctx, x, p, y, h_t(c.dy))
        torch.cuda.synchronize()
        results.append((h_np(y), dx.cpu().numpy(), h_np(dp)))
    assert np.array_equal(h_np(y_inf), results[0][0])  # inference == forward, bit for bit
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes()
    _, dx, g = results[0]
    assert np.abs(O.h2f(g)).max() > 0
    post, pre = gpu_stacks(c)
    S.check(dict(post=post, pre=pre, out=results[0][0], g=g, dx=O.f2h(dx)), c.reference_on(pre, post), S.BARS_FP16, label=f"gpu {S.NAMES[act]} {shape}")
    # and the chain as a whole stays near the restatement's own: wrong stacks from gpu_stacks() would show here, not above
    assert np.percentile(S.rae(O.h2f(results[0][0]), O.h2f(c.out_ref)), 90) < 3e-3


def test_trainer_with_a_sine_network():
    """create_from_config (small hash grid + 64 x 2 Sine network, L2): the step's network gradients are the module path's bits (the same
    kernels), the loss gradient is the oracle's on the GPU's own prediction, training reduces the loss, inference == the step's prediction."""
    T = tcnn()
    net = network(S.ACT_SINE, 64, 2)
    cfg = {"loss": {"otype": "L2"}, "optimizer": dict(ADAM_HASH), "encoding": dict(HASH_ENCODING_SMALL), "network": net}
    tm = T.create_from_config(3, 4, cfg, seed=1337)
    og = O.grid_init(3, 16, 2, 15, 16, 1.5)
    n_mlp = S.n_params(32, 64, 4, 2)
    rng = O.pcg32(O.seed_seq_first(1337))  # Trainer seed path: std::seed_seq{1337} -> pcg32 (trainer.h:53-56)
    init = np.concatenate([S.siren_init_params(32, 64, 4, 2, rng), O.generate_random_uniform(rng, og.n_params, -1e-4, 1e-4)])
    assert np.array_equal(tm.params_full_precision.cpu().numpy(), init)  # the grid's draw follows the SIREN draw in the stream, unchanged
    init[n_mlp:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))

    n = 1024
    pos = O.generate_random_uniform(O.pcg32(21), n * 3, 0.0, 1.0).reshape(n, 3)
    tgt = np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (k + 1) * pos[:, 0]) * np.cos(2 * np.pi * pos[:, 1]) for k in range(4)], 1).astype(np.float32)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()

    ctx = tm.training_step(x, t, run_optimizer=False)
    _, g_ref = O.loss(O.LOSS_L2, h_np(ctx.output), tgt, 4)
    assert np.array_equal(h_np(ctx.dL_doutput), g_ref)
    g_step = h_np(tm.param_gradients)[:n_mlp]
    m = T._C.create_network_with_input_encoding(3, 4, dict(HASH_ENCODING_SMALL), net)
    p = tm.params_view.detach().clone().requires_grad_(True)
    xm = x.clone().requires_grad_(True)
    mctx, y = m.fwd(xm, p)
    assert np.array_equal(h_np(y), h_np(ctx.output))
    _, dp = m.bwd(mctx, xm, p, y, ctx.dL_doutput)
    torch.cuda.synchronize()
    assert np.abs(O.h2f(g_step)).max() > 0
    assert np.array_equal(h_np(dp)[:n_mlp], g_step)

    out = tm.inference(x).cpu().numpy()
    assert np.array_equal(out, ctx.output.float().cpu().numpy()[:, :4])

    losses = []
    for _ in range(20):
        losses.append(tm.loss(tm.training_step(x, t)))
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_torch_network_module_autograd_and_padding():
    """tinycudann.Network with a Sine activation through autograd: a batch of 1000 is padded to 1024, and the gradients are those of the
    module C ABI on the padded batch (the comparison and its bar: tests/test_gpu_general_mlp.py)."""
    T = tcnn()
    cfg = {"activation": "Sine", "n_neurons": 64, "n_hidden_layers": 2}
    net = T.Network(5, 3, cfg, seed=1337)
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

    m = T._C.create_network(5, 3, cfg)
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

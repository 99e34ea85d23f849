"""The numpy restatement of the network's second-order pass (tests/second_order_mlp_reference.py) in float64 against
torch.autograd.grad(create_graph=True) through a float64 torch MLP on the CPU: 32 -> 64 x 2 -> 4 at n = 64, all ten hidden activations with
a None output and the seven output activations with Tanh hidden.  Both sides evaluate the same expression in float64, so the bar is a
relative 1e-10 of the largest entry."""
import numpy as np
import pytest
import torch

import second_order_mlp_reference as R

HIDDEN = ["None", "ReLU", "LeakyReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh", "SiLU", "Sine"]
OUTPUT = ["ReLU", "LeakyReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh"]
IN, W, H, OUT, OUTP, N = 32, 64, 2, 4, 16, 64


def torch_act(name, x):
    if name == "None":
        return x
    if name == "ReLU":
        return torch.relu(x)
    if name == "LeakyReLU":
        return torch.where(x > 0, x, x * 0.01)
    if name == "Exponential":
        return torch.exp(x)
    if name == "Sigmoid":
        return torch.sigmoid(x)
    if name == "Squareplus":
        y = x * R.K
        return 0.5 * (y + torch.sqrt(y * y + 4.0)) / R.K
    if name == "Softplus":
        return torch.log(torch.exp(x * R.K) + 1.0) / R.K
    if name == "Tanh":
        return torch.tanh(x)
    if name == "SiLU":
        return x * torch.sigmoid(x)
    if name == "Sine":
        return torch.sin(x)
    raise KeyError(name)


def torch_mlp(mats, x, hidden_act, output_act):
    a = x
    for m in mats[:-1]:
        a = torch_act(hidden_act, a @ m.T)
    return torch_act(output_act, a @ mats[-1].T)


def inputs(seed):
    rng = np.random.default_rng(seed)
    mats = []
    for rows, cols in [(W, IN)] + [(W, W)] * (H - 1) + [(OUTP, W)]:
        s = np.sqrt(6.0 / (rows + cols))
        mats.append(rng.uniform(-s, s, size=(rows, cols)))
    mats[-1][OUT:] = 0
    x = rng.uniform(-1, 1, size=(N, IN))
    dy = np.zeros((N, OUTP))
    dy[:, :OUT] = rng.uniform(-1, 1, size=(N, OUT))
    v = rng.uniform(-1, 1, size=(N, IN))
    return mats, x, dy, v


def compare(hidden_act, output_act):
    mats, x, dy, v = inputs(31)
    ddy, dinput, grads, _ = R.second_order(np.float64, mats, x, dy, v, hidden_act, output_act)
    tm = [torch.from_numpy(m).requires_grad_(True) for m in mats]
    tx, tdy, tv = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(dy).requires_grad_(True), torch.from_numpy(v)
    y = torch_mlp(tm, tx, hidden_act, output_act)
    (dx,) = torch.autograd.grad(y, tx, tdy, create_graph=True)
    want = torch.autograd.grad((dx * tv).sum(), [tdy, tx] + tm, allow_unused=True)
    want = [torch.zeros_like(t) if w is None else w for w, t in zip(want, [tdy, tx] + tm)]  # (nothing curves: S does not depend on x)
    pairs = [("dS/d(dy)", ddy, want[0].numpy()), ("dS/dx", dinput, want[1].numpy()), ("dS/dW", grads, np.concatenate([w.numpy().reshape(-1) for w in want[2:]]))]
    for name, got, ref in pairs:
        scale = max(float(np.abs(ref).max()), float(np.abs(got).max()))
        assert float(np.abs(got - ref).max()) <= 1e-10 * scale, (name, float(np.abs(got - ref).max()), scale)
    return pairs


@pytest.mark.parametrize("hidden_act", HIDDEN)
def test_hidden_activations(hidden_act):
    pairs = compare(hidden_act, "None")
    assert np.abs(pairs[0][2]).max() > 0 and np.abs(pairs[2][2]).max() > 0
    # piecewise linear activations: the pass has no curvature term, smooth ones do
    assert (np.abs(pairs[1][2]).max() == 0) == (hidden_act in ("None", "ReLU", "LeakyReLU"))


@pytest.mark.parametrize("output_act", OUTPUT)
def test_output_activations(output_act):
    pairs = compare("Tanh", output_act)
    assert all(np.abs(ref).max() > 0 for _, _, ref in pairs)

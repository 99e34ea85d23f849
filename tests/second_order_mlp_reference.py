"""The second-order pass of the fp32 network (csrc/mlp_general_fp32.hip mlp_f32_backward_backward) restated in numpy, in the dtype it is
given.  Helper, not a test.

The network: matrices W_0 [W][IN], W_1 .. W_HM [W][W], W_out [OUTP][W]; a_{-1} = x, p_j = W_j a_{j-1}, a_j = act(p_j), q = W_out a_HM,
y = out_act(q).  First order, from dy = dL/dy: g = dy * out_act'(q), e_j = W_{j+1}^T d_{j+1} (e_HM = W_out^T g), d_j = e_j * act'(p_j),
dx = W_0^T d_0.  Given v = dL/d(dx), the scalar is S = <v, dx>, and its gradients are, in four steps:
  1. tangent      t_0 = W_0 v, u_j = t_j * act'(p_j), t_{j+1} = W_{j+1} u_j, t_out = W_out u_HM;          dS/d(dy) = t_out * out_act'(q)
  2. first order  e_j and d_j once more (the forward context keeps neither)
  3. curvature    c_out = dy * out_act''(q) * t_out, c_j = e_j * t_j * act''(p_j) + (W_{j+1}^T c_{j+1}) * act'(p_j);   dS/dx = W_0^T c_0
  4. weights      dS/dW_j = sum over samples (d_j (x) u_{j-1} + c_j (x) a_{j-1}) with u_{-1} = v; dS/dW_out = sum (g (x) u_HM + c_out (x) a_HM)
The derivatives are written through the PRE-activation here (the kernels take them through the saved post-activation where one determines
them), so that the two are independent statements of the same function."""
import numpy as np

K = 10.0


def act3(name, x):
    """activation, first and second derivative at the pre-activation x, in x's dtype"""
    t = x.dtype.type
    one, two, k = t(1), t(2), t(K)
    zero = np.zeros_like(x)
    if name == "None":
        return x, np.ones_like(x), zero
    if name == "ReLU":
        return np.maximum(x, t(0)), (x > 0).astype(x.dtype), zero
    if name == "LeakyReLU":
        return np.where(x > 0, x, x * t(0.01)), np.where(x > 0, one, t(0.01)), zero
    if name == "Exponential":
        e = np.exp(x)
        return e, e, e
    if name == "Sigmoid":
        s = one / (one + np.exp(-x))
        return s, s * (one - s), s * (one - s) * (one - two * s)
    if name == "Squareplus":
        y = x * k
        r = np.sqrt(y * y + t(4))
        return t(0.5) * (y + r) / k, t(0.5) * (one + y / r), two * k / (r * r * r)
    if name == "Softplus":
        s = one / (one + np.exp(-x * k))
        return np.log(np.exp(x * k) + one) / k, s, k * s * (one - s)
    if name == "Tanh":
        y = np.tanh(x)
        return y, one - y * y, -two * y * (one - y * y)
    if name == "SiLU":
        s = one / (one + np.exp(-x))
        return x * s, s + x * (s * (one - s)), s * (one - s) * (two + x * (one - two * s))
    if name == "Sine":
        return np.sin(x), np.cos(x), -np.sin(x)
    raise KeyError(name)


def second_order(dtype, mats, x, dy, v, hidden_act, output_act):
    """mats: the weight matrices, input matrix first; x, v [n][IN]; dy [n][OUTP] -> (dS/d(dy) [n][OUTP], dS/dx [n][IN], dS/dW flat in parameter
    order, and a dict of the intermediate matrices by the names above)"""
    mats = [np.asarray(m).astype(dtype) for m in mats]
    x, dy, v = (np.asarray(a).astype(dtype) for a in (x, dy, v))
    H = len(mats) - 1
    acts, f1, f2 = [x], [], []
    for m in mats[:-1]:
        a, d1, d2 = act3(hidden_act, acts[-1] @ m.T)
        acts.append(a)
        f1.append(d1)
        f2.append(d2)
    y, o1, o2 = act3(output_act, acts[-1] @ mats[-1].T)
    # first order
    g = dy * o1
    e, d = [None] * H, [None] * H
    back = g @ mats[-1]
    for j in range(H - 1, -1, -1):
        e[j] = back
        d[j] = back * f1[j]
        back = d[j] @ mats[j]
    dx = back
    # 1. tangent
    t, u = [], []
    cur = v
    for j in range(H):
        t.append(cur @ mats[j].T)
        u.append(t[j] * f1[j])
        cur = u[j]
    t_out = cur @ mats[-1].T
    ddy = t_out * o1
    # 3. curvature
    c_out = dy * o2 * t_out
    c = [None] * H
    back = c_out @ mats[-1]
    for j in range(H - 1, -1, -1):
        c[j] = e[j] * t[j] * f2[j] + back * f1[j]
        back = c[j] @ mats[j]
    dinput = back
    # 4. weights
    grads = [None] * (H + 1)
    grads[H] = g.T @ u[H - 1] + c_out.T @ acts[H]
    for j in range(H):
        grads[j] = d[j].T @ (u[j - 1] if j > 0 else v) + c[j].T @ acts[j]
    parts = dict(acts=acts, y=y, g=g, e=e, d=d, dx=dx, t=t, u=u, t_out=t_out, c_out=c_out, c=c)
    return ddy, dinput, np.concatenate([w.reshape(-1) for w in grads]), parts


def errors(mats, x, dy, v, hidden_act, output_act):
    """the float64 restatement and, per result, max |float32 restatement - float64| on the same inputs: the CPU float32 error a GPU bar is
    a multiple of (tests/test_gpu_f32_network.py's rule)"""
    ref = second_order(np.float64, mats, x, dy, v, hidden_act, output_act)[:3]
    f32 = second_order(np.float32, mats, x, dy, v, hidden_act, output_act)[:3]
    return ref, [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(f32, ref)]

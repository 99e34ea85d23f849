"""Reference for the fp32 optimizer and loss tests (host emulator and GPU): the reference's optimizer kernels with T = float, restated in
numpy fp32 the way tests/optimizer_reference.py restates them for the 16-bit type -- one numpy fp32 operation per operation of the
reference, every intermediate rounded to fp32, nothing fused.  With T = float there is ONE weight vector (`weights[i] = (T)w` is the
identity), gradients and every wrapper buffer are float32.  Plain numpy; nothing here touches the emulator or the GPU library.

  sgd.h:44-69, novograd.h:45-90 + 121-165, lookahead.h:45-58 + 78-96, average.h:45-58 + 81-119, batched.h:46-61 + 78-89,
  exponential_decay.h:59-70, ema.h:45-81 + 102-136, common_device.h:1045-1048 (weight_decay)."""
import sys

import numpy as np

f32 = np.float32


# ---------------------------------------------------------------------------------------------- kernels
def sgd_step(loss_scale, learning_rate, l2_reg, w, g):
    """sgd.h:57-68, every parameter, in place"""
    gradient = (g / f32(loss_scale)).astype(f32)
    gradient = (gradient + (f32(l2_reg) * w).astype(f32)).astype(f32)
    w[:] = (w - (f32(learning_rate) * gradient).astype(f32)).astype(f32)


def novograd_norm64(g, begin, end):
    """the layer's sum of squared fp32 gradients in float64 (each square rounded to fp32 as g * g is)"""
    x = g[begin:end]
    return float(np.sum((x * x).astype(f32).astype(np.float64)))


def novograd_step_layer(h, loss_scale, first_step, second_moment, w, g, m1, begin, end):
    """novograd.h:56-69 for one layer [begin, end) with ITS second moment given; h: dict of hyperparameters; in place"""
    beta1 = f32(0) if first_step else f32(h["beta1"])
    lr = f32(h["learning_rate"])
    s = slice(begin, end)
    gradient = (g[s] / f32(loss_scale)).astype(f32)
    denominator = f32(np.sqrt(f32(second_moment)) + f32(h["epsilon"]))
    t = ((f32(1) - beta1) * gradient).astype(f32)
    t = (t / denominator).astype(f32)
    m1[s] = ((beta1 * m1[s]).astype(f32) + t).astype(f32)
    rel, ab = f32(f32(h["relative_decay"]) * lr), f32(f32(h["absolute_decay"]) * lr)
    decayed = (((f32(1) - rel) * w[s]).astype(f32) - np.copysign(ab, w[s]).astype(f32)).astype(f32)
    w[s] = (decayed - (lr * m1[s]).astype(f32)).astype(f32)


def lookahead_pull(alpha, w, slow):
    """lookahead.h:55-57, in place"""
    new = ((slow * f32(f32(1) - f32(alpha))).astype(f32) + (w * f32(alpha)).astype(f32)).astype(f32)
    w[:] = new
    slow[:] = new


def average_step(n_samples, w, sample, average):
    """average.h:55-57, in place"""
    d = (w - sample).astype(f32)
    d = (d / f32(n_samples)).astype(f32)
    average[:] = (average + d).astype(f32)
    sample[:] = w


def batched_accumulate(first, multiplier, g, pool):
    """batched.h:56-60, in place"""
    if first:
        pool[:] = 0
    pool[:] = (pool + (g / f32(multiplier)).astype(f32)).astype(f32)


def batched_cast(pool, g):
    """batched.h:84 cast<float>, in place"""
    g[:] = pool


def ema_step(decay, current_step, w, ema):
    """ema.h:45-60 + 107-108, in place"""
    old = f32(1 - f32(np.power(np.float64(f32(decay)), np.float64(current_step - 1))))
    new = f32(f32(1) / f32(1 - f32(np.power(np.float64(f32(decay)), np.float64(current_step)))))
    a = ((ema * f32(decay)).astype(f32) * old).astype(f32)
    b = (w * f32(f32(1) - f32(decay))).astype(f32)
    ema[:] = ((a + b).astype(f32) * new).astype(f32)


# ---------------------------------------------------------------------------------------------- the classes' host logic
# K: where the kernels come from -- this module (the default), or an object with the same functions that runs the library's kernels
# (tests/emu/emu_optimizers_f32.py Kernels), so that one statement of the host logic serves both sides.
_NUMPY_KERNELS = sys.modules[__name__]


class SGD:
    def __init__(self, learning_rate=1e-3, l2_reg=1e-8, K=None):
        self.learning_rate, self.l2_reg, self.current_step, self.K = f32(learning_rate), f32(l2_reg), 0, K or _NUMPY_KERNELS

    def step(self, loss_scale, w, g):
        self.current_step += 1
        self.K.sgd_step(loss_scale, self.learning_rate, self.l2_reg, w, g)

    def step_count(self):
        return self.current_step

    def custom_weights(self):
        return None


class Lookahead:
    def __init__(self, nested, n, alpha=0.5, n_steps=16, K=None, alloc=np.zeros):
        self.nested, self.alpha, self.n_steps, self.K = nested, alpha, n_steps, K or _NUMPY_KERNELS
        self.slow = alloc(n, f32)

    def step(self, loss_scale, w, g):
        current = self.nested.step_count()
        if current == 0:
            self.slow[:] = w
        if current % self.n_steps == 0:
            self.K.lookahead_pull(self.alpha, w, self.slow)
        self.nested.step(loss_scale, w, g)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.slow


class Average:
    def __init__(self, nested, n, n_samples=128, K=None, alloc=np.zeros):
        self.nested, self.n_samples, self.K = nested, n_samples, K or _NUMPY_KERNELS
        self.samples, self.average = alloc(n_samples * n, f32).reshape(n_samples, n), alloc(n, f32)  # the ring is ONE block: slots n apart

    def step(self, loss_scale, w, g):
        self.nested.step(loss_scale, w, g)
        self.K.average_step(self.n_samples, w, self.samples[self.nested.step_count() % self.n_samples], self.average)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.average


class Batched:
    def __init__(self, nested, n, batch_size_multiplier=16, K=None, alloc=np.zeros):
        self.nested, self.multiplier, self.current_step, self.K = nested, batch_size_multiplier, 0, K or _NUMPY_KERNELS
        self.pool, self.pool_cast = alloc(n, f32), alloc(n, f32)

    def step(self, loss_scale, w, g):
        self.K.batched_accumulate(self.current_step % self.multiplier == 0, self.multiplier, g, self.pool)
        self.current_step += 1
        if self.current_step % self.multiplier == 0:
            self.K.batched_cast(self.pool, self.pool_cast)
            self.nested.step(loss_scale, w, self.pool_cast)

    def step_count(self):
        return self.current_step

    def custom_weights(self):
        return self.nested.custom_weights()


class ExponentialDecay:
    def __init__(self, nested, decay_base=0.1, decay_interval=10000, decay_start=10000, decay_end=10000000):
        self.nested, self.base, self.interval, self.start, self.end = nested, f32(decay_base), decay_interval, decay_start, decay_end
        self.factor, self.base_lr = f32(1), f32(nested.learning_rate)

    def step(self, loss_scale, w, g):
        s = self.nested.step_count()
        if s == 0:
            self.factor = f32(1)
        if s >= self.start and (s - self.start) % self.interval == 0 and s <= self.end:
            self.factor = f32(self.factor * self.base)
        self.nested.learning_rate = f32(self.base_lr * self.factor)
        self.nested.step(loss_scale, w, g)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.nested.custom_weights()


class Ema:
    def __init__(self, nested, n, decay=0.99, K=None, alloc=np.zeros):
        self.nested, self.decay, self.K, self.ema = nested, decay, K or _NUMPY_KERNELS, alloc(n, f32)

    def step(self, loss_scale, w, g):
        self.nested.step(loss_scale, w, g)
        custom = self.nested.custom_weights()
        self.K.ema_step(self.decay, self.nested.step_count(), w if custom is None else custom, self.ema)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.ema


# ---------------------------------------------------------------------------------------------- shared test data and cases
N = 4099
LAYERS = [(64, 32), (16, 64)]
BEGINS = [0, 2048, 3072]
STEPS = 7
LOSS_SCALE = 128.0
SGD_CFG = {"otype": "SGD", "learning_rate": 1e-2, "l2_reg": 1e-6}
NOVOGRAD = {"learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8, "relative_decay": 1e-3, "absolute_decay": 1e-4}


def gradients(rng, n):
    """magnitudes mixed over 1e-3, 1, 60, as float32"""
    return (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 60.0], n)).astype(f32)


def weights(seed, n=N):
    return np.random.default_rng(seed).standard_normal(n).astype(f32)


def chains(K=None, alloc=np.zeros):
    """name -> (config of the library's optimizer, the restatement's object, {library state name: attribute of the object})"""
    kw = {} if K is None else {"K": K, "alloc": alloc}
    sgd = lambda: SGD(learning_rate=1e-2, l2_reg=1e-6, **({"K": K} if K else {}))  # noqa: E731
    return {
        "SGD": (SGD_CFG, sgd(), {}),
        "Lookahead": ({"otype": "Lookahead", "alpha": 0.5, "n_steps": 3, "nested": SGD_CFG}, Lookahead(sgd(), N, alpha=0.5, n_steps=3, **kw), {"weights_lookahead": "slow"}),
        "Average": ({"otype": "Average", "n_samples": 3, "nested": SGD_CFG}, Average(sgd(), N, n_samples=3, **kw), {"weights_samples": "samples", "weights_average": "average"}),
        "Batched": ({"otype": "Batched", "batch_size_multiplier": 3, "nested": SGD_CFG}, Batched(sgd(), N, batch_size_multiplier=3, **kw),
                    {"averaged_gradients": "pool", "averaged_gradients_half": "pool_cast"}),
        "EmaDecay": ({"otype": "Ema", "decay": 0.9, "nested": {"otype": "ExponentialDecay", "decay_base": 0.5, "decay_start": 2, "decay_interval": 2, "nested": SGD_CFG}},
                     Ema(ExponentialDecay(sgd(), decay_base=0.5, decay_interval=2, decay_start=2), N, decay=0.9, **kw), {"weights_ema": "ema"}),
    }


def state_arrays(obj, attr):
    """the array `attr` of the object or of one nested in it"""
    while not hasattr(obj, attr):
        obj = obj.nested
    return getattr(obj, attr)


# ---------------------------------------------------------------------------------------------- loss cases
LOSSES = ["L2", "RelativeL2", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance", "RelativeL2Luminance"]  # = LossType order


def loss_case(n=256, stride=16, dims=3, seed=21):
    """predictions representable in fp16 AND bf16 (8 significant bits, in [1/8, 2): positive, as CrossEntropy / Variance need), targets,
    data_pdf in [0.5, 1.5) -> (prediction fp32 [n, stride], target [n, dims], data_pdf [n, dims]).  Targets lie in [0.25, 1): the gradients of
    CrossEntropy and Variance scale with target and target^2, and targets near zero would push them below the 16-bit type's normal range"""
    rng = np.random.default_rng(seed)
    mant = rng.integers(128, 256, (n, stride)).astype(f32) / f32(128)
    prediction = (mant * np.exp2(rng.integers(-3, 1, (n, stride)).astype(f32))).astype(f32)
    target = rng.uniform(0.25, 1.0, (n, dims)).astype(f32)
    pdf = rng.uniform(0.5, 1.5, (n, dims)).astype(f32)
    return prediction, target, pdf

"""Reference for the optimizer tests (host emulator and GPU): numpy-fp32 restatements of the reference's optimizer kernels and of the
host logic of its wrapper classes, one numpy fp32 operation per operation of the reference (every intermediate is rounded to fp32, nothing
is fused).  16-bit values are bit patterns (uint16) in the oracle's current half format (O.set_half_format): O.f2h is the round-to-nearest
-even cast, O.h2f the widening.  Plain numpy over the oracle; nothing here touches the emulator or the GPU library.

  sgd.h:44-69, novograd.h:45-90 + 121-165, lookahead.h:45-58 + 78-96, average.h:45-58 + 81-119, batched.h:46-61 + 78-89,
  exponential_decay.h:59-70, ema.h:45-81 + 102-136, common_device.h:1045-1048 (weight_decay)."""
import numpy as np

from oracle import oracle as O

f32 = np.float32


# ---------------------------------------------------------------------------------------------- kernels
def sgd_step(loss_scale, learning_rate, l2_reg, w32, w16, g16):
    """sgd.h:57-68, every parameter, in place"""
    gradient = (O.h2f(g16) / f32(loss_scale)).astype(f32)
    gradient = (gradient + (f32(l2_reg) * w32).astype(f32)).astype(f32)
    w32[:] = (w32 - (f32(learning_rate) * gradient).astype(f32)).astype(f32)
    w16[:] = O.f2h(w32)


def novograd_norm64(g16, begin, end):
    """the layer's sum of squared fp32 gradients in float64 (each square rounded to fp32 as (float)g * (float)g is)"""
    g = O.h2f(g16[begin:end])
    return float(np.sum((g * g).astype(f32).astype(np.float64)))


def novograd_second_moment(beta2, loss_scale, old, gradient_norm):
    """novograd.h:84 (beta2 = 0 on the first step, :143)"""
    t = (f32(1) - f32(beta2)) * f32(gradient_norm)
    t = f32(f32(t) / f32(loss_scale))
    t = f32(t / f32(loss_scale))
    return f32(f32(f32(beta2) * f32(old)) + t)


def novograd_step_layer(h, loss_scale, first_step, second_moment, w32, w16, g16, m1, begin, end):
    """novograd.h:56-69 for one layer [begin, end) with ITS second moment given; h: dict of hyperparameters; in place"""
    beta1 = f32(0) if first_step else f32(h["beta1"])
    lr = f32(h["learning_rate"])
    s = slice(begin, end)
    gradient = (O.h2f(g16[s]) / f32(loss_scale)).astype(f32)
    denominator = f32(np.sqrt(f32(second_moment)) + f32(h["epsilon"]))
    t = ((f32(1) - beta1) * gradient).astype(f32)
    t = (t / denominator).astype(f32)
    m1[s] = ((beta1 * m1[s]).astype(f32) + t).astype(f32)
    rel, ab = f32(f32(h["relative_decay"]) * lr), f32(f32(h["absolute_decay"]) * lr)
    decayed = (((f32(1) - rel) * w32[s]).astype(f32) - np.copysign(ab, w32[s]).astype(f32)).astype(f32)
    w32[s] = (decayed - (lr * m1[s]).astype(f32)).astype(f32)
    w16[s] = O.f2h(w32[s])


def lookahead_pull(alpha, w32, w16, slow16):
    """lookahead.h:55-57, in place"""
    new = ((O.h2f(slow16) * f32(f32(1) - f32(alpha))).astype(f32) + (w32 * f32(alpha)).astype(f32)).astype(f32)
    w32[:] = new
    w16[:] = O.f2h(new)
    slow16[:] = w16


def average_step(n_samples, w16, sample16, average16):
    """average.h:55-57, in place"""
    d = (O.h2f(w16) - O.h2f(sample16)).astype(f32)
    d = (d / f32(n_samples)).astype(f32)
    average16[:] = O.f2h((O.h2f(average16) + d).astype(f32))
    sample16[:] = w16


def batched_accumulate(first, multiplier, g16, pool):
    """batched.h:56-60, in place"""
    if first:
        pool[:] = 0
    pool[:] = (pool + (O.h2f(g16) / f32(multiplier)).astype(f32)).astype(f32)


def batched_cast(pool, g16):
    """batched.h:84 cast<T>, in place"""
    g16[:] = O.f2h(pool)


def ema_step(decay, current_step, w16, ema16):
    """ema.h:45-60 + 107-108 (half precision form), in place"""
    old = f32(1 - f32(np.power(np.float64(f32(decay)), np.float64(current_step - 1))))
    new = f32(f32(1) / f32(1 - f32(np.power(np.float64(f32(decay)), np.float64(current_step)))))
    a = ((O.h2f(ema16) * f32(decay)).astype(f32) * old).astype(f32)
    b = (O.h2f(w16) * f32(f32(1) - f32(decay))).astype(f32)
    ema16[:] = O.f2h(((a + b).astype(f32) * new).astype(f32))


# ---------------------------------------------------------------------------------------------- the classes' host logic
# K: where the kernels come from -- this module (the default), or an object with the same functions that runs the library's kernels
# (tests/emu/emu_optimizers.py Kernels), so that one statement of the host logic serves both sides.
import sys

_NUMPY_KERNELS = sys.modules[__name__]


class SGD:
    def __init__(self, learning_rate=1e-3, l2_reg=1e-8, K=None):
        self.learning_rate, self.l2_reg, self.current_step, self.K = f32(learning_rate), f32(l2_reg), 0, K or _NUMPY_KERNELS

    def step(self, loss_scale, w32, w16, g16):
        self.current_step += 1
        self.K.sgd_step(loss_scale, self.learning_rate, self.l2_reg, w32, w16, g16)

    def step_count(self):
        return self.current_step

    def custom_weights(self):
        return None


class Lookahead:
    def __init__(self, nested, n, alpha=0.5, n_steps=16, K=None, alloc=np.zeros):
        self.nested, self.alpha, self.n_steps, self.K = nested, alpha, n_steps, K or _NUMPY_KERNELS
        self.slow16 = alloc(n, np.uint16)

    def step(self, loss_scale, w32, w16, g16):
        current = self.nested.step_count()
        if current == 0:
            self.slow16[:] = w16
        if current % self.n_steps == 0:
            self.K.lookahead_pull(self.alpha, w32, w16, self.slow16)
        self.nested.step(loss_scale, w32, w16, g16)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.slow16


class Average:
    def __init__(self, nested, n, n_samples=128, K=None, alloc=np.zeros):
        self.nested, self.n_samples, self.K = nested, n_samples, K or _NUMPY_KERNELS
        self.samples16, self.average16 = alloc(n_samples * n, np.uint16).reshape(n_samples, n), alloc(n, np.uint16)  # the ring is ONE block: slots n apart

    def step(self, loss_scale, w32, w16, g16):
        self.nested.step(loss_scale, w32, w16, g16)
        self.K.average_step(self.n_samples, w16, self.samples16[self.nested.step_count() % self.n_samples], self.average16)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.average16


class Batched:
    def __init__(self, nested, n, batch_size_multiplier=16, K=None, alloc=np.zeros):
        self.nested, self.multiplier, self.current_step, self.K = nested, batch_size_multiplier, 0, K or _NUMPY_KERNELS
        self.pool, self.pool16 = alloc(n, f32), alloc(n, np.uint16)

    def step(self, loss_scale, w32, w16, g16):
        self.K.batched_accumulate(self.current_step % self.multiplier == 0, self.multiplier, g16, self.pool)
        self.current_step += 1
        if self.current_step % self.multiplier == 0:
            self.K.batched_cast(self.pool, self.pool16)
            self.nested.step(loss_scale, w32, w16, self.pool16)

    def step_count(self):
        return self.current_step

    def custom_weights(self):
        return self.nested.custom_weights()


class ExponentialDecay:
    def __init__(self, nested, decay_base=0.1, decay_interval=10000, decay_start=10000, decay_end=10000000):
        self.nested, self.base, self.interval, self.start, self.end = nested, f32(decay_base), decay_interval, decay_start, decay_end
        self.factor, self.base_lr = f32(1), f32(nested.learning_rate)

    def step(self, loss_scale, w32, w16, g16):
        s = self.nested.step_count()
        if s == 0:
            self.factor = f32(1)
        if s >= self.start and (s - self.start) % self.interval == 0 and s <= self.end:
            self.factor = f32(self.factor * self.base)
        self.nested.learning_rate = f32(self.base_lr * self.factor)
        self.nested.step(loss_scale, w32, w16, g16)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.nested.custom_weights()


class Ema:
    def __init__(self, nested, n, decay=0.99):
        self.nested, self.decay, self.ema16 = nested, decay, np.zeros(n, np.uint16)

    def step(self, loss_scale, w32, w16, g16):
        self.nested.step(loss_scale, w32, w16, g16)
        custom = self.nested.custom_weights()
        ema_step(self.decay, self.nested.step_count(), w16 if custom is None else custom, self.ema16)

    def step_count(self):
        return self.nested.step_count()

    def custom_weights(self):
        return self.ema16


# ---------------------------------------------------------------------------------------------- shared test data
def gradients(rng, n):
    """magnitudes mixed over 1e-3, 1, 60 (tests/test_gpu_parity_full.py::test_optimizer_object_on_its_own_bit_level), as 16-bit patterns"""
    return O.f2h((rng.standard_normal(n) * rng.choice([1e-3, 1.0, 60.0], n)).astype(f32))

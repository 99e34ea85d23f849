"""csrc/optimizer_kernels.hip on the host SIMT emulator (no GPU), for the 16-bit type of either build, against the numpy restatement
(tests/optimizer_reference.py) -- the shapes and bars of tests/test_gpu_optimizers.py:

n_weights = 4099 (16-byte vector body, a ragged scalar tail of 3, a last partial workgroup; the Average ring's slots 1 and 2 start at
2 * 4099 and 4 * 4099 bytes, no multiples of 16: the scalar form of the whole kernel), layers [(64, 32), (16, 64)] = 3072 matrix weights
+ 1027 others, 7 steps: Lookahead(n_steps = 3) pulls at nested counts 0, 3, 6; Average(n_samples = 3) wraps its ring twice;
Batched(batch_size_multiplier = 3) runs the nested step twice and ends on a partly filled pool.

SGD, Lookahead, Average, Batched: every buffer BIT-EQUAL after every step (single-rounding fp32 operations, -ffp-contract=off).
Novograd: the per-layer second moment against a float64 sum of the squared fp32 gradients within (n_layer + 2) 2^-24 relative (a sum of n
non-negative fp32 terms in any order errs by at most n - 1 roundings, plus one per square and one for the moment's update); first moments
and weights bit-equal to the restatement fed with the kernel's own second moment; two runs give the same bits; the 1027 non-matrix weights
stay untouched."""
import numpy as np
import pytest

import emu_optimizers as E
import optimizer_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not E.available(), reason="no host compiler for the emulator")

N = 4099
LAYERS = [(64, 32), (16, 64)]
BEGINS = np.concatenate([[0], np.cumsum([r * c for r, c in LAYERS])]).astype(np.uint32)
STEPS = 7
LOSS_SCALE = 128.0


@pytest.fixture(params=[False, True], ids=["fp16", "bf16"])
def bf16(request):
    O.set_half_format(request.param)
    yield request.param
    O.set_half_format(False)


def _weights(seed):
    w32 = np.random.default_rng(seed).standard_normal(N).astype(np.float32)
    return w32, O.f2h(w32)


def _chains(K=None, alloc=np.zeros):
    kw = {} if K is None else {"K": K, "alloc": alloc}
    sgd = lambda: R.SGD(learning_rate=1e-2, l2_reg=1e-6, **({"K": K} if K else {}))  # noqa: E731
    return {
        "SGD": sgd(),
        "Lookahead": R.Lookahead(sgd(), N, alpha=0.5, n_steps=3, **kw),
        "Average": R.Average(sgd(), N, n_samples=3, **kw),
        "Batched": R.Batched(sgd(), N, batch_size_multiplier=3, **kw),
    }


def _state(opt):
    return {k: v for k, v in vars(opt).items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("which", ["SGD", "Lookahead", "Average", "Batched"])
def test_sgd_and_wrappers_bit_equal(which, bf16):
    ref, got = _chains()[which], _chains(E.Kernels(bf16), E.aligned_zeros)[which]
    w32, w16 = _weights(5)
    gw32, gw16 = E.aligned_copy(w32), E.aligned_copy(w16)
    rng = np.random.default_rng(6)
    for k in range(STEPS):
        g = R.gradients(rng, N)
        ref.step(LOSS_SCALE, w32, w16, g)
        got.step(LOSS_SCALE, gw32, gw16, E.aligned_copy(g))
        assert ref.step_count() == got.step_count()
        assert np.array_equal(gw32.view(np.uint32), w32.view(np.uint32)), k
        assert np.array_equal(gw16, w16), k
        for name, value in _state(ref).items():
            assert np.array_equal(_state(got)[name].view(np.uint8), value.view(np.uint8)), (k, name)
    if which == "Batched":
        assert ref.step_count() == STEPS and ref.nested.step_count() == 2
    if which == "Average":
        assert ref.nested.step_count() // 3 == 2  # the ring wrapped twice


def test_sgd_steps_a_range_only(bf16):
    """[begin, end) as adam_step / ema_step take it: parameters outside keep their bits; two ranges tile one whole step"""
    w32, w16 = _weights(7)
    g = R.gradients(np.random.default_rng(8), N)
    whole32, whole16 = E.aligned_copy(w32), E.aligned_copy(w16)
    E.sgd_step(LOSS_SCALE, 1e-2, 1e-6, whole32, whole16, E.aligned_copy(g), bf16=bf16)
    part32, part16 = E.aligned_copy(w32), E.aligned_copy(w16)
    E.sgd_step(LOSS_SCALE, 1e-2, 1e-6, part32, part16, E.aligned_copy(g), 0, 2056, bf16=bf16)
    assert np.array_equal(part32[2056:], w32[2056:]) and np.array_equal(part16[2056:], w16[2056:])
    E.sgd_step(LOSS_SCALE, 1e-2, 1e-6, part32, part16, E.aligned_copy(g), 2056, N, bf16=bf16)
    assert np.array_equal(part32.view(np.uint32), whole32.view(np.uint32)) and np.array_equal(part16, whole16)
    R.sgd_step(LOSS_SCALE, 1e-2, 1e-6, w32, w16, g)
    assert np.array_equal(whole32.view(np.uint32), w32.view(np.uint32)) and np.array_equal(whole16, w16)


NOVOGRAD = {"learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8, "relative_decay": 1e-3, "absolute_decay": 1e-4}


def test_novograd(bf16):
    w32, w16 = _weights(9)
    w_init32, w_init16 = w32.copy(), w16.copy()
    gw32, gw16, gm1 = E.aligned_copy(w32), E.aligned_copy(w16), E.aligned_zeros(N, np.float32)
    m1 = np.zeros(N, np.float32)
    moments = np.zeros(len(LAYERS), np.float32)
    rng = np.random.default_rng(10)
    for k in range(STEPS):
        g = R.gradients(rng, N)
        ga = E.aligned_copy(g)
        # determinism: the same step from copies of the same state
        again = E.novograd_step(BEGINS, NOVOGRAD, LOSS_SCALE, k == 0, gw32.copy(), gw16.copy(), ga, gm1.copy(), moments, bf16=bf16)
        new = E.novograd_step(BEGINS, NOVOGRAD, LOSS_SCALE, k == 0, gw32, gw16, ga, gm1, moments, bf16=bf16)
        assert np.array_equal(new.view(np.uint32), again.view(np.uint32)), k
        for l in range(len(LAYERS)):
            b, e = int(BEGINS[l]), int(BEGINS[l + 1])
            want = (0.0 if k == 0 else float(np.float32(NOVOGRAD["beta2"])) * float(moments[l])) + \
                (1.0 - (0.0 if k == 0 else float(np.float32(NOVOGRAD["beta2"])))) * R.novograd_norm64(g, b, e) / LOSS_SCALE / LOSS_SCALE
            assert abs(float(new[l]) - want) <= ((e - b) + 2) * 2.0 ** -24 * want, (k, l)
            R.novograd_step_layer(NOVOGRAD, LOSS_SCALE, k == 0, new[l], w32, w16, g, m1, b, e)
        moments = new
        assert np.array_equal(gm1.view(np.uint32), m1.view(np.uint32)), k
        assert np.array_equal(gw32.view(np.uint32), w32.view(np.uint32)), k
        assert np.array_equal(gw16, w16), k
    nm = int(BEGINS[-1])
    assert np.array_equal(gw32[nm:].view(np.uint32), w_init32[nm:].view(np.uint32)) and np.array_equal(gw16[nm:], w_init16[nm:])
    assert not np.array_equal(gw32[:nm], w_init32[:nm])


def test_restatement_known_answers():
    """the restatement itself, on values whose results are exact"""
    O.set_half_format(False)
    w32, w16 = np.array([1.0, -2.0], np.float32), O.f2h(np.array([1.0, -2.0], np.float32))
    R.sgd_step(128.0, 0.5, 0.0, w32, w16, O.f2h(np.array([128.0, -256.0], np.float32)))
    assert np.array_equal(w32, np.array([0.5, -1.0], np.float32)) and np.array_equal(w16, O.f2h(w32))
    slow = O.f2h(np.array([0.0, 0.0], np.float32))
    R.lookahead_pull(0.5, w32, w16, slow)
    assert np.array_equal(w32, np.array([0.25, -0.5], np.float32)) and np.array_equal(slow, w16)
    avg, sample = O.f2h(np.array([1.0, 1.0], np.float32)), O.f2h(np.array([0.25, 0.5], np.float32))
    R.average_step(2, w16, sample, avg)
    assert np.array_equal(O.h2f(avg), np.array([1.0, 0.5], np.float32)) and np.array_equal(sample, w16)
    pool = np.array([7.0, 7.0], np.float32)
    R.batched_accumulate(True, 4, O.f2h(np.array([2.0, -4.0], np.float32)), pool)
    assert np.array_equal(pool, np.array([0.5, -1.0], np.float32))
    assert R.novograd_second_moment(0.0, 2.0, 5.0, 8.0) == np.float32(2.0)

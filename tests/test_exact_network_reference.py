"""The exact-arithmetic network cases (tests/exact_network_cases.py) on the CPU, on the reference alone: every case meets the exactness
conditions C1 - C3, the float64 restatement equals the oracle (which tests/test_oracle_ref.py pins to the reference's own code) bit for
bit, and each case notices three deliberate mistakes.  tests/test_gpu_exact_network.py then holds the HIP kernels to the same bits."""
import numpy as np
import pytest

import exact_network_cases as E
from oracle import oracle as O

ALL = [(c, E.FP16) for c in E.CASES] + [(c, E.BF16) for c in E.BF16_CASES]
IDS = [f"{c.name}-{f.name}" for c, f in ALL]


@pytest.fixture(scope="module")
def built():
    """generate + restate + audit once per case, shared by the tests below (nothing here changes them)"""
    cache = {}

    def get(case, fmt):
        key = (case.name, fmt.name)
        if key not in cache:
            data = E.generate(case, fmt)
            res = E.restate(case, data, fmt)
            cache[key] = (data, res, E.audit(case, data, fmt, res))
        return cache[key]
    return get


class half_format:
    def __init__(self, fmt):
        self.bf16 = fmt is E.BF16

    def __enter__(self):
        O.set_half_format(self.bf16)

    def __exit__(self, *exc):
        O.set_half_format(False)


def assert_conditions(case, fig, for_the_gpu=True):
    print(E.describe(case, fig))
    assert fig["c1_log2"] < 24, ("C1", fig["c1"])
    assert fig["inputs_are_16_bit"]
    assert fig["f32_exact"], "the loss gradient's fp32 arithmetic is not exact"
    assert fig["padding_gradients_zero"]
    if for_the_gpu:
        assert fig["c2"], "C2"
        assert min(fig["c3_rounded"].values()) >= 0.10, ("C3: share of entries that need rounding", fig["c3_rounded"])
        assert min(fig["c3_nonzero"].values()) >= 0.90, ("C3: share of nonzero entries", fig["c3_nonzero"])


@pytest.mark.parametrize("case,fmt", ALL, ids=IDS)
def test_case_meets_the_exactness_conditions(built, case, fmt):
    assert_conditions(case, built(case, fmt)[2])


def oracle_mlp(case):
    return O.mlp_init(case.IN, case.W, case.OUT, case.H, activation=O.ACTIVATION_NAMES.index(case.act), output_activation=O.ACT_NONE)


@pytest.mark.parametrize("case,fmt", ALL, ids=IDS)
def test_restatement_equals_the_oracle(built, case, fmt):
    data, res, _ = built(case, fmt)
    with half_format(fmt):
        om = oracle_mlp(case)
        assert om.n_params == case.n_params and om.padded_out == case.OUTP
        ph, enc = E.to_bits(data.params, fmt), E.to_bits(data.x, fmt)
        hid, out = O.mlp_forward(om, ph, enc)
        for l in range(case.H):
            assert not E.mismatch(f"hidden {l}", hid[l], E.to_bits(res.hidden[l], fmt))
        assert not E.mismatch("output", out, E.to_bits(res.out, fmt))
        if case.trainer:
            _, dout = O.loss(O.LOSS_L2, out, data.targets, case.OUT, loss_scale=E.LOSS_SCALE)
        else:
            dout = E.to_bits(data.dy, fmt)
        assert not E.mismatch("dL/doutput", dout, E.to_bits(res.dout, fmt))
        grad, dinput = O.mlp_backward(om, ph, enc, hid, out, dout)
        assert np.array_equal(grad.astype(np.float32).astype(np.float64), grad)  # (C1: the sums are fp32 numbers)
        assert not E.mismatch("weight gradients", O.f2h(grad), E.to_bits(res.grads, fmt))
        assert not E.mismatch("dL/dinput", dinput, E.to_bits(res.dinput, fmt))


@pytest.mark.parametrize("case", E.TRAINER_CASES, ids=[c.name for c in E.TRAINER_CASES])
def test_trainer_restatement_equals_the_oracle_training_step(case):
    """O.training_step composes encoding, network, loss and backward itself.  Its model has a grid encoding in front: a dense grid with
    nearest-neighbour lookup and parameters from {-1, 0, 1} hands the network exactly such values, so the case's weights and a target
    drawn the same way go through the whole step; prediction and network gradients against the restatement."""
    F = 8
    og = O.grid_init(2, case.IN // F, F, 19, 4, 1.5, O.GRID_DENSE, O.INTERP_NEAREST)
    rng = np.random.default_rng(case.seed)
    table = rng.integers(-1, 2, size=og.n_params).astype(np.float32)
    pos = rng.random((case.n, 2), dtype=np.float32)
    x = E.from_bits(O.grid_forward(og, O.f2h(table), pos, out_stride=case.IN))
    assert set(np.unique(x)) == {-1.0, 0.0, 1.0}
    data = E.generate(case, x=x)
    res = E.restate(case, data)
    # (this batch never reaches a kernel: the order of summation must not matter, C1; a subnormal is the same number to both sides here)
    assert_conditions(case, E.audit(case, data, res=res), for_the_gpu=False)
    md = O.model_init(2, case.OUT, og, case.W, case.H, O.LOSS_L2, O.adam_defaults())
    assert md.mlp.n_params == case.n_params and md.mlp.in_width == case.IN
    st = O.TrainState(md, np.concatenate([data.params.astype(np.float32), table]))
    _, pred = O.training_step(st, pos, data.targets, loss_scale=E.LOSS_SCALE, run_optimizer=False, want_prediction=True)
    assert not E.mismatch("prediction", pred, E.to_bits(res.out))
    assert not E.mismatch("network gradients", st.grads[:case.n_params], E.to_bits(res.grads))


def differs(case, fmt, base, other):
    a, b = base.compared(case), other.compared(case)
    return any(not np.array_equal(E.to_bits(a[k], fmt), E.to_bits(b[k], fmt)) for k in a)


@pytest.mark.parametrize("case,fmt", ALL, ids=IDS)
def test_case_notices_deliberate_mistakes(built, case, fmt):
    data, res, _ = built(case, fmt)
    assert differs(case, fmt, res, E.restate(case, data, fmt, mode="toward-zero")), "a truncating conversion goes unnoticed"
    assert differs(case, fmt, res, E.restate(case, data, fmt, drop_last=32)), "a dropped last tile of 32 samples goes unnoticed"
    matrix = 1 if case.H > 1 else 0
    assert differs(case, fmt, res, E.restate(case, data, fmt, swap=(matrix, 3, 4))), "two exchanged K indices go unnoticed"
    # each mistake alone, on the tensor it is about
    assert not np.array_equal(E.restate(case, data, fmt, drop_last=32).grads, res.grads)
    assert not np.array_equal(E.restate(case, data, fmt, swap=(matrix, 3, 4)).out, res.out)
    assert not np.array_equal(E.restate(case, data, fmt, mode="toward-zero").out, res.out)


def test_round16_is_the_oracles_conversion():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(4096) * np.exp2(rng.integers(-20, 14, 4096)), [0.0, 1.0 - 2.0 ** -13, 1.0 + 2.0 ** -12, 2049.0, 2051.0, 65504.0]])
    v = v.astype(np.float32).astype(np.float64)
    for fmt in (E.FP16, E.BF16):
        with half_format(fmt):
            r = E.round16(v, fmt)
            keep = ~((v < 0) & (r == 0))  # (a negative number that underflows keeps its sign in the oracle and is +0 here; C2 keeps every case away from it)
            assert np.array_equal(E.to_bits(r, fmt)[keep], O.f2h(v)[keep])
            assert np.array_equal(E.from_bits(O.f2h(v), fmt), O.h2f(O.f2h(v)).astype(np.float64))
    assert E.round16(2049.0) == 2048.0 and E.round16(2051.0) == 2052.0 and E.round16(2051.0, mode="toward-zero") == 2050.0  # ties to even

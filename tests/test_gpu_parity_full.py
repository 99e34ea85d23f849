"""Parity of the training step AT THE SIZE THE BENCH RUNS (BASELINE.json configs[2]: HashGrid L16 F2 T=2^19 scale 2.0 +
FullyFusedMLP 64x2, N = 2^18) against the CPU oracle, plus the optional arguments of Trainer::training_step
(trainer.h:254-264) and a bit-level check of the optimizer.

At this size every wavefront of k_mlp_train_wave walks several 32-sample strips (prefetch of the next strip, weight
gradients accumulated across strips) and the grid backward runs its bucketed form with full queues -- the code paths
that the small cases of test_gpu_parity.py do not reach.

Bars (the fp16 tolerance of BASELINE.json's north_star, stated here):
  * loss: 2e-3 relative; prediction: RAE p99 <= 3e-3 (the reference's own bar for its kernels is 1e-2, tests/test_common.h);
  * loss gradient: bit-exact given the GPU's own prediction;
  * network weight gradients: RAE p99 <= 5e-3 and relative L2 <= 2e-3;
  * grid gradients, per level: relative L2 <= 1e-2, RAE p99 <= 3e-2 over the entries above 1 % of the level's maximum;
  * the GPU's distance from the fp32-accumulate oracle is below the distance between the oracle's fp16-accumulate mode
    (the reference's own accumulator type, fully_fused_mlp.cu:68,198) and its fp32-accumulate mode;
  * Adam: first / second moments and step counters bit-exact, fp32 master weights within 4 ulp (powf of the bias
    correction is not correctly rounded on either side), fp16 weights = RNE of the GPU's own master weights.
"""
import math
import msgpack
import numpy as np
import pytest
import torch

from conftest import config_hash
from oracle import oracle as O
from test_gpu_parity import _trainer_and_oracle, h_np, h_t, positions, rae, targets_for, tcnn

pytestmark = pytest.mark.gpu


def _scaled_init(tm, md, scale=1.0e3):
    init = tm.params_full_precision.cpu().numpy().copy()
    init[md.mlp.n_params:] *= scale  # grid.h:1076-1079 initialises in U(-1e-4, 1e-4): mostly fp16 subnormals
    tm.set_params_full_precision(torch.from_numpy(init))
    return init


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize("d,out,log2_t,per_level_scale", [(3, 4, 19, 2.0), (3, 4, 19, 1.5), (2, 3, 15, 1.5)],
                         ids=["headline-scale2.0", "headline-scale1.5", "hash_shipped-2d-T15"])
def test_headline_training_step_matches_oracle_at_full_size(d, out, log2_t, per_level_scale):
    """Both scales SURVEY 8's headline lists: 2.0 (three dense levels, thirteen hashed power-of-two tables) and data/config_hash.json's 1.5
    (four dense levels whose sizes are no powers of two, resolutions 16 ... 7007); and data/config_hash.json AS SHIPPED -- 2-D -> 3,
    T = 2^15, the one configuration the reference publishes a figure for and `bench.py --workload hash_shipped` measures -- at the batch
    it is benchmarked at (six dense 2-D levels, ten hashed tables of 2^15 entries that a batch of 2^18 samples hits 32 times per entry)."""
    cfg = config_hash(log2_hashmap_size=log2_t, per_level_scale=per_level_scale)
    tm, md = _trainer_and_oracle(cfg, d, out)
    init = _scaled_init(tm, md)
    st, st16 = O.TrainState(md, init), O.TrainState(md, init)
    n = 1 << 18
    pos = positions(n, d, seed=77)
    tgt = targets_for(pos, out)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    nm = md.mlp.n_params

    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    loss16, pred16 = O.training_step(st16, pos, tgt, run_optimizer=False, want_prediction=True, accum_fp16=True)

    loss = tm.loss(ctx)
    assert abs(loss - loss_ref) <= 2e-3 * abs(loss_ref), (loss, loss_ref)
    pred = O.h2f(h_np(ctx.output))
    pr, p16 = O.h2f(pred_ref), O.h2f(pred16)
    assert np.percentile(rae(pred[:, :out], pr[:, :out]), 99) < 3e-3
    assert np.percentile(rae(pred, pr), 99) < 3e-3  # the padded output rows are computed like the live ones (fully_fused_mlp.cu:656)
    _, g_loss = O.loss(md.loss_type, h_np(ctx.output), tgt, out)
    assert np.array_equal(h_np(ctx.dL_doutput), g_loss)

    g = tm.param_gradients.float().cpu().numpy()
    gref, g16 = O.h2f(st.grads), O.h2f(st16.grads)
    assert np.isfinite(g).all()
    assert np.percentile(rae(g[:nm], gref[:nm]), 99) < 5e-3, np.percentile(rae(g[:nm], gref[:nm]), [50, 99, 100])
    assert _rel_l2(g[:nm], gref[:nm]) < 2e-3
    off = np.asarray(md.grid.offsets[:md.grid.n_levels + 1], np.int64) * md.grid.n_features_per_level
    for l in range(md.grid.n_levels):
        a, b = g[nm + off[l]:nm + off[l + 1]], gref[nm + off[l]:nm + off[l + 1]]
        assert _rel_l2(a, b) < 1e-2, (l, _rel_l2(a, b))
        big = np.abs(b) > 1e-2 * np.abs(b).max()
        assert np.percentile(rae(a[big], b[big]), 99) < 3e-2, l
        # entries no sample touched are exactly zero on both sides (the optimizer skips them, adam.h:79-82)
        assert np.array_equal(a == 0, b == 0) or np.mean((a == 0) != (b == 0)) < 1e-3, l

    # bracket: fp32-accumulate MFMA sits closer to the fp32-accumulate oracle than the reference's fp16 accumulators do
    assert np.abs(pred[:, :out] - pr[:, :out]).mean() <= np.abs(p16[:, :out] - pr[:, :out]).mean()
    assert _rel_l2(g[:nm], gref[:nm]) <= _rel_l2(g16[:nm], gref[:nm])
    assert _rel_l2(g[nm:], gref[nm:]) <= _rel_l2(g16[nm:], gref[nm:])

    # one optimizer step from the GPU's own gradients: the oracle's Adam fed with the same fp16 gradients
    ref = O.TrainState(md, init)
    ref.step = 1
    O.adam_step(md.adam, nm, 128.0, 1, ref.w32, ref.w16, h_np(tm.param_gradients), ref.m1, ref.m2, ref.steps)
    tm.optimizer_step()
    w = tm.params_full_precision.cpu().numpy()
    assert _within_ulps(w, ref.w32, init)
    assert np.array_equal(h_np(tm.params), O.f2h(w))
    # ... and the step itself tracks the oracle's own step (first Adam step = -lr * sign(gradient))
    O.training_step(st, pos, tgt)
    assert np.mean(np.abs(w - st.w32) > 1e-3) < 2e-3


def test_stress_shape_training_step_at_its_stated_size_in_fp16():
    """BASELINE.json configs[4] AT ITS STATED SIZE in the fp16 library (tests/bf16_cases.py holds the same step against the bfloat16 build,
    the precision configs[4] names; `bench.py --workload stress` quotes an fp16 line as well): HashGrid(L = 16, F = 2, T = 2^22,
    per_level_scale 1.5) + FullyFusedMLP 128 x 4, 3-D -> 16, N = 2^18.  At this size the gather plan carries its L2-miss term, the 128-wide
    single-kernel training pass (k_mlp_train_wide) walks 8192 tiles, the bucketed backward holds 512 buckets per hashed level and Adam
    streams its state.  Bars as for the headline (fp16): encoded features bit-exact; loss 2e-3; prediction RAE p99 <= 3e-3; loss gradient
    bit-exact on the GPU's own prediction; network gradients relative L2 <= 5e-3; grid gradients per level relative L2 <= 1e-2, untouched
    entries exactly zero on both sides; then one Adam step: moments and counters bit-exact, master weights within 4 ulp."""
    T = tcnn()
    n, out, log2_t = 1 << 18, 16, 22
    cfg = config_hash(log2_hashmap_size=log2_t, per_level_scale=1.5, n_neurons=128, n_hidden_layers=4)
    tm, md = _trainer_and_oracle(cfg, 3, out)
    assert tm.n_params == md.n_params
    init = _scaled_init(tm, md)
    nm = md.mlp.n_params
    st = O.TrainState(md, init)
    pos = positions(n, 3, seed=91)
    tgt = np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c % 4 + 1) * pos[:, 0]) * np.cos(2 * np.pi * pos[:, 1]) for c in range(out)], 1).astype(np.float32)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()

    e = T._C.create_encoding(3, cfg["encoding"])  # the gather alone, through the encoding module on the trainer's table
    _, enc = e.fwd(x, tm.params[nm:].contiguous())
    assert np.array_equal(h_np(enc), O.grid_forward(md.grid, O.f2h(init[nm:]), pos))
    del enc

    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-3 * abs(loss_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(pred_ref)), 99) < 3e-3
    _, g_loss = O.loss(md.loss_type, h_np(ctx.output), tgt, out)
    assert np.array_equal(h_np(ctx.dL_doutput), g_loss)
    g, gref = tm.param_gradients.float().cpu().numpy(), O.h2f(st.grads)
    assert np.isfinite(g).all()
    assert _rel_l2(g[:nm], gref[:nm]) < 5e-3, _rel_l2(g[:nm], gref[:nm])
    off = np.asarray(md.grid.offsets[:md.grid.n_levels + 1], np.int64) * md.grid.n_features_per_level
    for l in range(md.grid.n_levels):
        a, b = g[nm + off[l]:nm + off[l + 1]], gref[nm + off[l]:nm + off[l + 1]]
        assert _rel_l2(a, b) < 1e-2, (l, _rel_l2(a, b))
        assert np.array_equal(a == 0, b == 0) or np.mean((a == 0) != (b == 0)) < 1e-3, l

    ref = O.TrainState(md, init)
    ref.step = 1
    O.adam_step(md.adam, nm, 128.0, 1, ref.w32, ref.w16, h_np(tm.param_gradients), ref.m1, ref.m2, ref.steps)
    tm.optimizer_step()
    w = tm.params_full_precision.cpu().numpy()
    assert _within_ulps(w, ref.w32, init)
    assert np.array_equal(h_np(tm.params), O.f2h(w))
    m1, m2, steps, _ = _optimizer_state(tm)
    assert np.array_equal(m1, ref.m1) and np.array_equal(m2, ref.m2) and np.array_equal(steps, ref.steps)


def _within_ulps(w, w_ref, w_before, ulps=4):
    """|w - w_ref| <= `ulps` units in the last place of the larger of the old weight, the new weight and the largest Adam
    update (~3 lr): the update is a difference, so a result close to zero carries the absolute error of its operands."""
    scale = np.maximum(np.maximum(np.abs(w_before), np.abs(w_ref)), np.float32(0.03))
    return bool((np.abs(w - w_ref) <= ulps * np.spacing(scale)).all())


def _optimizer_state(tm):
    doc = msgpack.unpackb(tm.serialize(serialize_optimizer=True), raw=False)
    o = doc["optimizer"]
    return (np.frombuffer(o["first_moments_binary"], np.float32), np.frombuffer(o["second_moments_binary"], np.float32),
            np.frombuffer(o["param_steps_binary"], np.uint32), o["current_step"])


@pytest.mark.parametrize("l2_reg,clip", [(1e-6, 0.0), (0.0, 0.5)])
def test_adam_bit_level_in_both_step_counter_forms(l2_reg, clip):
    """optimizers/adam.h:48-127 on identical fp16 gradients: moments, per-parameter step counters exact in the counter
    form, the deficit form and across both flips; skipped (zero-gradient) hash entries keep their state."""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=12, per_level_scale=1.5)
    cfg["optimizer"] = dict(cfg["optimizer"], l2_reg=l2_reg, gradient_clipping_magnitude=clip, non_matrix_learning_rate_factor=0.5)
    tm = T.create_from_config(3, 4, cfg)
    og = O.grid_init(3, 16, 2, 12, 16, 1.5)
    adam = O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=l2_reg, gradient_clipping_magnitude=clip,
                           non_matrix_learning_rate_factor=0.5)
    md = O.model_init(3, 4, og, 64, 2, O.LOSS_RELATIVE_L2, adam)
    n, nm = tm.n_params, tm.n_mlp_params
    assert n == md.n_params
    st = O.TrainState(md, tm.params_full_precision.cpu().numpy())
    rng = np.random.default_rng(3)
    # global batch -> representation (trainer_optimizer.hip choose_step_representation): 1 sample keeps counters, 2^20 samples deficits
    schedule = [1, 1, 1 << 20, 1 << 20, 1 << 20, 1, 1, 1 << 20]
    for k, batch in enumerate(schedule):
        g = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 60.0], n)).astype(np.float16)
        g[nm:][rng.random(n - nm) < 0.4] = 0  # untouched hash entries: skipped, their counters fall behind
        tm.set_global_batch_size(batch)
        tm.param_gradients.copy_(h_t(g.view(np.uint16)))
        tm.optimizer_step()
        st.step += 1
        w_before = st.w32.copy()
        O.adam_step(md.adam, nm, 128.0, st.step, st.w32, st.w16, g.view(np.uint16), st.m1, st.m2, st.steps)
        m1, m2, steps, current = _optimizer_state(tm)
        assert current == st.step
        assert np.array_equal(steps, st.steps), k
        assert np.array_equal(m1, st.m1) and np.array_equal(m2, st.m2), k
        w = tm.params_full_precision.cpu().numpy()
        assert _within_ulps(w, st.w32, w_before), k
        assert np.array_equal(h_np(tm.params), O.f2h(w)), k
        st.w32[:] = w  # continue from the GPU's master weights so that ulp-level differences do not compound
        st.w16[:] = O.f2h(w)
    assert len(np.unique(st.steps)) > 3  # the skip path was exercised


def test_adam_byte_deficits_beyond_254_skipped_steps():
    """The step-counter deficits kept as bytes (trainer_optimizer.hip choose_step_representation; elementwise_kernels.h AdamStepsForm): entries that are
    skipped more than 254 times in a row move into the 32-bit counter array (byte 255) and keep their exact count -- 300 optimizer steps on
    the GPU against the oracle's counters, with a snapshot (which converts to counters and back) in the middle."""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=10, per_level_scale=1.5)
    tm = T.create_from_config(3, 4, cfg)
    n, nm = tm.n_params, tm.n_mlp_params
    tm.set_global_batch_size(1 << 20)  # deficit form
    rng = np.random.default_rng(12)
    counters = np.zeros(n, np.uint32)
    never = np.arange(nm + 64, nm + 640)  # grid entries that see a gradient at steps 1 and 290 only
    for step in range(1, 301):
        g = (rng.standard_normal(n) * 0.1).astype(np.float16)
        g[nm:][rng.random(n - nm) < 0.3] = 0
        if step not in (1, 290):
            g[never] = 0
        tm.param_gradients.copy_(h_t(g.view(np.uint16)))
        tm.optimizer_step()
        stepped = np.ones(n, bool)
        stepped[nm:] = g[nm:] != 0  # adam.h:79-82: zero-gradient non-matrix entries are skipped
        counters += stepped
        if step in (100, 270, 300):
            _, _, steps, current = _optimizer_state(tm)  # serialises: bytes -> counters (and back at the next step)
            assert current == step and np.array_equal(steps, counters), step
    assert counters[never].max() == 2 and counters[:nm].min() == 300


def test_parameters_written_through_the_exposed_pointers_survive_the_optimizer():
    """tcnn_trainer_params / _params_full_precision hand out mutable pointers (trainer.h:489-503).  The reference's Adam leaves the 16-bit weight
    of a skipped (zero-gradient) entry untouched (adam.h:79-82); the library's shortcut "16-bit weight = rounded master weight" must
    therefore be off while a caller holds either pointer, and tcnn_trainer_params_written must bring the master weights in line with what
    was written before the shortcut is trusted again."""
    T = tcnn()
    tm = T.create_from_config(3, 4, config_hash(log2_hashmap_size=12, per_level_scale=1.5))
    n, nm = tm.n_params, tm.n_mlp_params
    tm.set_global_batch_size(1 << 20)  # deficit form of the step counters: the form whose mixed lanes re-derive skipped weights
    rng = np.random.default_rng(3)

    def step_with_sparse_gradient():
        g = (rng.standard_normal(n) * 0.1).astype(np.float16)
        g[nm:][rng.random(n - nm) < 0.5] = 0  # half of the grid entries are skipped: most lanes of four are mixed
        tm.param_gradients.copy_(h_t(g.view(np.uint16)))
        tm.optimizer_step()
        return g

    step_with_sparse_gradient()
    # (1) a caller writes the 16-bit parameters directly and says so
    written = nm + rng.choice(n - nm, 500, replace=False)
    p = tm.params  # exposes the buffer
    before_master = tm.params_full_precision.cpu().numpy().copy()
    new16 = (rng.standard_normal(500) * 0.5).astype(np.float16)
    p[torch.from_numpy(written).cuda()] = h_t(new16.view(np.uint16))
    tm.params_written()
    master = tm.params_full_precision.cpu().numpy()
    assert np.array_equal(master[written], new16.astype(np.float32))  # re-derived from what was written
    untouched = np.setdiff1d(np.arange(n), written)
    assert np.array_equal(master[untouched].view(np.uint32), before_master[untouched].view(np.uint32))  # the others keep their extra bits
    g = step_with_sparse_gradient()
    skipped = written[g[written] == 0]
    assert len(skipped) > 100
    assert np.array_equal(h_np(tm.params)[skipped], new16[g[written] == 0].view(np.uint16))  # skipped entries keep the written value

    # (2) a caller holds the MASTER pointer and writes it (no params_written yet): skipped 16-bit weights stay what they were
    p16_before = h_np(tm.params).copy()
    tm.params_written()  # the shortcut is trusted again (this call leaves the 16-bit buffer as it is) ...
    pm = tm.params_full_precision_mutable  # ... and the master pointer is the only one out
    pm[torch.from_numpy(written).cuda()] = torch.from_numpy((new16.astype(np.float32) * 3.0)).cuda()
    g = step_with_sparse_gradient()
    skipped = written[g[written] == 0]
    assert len(skipped) > 100 and np.array_equal(h_np(tm.params)[skipped], p16_before[skipped])


def test_reading_the_master_weights_does_not_change_the_trainer_s_mode():
    """tcnn_trainer_params_full_precision_view: a host that only reads the master weights -- logging, a checkpoint -- must not
    switch off Adam's "16-bit weights follow the master weights" shortcut for good.  Observable: with the shortcut ON the 16-bit weight of a
    skipped entry is re-derived from the master weight, so a master weight changed behind the library's back (through the mutable pointer of
    ANOTHER handle on the same memory: here a raw view made before) shows up in the 16-bit buffer of a skipped entry; with it OFF it would not."""
    T = tcnn()
    tm = T.create_from_config(3, 4, config_hash(log2_hashmap_size=12, per_level_scale=1.5))
    n, nm = tm.n_params, tm.n_mlp_params
    tm.set_global_batch_size(1 << 20)
    rng = np.random.default_rng(4)
    view = tm.params_full_precision_view  # read-only accessor: same memory, no mode change
    assert view.data_ptr() == tm.params_full_precision_view.data_ptr()
    assert tm.params_full_precision.data_ptr() != view.data_ptr()  # (the plain accessor hands out a copy: ADVICE round 5)
    before = view.cpu().numpy().copy()
    g = (rng.standard_normal(n) * 0.1).astype(np.float16)
    g[nm:][rng.random(n - nm) < 0.5] = 0
    tm.param_gradients.copy_(h_t(g.view(np.uint16)))
    probe = nm + np.flatnonzero(g[nm:] == 0)[:64]
    # lanes of four that mix stepped and skipped parameters re-derive the skipped ones: find probes whose lane is mixed
    lane = (probe // 4) * 4
    mixed = np.array([np.any(g[l:l + 4] != 0) for l in lane])
    probe = probe[mixed]
    assert len(probe) > 8
    view[torch.from_numpy(probe).cuda()] = 0.75  # (torch lets us write through the view; the library was told nothing)
    tm.optimizer_step()
    torch.cuda.synchronize()
    got = h_np(tm.params)[probe]
    assert np.array_equal(got, np.full(len(probe), np.float16(0.75)).view(np.uint16)), "the shortcut is off: the read-only view changed the trainer's mode"
    assert not np.array_equal(before[probe], np.full(len(probe), 0.75, np.float32))


def test_optimizer_object_on_its_own_bit_level():
    """tcnn_create_optimizer / Optimizer<T>::allocate + step (optimizer.h:52-60) over buffers the caller owns: the trainer's Adam kernel
    behind another door -- moments and per-parameter step counters bit-equal to the oracle's adam_step (itself pinned against the
    reference's kernel), master weights within ulps, 16-bit weights = RNE of the master weights; zero-gradient non-matrix entries skipped."""
    from tinycudann import native
    n, nm = 40000, 4096
    cfg = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6, "non_matrix_learning_rate_factor": 0.5}
    adam = O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=1e-6, non_matrix_learning_rate_factor=0.5)
    rng = np.random.default_rng(5)
    w32 = rng.standard_normal(n).astype(np.float32)
    w16 = O.f2h(w32)
    m1, m2, steps = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    opt = native.Optimizer(cfg, n, nm)
    wfp = torch.from_numpy(w32.copy()).cuda()
    wh = h_t(w16.copy())
    for k in range(4):
        g = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 60.0], n)).astype(np.float16)
        g[nm:][rng.random(n - nm) < 0.4] = 0
        opt.step(wfp, wh, h_t(g.view(np.uint16)))
        w_before = w32.copy()
        O.adam_step(adam, nm, 128.0, k + 1, w32, w16, g.view(np.uint16), m1, m2, steps)
        gm1, gm2, gsteps = opt.state()
        torch.cuda.synchronize()
        assert opt.step_count == k + 1
        assert np.array_equal(gsteps.cpu().numpy().view(np.uint32), steps) and np.array_equal(gm1.cpu().numpy(), m1) and np.array_equal(gm2.cpu().numpy(), m2), k
        w = wfp.cpu().numpy()
        assert _within_ulps(w, w32, w_before), k
        assert np.array_equal(h_np(wh), O.f2h(w)), k
        w32[:] = w
        w16[:] = O.f2h(w)
    assert len(np.unique(steps)) > 2
    with pytest.raises(RuntimeError, match="not available"):
        native.Optimizer({"otype": "Shampoo"}, 8)


def test_training_step_data_pdf_external_gradient_and_input_gradient():
    """data_pdf, external_dL_dy and dL_dinput of Trainer::training_step (trainer.h:254-264) against the oracle."""
    cfg = config_hash(log2_hashmap_size=15, per_level_scale=1.5)
    tm, md = _trainer_and_oracle(cfg, 3, 4)
    init = _scaled_init(tm, md)
    nm = md.mlp.n_params
    n = 8192
    pos = positions(n, 3, seed=31)
    tgt = targets_for(pos, 4)
    pdf = (0.5 + 1.5 * O.generate_random_uniform(O.pcg32(8), n * 4)).reshape(n, 4).astype(np.float32)
    x, t, p = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(pdf).cuda()

    def check_grads(g, gref):
        assert np.percentile(rae(g[:nm], gref[:nm]), 99) < 5e-3
        big = np.abs(gref[nm:]) > 1e-2 * np.abs(gref[nm:]).max()
        assert np.percentile(rae(g[nm:][big], gref[nm:][big]), 99) < 3e-2
        assert _rel_l2(g[nm:], gref[nm:]) < 1e-2

    # ---- data_pdf + dL_dinput through the fused training kernel
    st = O.TrainState(md, init)
    dx_ref = np.zeros((n, 3), np.float32)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True, data_pdf=pdf, dL_dinput=dx_ref)
    dx = torch.zeros((n, 3), device="cuda")
    ctx = tm.training_step(x, t, data_pdf=p, run_optimizer=False, dL_dinput=dx)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-3 * abs(loss_ref)
    _, g_loss = O.loss(md.loss_type, h_np(ctx.output), tgt, 4, data_pdf=pdf)
    assert np.array_equal(h_np(ctx.dL_doutput), g_loss)
    check_grads(tm.param_gradients.float().cpu().numpy(), O.h2f(st.grads))
    assert _rel_l2(dx.cpu().numpy(), dx_ref) < 2e-2
    # without the pdf the gradients differ (the argument is not ignored)
    ctx0 = tm.training_step(x, t, run_optimizer=False)
    assert not np.array_equal(h_np(ctx0.dL_doutput), g_loss)

    # ---- external_dL_dy (the loss is not evaluated, trainer.h:124-128; the fused network kernel continues from the caller's gradient)
    ext = O.f2h(O.h2f(g_loss) * 0.5 + 0.25 * (O.h2f(g_loss) != 0))
    st = O.TrainState(md, init)
    dx_ref = np.zeros((n, 3), np.float32)
    O.training_step(st, pos, None, run_optimizer=False, external_dL_dy=ext, dL_dinput=dx_ref)
    dx = torch.zeros((n, 3), device="cuda")
    ctx = tm.training_step(x, t, run_optimizer=False, dL_dinput=dx, external_dL_dy=h_t(ext))
    assert np.array_equal(h_np(ctx.dL_doutput), ext)
    check_grads(tm.param_gradients.float().cpu().numpy(), O.h2f(st.grads))
    assert _rel_l2(dx.cpu().numpy(), dx_ref) < 2e-2
    with pytest.raises(RuntimeError):
        tm.loss(ctx)


@pytest.mark.parametrize("n,log2_t,cfg_kw", [(1 << 18, 19, {}), (4096, 15, {"per_level_scale": 1.5}), (1 << 16, 17, {"n_neurons": 128, "n_hidden_layers": 4}),
                                             (8192, 15, {"n_neurons": 32, "n_hidden_layers": 3})])
def test_weight_gradient_slabs_summed_inside_the_optimizer_launch_equal_the_separate_kernel(n, log2_t, cfg_kw):
    """tcnn_set_finalize_in_optimizer: training_step(run_optimizer = True) sums the network kernel's fp32 weight-gradient slabs in the first
    workgroups of k_adam_step's launch (AdamFinalize) -- the same additions in the same order as k_mlp_finalize_gradients -- and steps those
    parameters there.  From identical states a step with and a step without it leave bit-identical network gradients, 16-bit and master
    weights and optimizer state (the register-order slabs of the wave kernels, the parameter-order slabs of the 128-wide kernel); also after
    a step that did NOT run the optimizer (run_optimizer = False falls back to the kernel of its own).  The encoding's part is the same
    code either way and is compared as the run-to-run spread of its coarse levels' packed-half atomics allows (chunked small tables)."""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=log2_t, **cfg_kw)
    a, b = T.create_from_config(3, 4, cfg, seed=11), T.create_from_config(3, 4, cfg, seed=12)
    w = a.params_full_precision.cpu().numpy().copy()
    nm = a.n_mlp_params
    w[nm:] *= 1.0e3
    a.set_params_full_precision(torch.from_numpy(w))
    try:
        for step in range(5):
            b.deserialize(a.serialize(serialize_optimizer=True))  # identical weights and optimizer state
            b.set_params_full_precision(a.params_full_precision.clone())  # (snapshots carry the 16-bit weights: the master weights as well)
            pos = positions(n, 3, seed=100 + step)
            x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()
            run = step != 3  # one step without the optimizer in between
            T._C.set_finalize_in_optimizer(True)
            a.training_step(x, t, run_optimizer=run)
            T._C.set_finalize_in_optimizer(False)
            b.training_step(x, t, run_optimizer=run)
            ga, gb = a.param_gradients, b.param_gradients
            assert torch.equal(ga[:nm].view(torch.int16), gb[:nm].view(torch.int16)), step
            assert ga[:nm].float().abs().max() > 0
            assert torch.equal(a.params[:nm].view(torch.int16), b.params[:nm].view(torch.int16)), step
            assert torch.equal(a.params_full_precision[:nm].view(torch.int32), b.params_full_precision[:nm].view(torch.int32)), step
            for u, v in zip(_optimizer_state(a)[:3], _optimizer_state(b)[:3]):
                assert np.array_equal(u[:nm], v[:nm]), step
            d = (ga[nm:].float() - gb[nm:].float()).abs()
            assert float(d.max()) <= 2.0 ** -8 * float(ga[nm:].float().abs().max()) and float((d > 0).float().mean()) < 0.05, step
    finally:
        T._C.set_finalize_in_optimizer(True)


def test_training_step_as_one_graph_launch_leaves_the_plain_steps_bits():
    """tcnn_trainer_set_graph_capture (trainer.h:343-350, cuda_graph.h:65-155: the reference records its passes into a CUDA graph on every
    call, patches the instantiated graph and launches it): on a non-null stream every training_step after the first of a shape is ONE graph
    launch.  From identical states a captured and a plain step leave bit-identical network gradients, weights and optimizer state and the same
    prediction in the context (the encoding's part within the run-to-run spread of its coarse levels' packed-half atomics); a new batch size
    runs plainly once and is captured again; the null stream and profiled steps are never captured."""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=15, per_level_scale=1.5)
    a, b = T.create_from_config(3, 4, cfg, seed=21), T.create_from_config(3, 4, cfg, seed=22)
    nm = a.n_mlp_params
    side = torch.cuda.Stream()
    a.set_graph_capture(True)
    expected_launches = 0
    seen_shapes = set()
    with torch.cuda.stream(side):
        for step, n in enumerate([4096, 4096, 4096, 1024, 1024, 4096, 4096]):
            b.deserialize(a.serialize(serialize_optimizer=True))
            b.set_params_full_precision(a.params_full_precision.clone())
            pos = positions(n, 3, seed=300 + step)
            x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()
            side.synchronize()
            want_ctx = n == 4096
            ca = a.training_step(x, t, want_context=want_ctx)
            cb = b.training_step(x, t, want_context=want_ctx)
            side.synchronize()
            # the first step of a shape runs plainly (it fills the stream's scratch cache); a step of another shape forgets the previous one
            shape = (n, want_ctx)
            if seen_shapes == {shape}:
                expected_launches += 1
            seen_shapes = {shape}
            assert a.graph_capture_stats()[0] == expected_launches, (step, a.graph_capture_stats())
            if want_ctx:
                assert torch.equal(ca.output.view(torch.int16), cb.output.view(torch.int16)), step
                assert abs(a.loss(ca) - b.loss(cb)) <= 1e-6 * abs(b.loss(cb)), step
            ga, gb = a.param_gradients, b.param_gradients
            assert torch.equal(ga[:nm].view(torch.int16), gb[:nm].view(torch.int16)), step
            assert torch.equal(a.params[:nm].view(torch.int16), b.params[:nm].view(torch.int16)), step
            assert torch.equal(a.params_full_precision[:nm].view(torch.int32), b.params_full_precision[:nm].view(torch.int32)), step
            for u, v in zip(_optimizer_state(a)[:3], _optimizer_state(b)[:3]):
                assert np.array_equal(u[:nm], v[:nm]), step
            d = (ga[nm:].float() - gb[nm:].float()).abs()
            assert float(d.max()) <= 2.0 ** -8 * float(ga[nm:].float().abs().max()) and float((d > 0).float().mean()) < 0.05, step
    launches, instantiations = a.graph_capture_stats()
    assert launches == expected_launches and launches >= 2 and 1 <= instantiations <= launches
    assert b.graph_capture_stats() == (0, 0)
    # the null stream is never captured (cuda_graph.h:67-69), a profiled step neither (its events would be recorded into the graph)
    pos = positions(4096, 3, seed=99)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()
    for _ in range(3):
        a.training_step(x, t)
    assert a.graph_capture_stats()[0] == launches
    a.set_profiling(True)
    with torch.cuda.stream(side):
        for _ in range(3):
            a.training_step(x, t)
    a.set_profiling(False)
    torch.cuda.synchronize()
    assert a.graph_capture_stats()[0] == launches
    a.set_graph_capture(False)
    with torch.cuda.stream(side):
        for _ in range(3):
            a.training_step(x, t)
    torch.cuda.synchronize()
    assert a.graph_capture_stats()[0] == launches and math.isfinite(a.loss(a.training_step(x, t)))


@pytest.mark.parametrize("scale,offset,loss,hidden_layers", [(1.0, 0.0, "L2", 2), (0.5, 0.25, "RelativeL2", 2), (1.0, 0.0, "RelativeL2", 1)])
def test_network_kernel_reading_the_fp32_input_of_an_identity_encoding_itself(scale, offset, loss, hidden_layers):
    """BASELINE configs[1] (64 inputs -> 64 x 2 -> 16, Identity encoding): training_step lets the register-resident network kernel load the
    caller's fp32 matrix itself (MlpF32Input, tcnn_set_fused_identity_input) instead of running the encoding as a transpose kernel in front of
    it.  Prediction, loss, gradients, parameters and optimizer state after several steps must equal the two-kernel path's BIT FOR BIT, the
    returned context must still carry what `loss()` and a later `backward()` need, and the kernel that ran must be the fused one (no encoding
    stage in the profile)."""
    T = tcnn()
    C = T._C
    cfg = {"loss": {"otype": loss}, "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6},
           "encoding": {"otype": "Identity", "scale": scale, "offset": offset},
           "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": hidden_layers}}
    n = (1 << 16) + 256
    g = torch.Generator().manual_seed(5)
    x = (torch.rand((n, 64), generator=g) * 2 - 1).cuda()
    t = torch.rand((n, 16), generator=g).cuda()
    results = {}
    try:
        for fused in (True, False):
            C.set_fused_identity_input(fused)
            tm = T.create_from_config(64, 16, cfg, seed=9)
            tm.set_profiling(True)
            losses = []
            for _ in range(4):
                ctx = tm.training_step(x, t)
                losses.append(tm.loss(ctx))
            stages = {k for k, (ms, c) in tm.stage_times().items() if c}
            tm.set_profiling(False)
            tm.training_step(x, t, want_context=False)  # (no context asked for: the kernel does not write the encoded matrix at all)
            inferred = tm.inference(x).clone()  # the inference kernel reads the fp32 input itself as well (no encoding kernel, no encoded matrix)
            ctx = tm.training_step(x, t, run_optimizer=False)
            pred = ctx.output.clone()
            grads_step = tm.param_gradients.clone()
            tm.backward(ctx, x)  # the context's encoded input, whoever wrote it, feeds the recomputing backward pass
            torch.cuda.synchronize()
            m1, m2, steps, _ = tm.optimizer_state()
            results[fused] = (losses, pred, grads_step, tm.param_gradients.clone(), tm.params_full_precision.clone(), m1.clone(), m2.clone(), steps.clone(), stages, inferred)
    finally:
        C.set_fused_identity_input(True)
    # a PyTorch module's inference (no_grad: tcnn_module_inference, padded 16-bit output) takes the same way in
    net_out = {}
    try:
        for fused in (True, False):
            C.set_fused_identity_input(fused)
            net = T.Network(64, 16, cfg["network"], seed=3)
            with torch.no_grad():
                net_out[fused] = net(x).clone()
    finally:
        C.set_fused_identity_input(True)
    assert net_out[True].dtype == torch.half and torch.equal(net_out[True].view(torch.int16), net_out[False].view(torch.int16)) and torch.isfinite(net_out[True].float()).all()
    a, b = results[True], results[False]
    assert a[0] == b[0] and a[0][-1] < a[0][0]
    for u, v in zip(a[1:8], b[1:8]):
        assert torch.equal(u.view(torch.int16) if u.dtype == torch.half else u, v.view(torch.int16) if v.dtype == torch.half else v)
    # (a[3] == b[3] above: backward(ctx) recomputes from the context's encoded input, which the network kernel left behind in one case and the
    # encoding kernel wrote in the other)
    assert float((a[2].float() - a[3].float()).abs().max()) <= 2.0 ** -9 * float(a[2].float().abs().max())  # and reproduces the step's gradients
    assert "grid_forward" in b[8] and "grid_forward" not in a[8] and "mlp_train_fused" in a[8]  # (the encoding stage is named after its first user)
    assert torch.equal(a[9], b[9]) and torch.isfinite(a[9]).all()

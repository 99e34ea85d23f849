"""Parity cases of the bfloat16 build (libtcnn_hip_bf16.so: the same sources compiled with -DTCNN_BF16, bf16 MFMA tiles,
bf16 parameters / activations / gradients) against the oracle's bfloat16 mode.  Run by tests/test_gpu_bf16.py in a process
of its own with TCNN_PRECISION=bf16 (the 16-bit type is a build-time choice of the library, one library per process).

Bars: grid indices and encoded features bit-exact (the bf16 interpolation chain is an fp32 fma rounded to bf16 on both
sides); loss gradients bit-exact given the GPU's own prediction; network outputs / gradients RAE p99 <= 3e-2 (bf16 has 8
significant bits: 8x fp16's spacing, and the fp16 bar is 3e-3); training converges.
"""
import os

import numpy as np
import pytest
import torch

from conftest import ADAM_HASH, HASH_ENCODING, HASH_ENCODING_SMALL, MLP_64x2, config_hash
from oracle import oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(autouse=True, scope="module")
def _bf16_oracle():
    O.set_half_format(True)
    yield
    O.set_half_format(False)


def tcnn():
    import tinycudann
    return tinycudann


def h_np(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def h_t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(BF).cuda()


def rae(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (0.5 * (np.abs(a) + np.abs(b)) + np.abs(b).mean() * 1e-2 + 1e-12)


def positions(n, d, seed=1337):
    return O.generate_random_uniform(O.pcg32(seed), n * d, 0.0, 1.0).reshape(n, d)


def targets_for(pos, out):
    return np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c % 4 + 1) * pos[:, 0]) * np.cos(2 * np.pi * pos[:, 1]) for c in range(out)], 1).astype(np.float32)


def test_the_bf16_library_is_the_one_loaded():
    T = tcnn()
    assert os.environ.get("TCNN_PRECISION") == "bf16"
    assert T._C.library_path().endswith("libtcnn_hip_bf16.so") and "libtcnn_hip_bf16.so" in open("/proc/self/maps").read()
    assert T._C.preferred_precision() == T._C.Precision.Bf16
    with pytest.raises(RuntimeError):
        T._C.create_encoding(3, HASH_ENCODING_SMALL, T._C.Precision.Fp16)  # the other build's type


@pytest.mark.parametrize("d,enc", [(3, HASH_ENCODING), (3, HASH_ENCODING_SMALL), (2, HASH_ENCODING_SMALL),
                                   (3, dict(HASH_ENCODING, n_levels=8, n_features_per_level=4, log2_hashmap_size=14, interpolation="Smoothstep"))])
def test_grid_forward_bit_exact_and_backward(d, enc):
    C = tcnn()._C
    m = C.create_encoding(d, enc)
    g = O.grid_init(d, enc["n_levels"], enc["n_features_per_level"], enc["log2_hashmap_size"], enc["base_resolution"], enc["per_level_scale"],
                    O.GRID_HASH, O.INTERP_SMOOTHSTEP if enc.get("interpolation") == "Smoothstep" else O.INTERP_LINEAR)
    assert m.n_params() == g.n_params
    n = 4096
    pos = positions(n, d, seed=4)
    params = O.f2h(O.generate_random_uniform(O.pcg32(9), g.n_params, -1.0, 1.0))
    x, p = torch.from_numpy(pos).cuda(), h_t(params).requires_grad_(True)
    ctx, out = m.fwd(x, p)
    assert out.dtype == BF
    assert np.array_equal(m.grid_indices(x).cpu().numpy().reshape(n, g.n_levels, 1 << d), O.grid_indices(g, pos))
    assert np.array_equal(h_np(out), O.grid_forward(g, params, pos))
    dy = O.f2h(np.random.default_rng(1).standard_normal((n, out.shape[1])).astype(np.float32) * 0.1)
    _, grad = m.bwd(ctx, x, p, out, h_t(dy))
    ref = O.grid_backward(g, pos, dy)
    scale = np.abs(ref).max()
    assert np.abs(grad.float().cpu().numpy() - ref).max() <= 2.0 ** -6 * scale  # exact sums rounded once to bf16


@pytest.mark.parametrize("IN,W,OUT,H", [(32, 64, 4, 2), (32, 128, 16, 4), (64, 64, 16, 2), (32, 32, 3, 3)])
def test_network_forward_backward(IN, W, OUT, H):
    C = tcnn()._C
    net = dict(MLP_64x2, n_neurons=W, n_hidden_layers=H)
    m = C.create_network(IN, OUT, net)
    om = O.mlp_init(IN, W, OUT, H)
    ph = O.f2h(O.mlp_init_params(om, O.pcg32(5)))
    n = 2048
    rng = np.random.default_rng(3)
    xin = rng.random((n, IN), dtype=np.float32)
    x = torch.from_numpy(xin).cuda()
    p = h_t(ph).requires_grad_(True)
    ctx, out = m.fwd(x, p)
    enc = O.identity_forward(xin, IN)
    hid, ref = O.mlp_forward(om, ph, enc)
    assert np.percentile(rae(O.h2f(h_np(out)), O.h2f(ref)), 99) < 3e-2
    dy = O.f2h(rng.standard_normal((n, om.padded_out)).astype(np.float32))
    dx, grad = m.bwd(ctx, x, p, out, h_t(dy))
    gref, _ = O.mlp_backward(om, ph, enc, hid, ref, dy)
    got = grad.float().cpu().numpy()
    # sums of n random-signed terms cancel: entry-wise bars for the shallow shapes, the norm for the deep ones (every layer's
    # dL/dactivation is rounded to 8 significant bits and flips ReLU masks of borderline activations)
    assert np.linalg.norm(got - gref) < 2e-2 * np.linalg.norm(gref)
    if H <= 2:
        assert np.percentile(rae(got, gref), 99) < 3e-2


@pytest.mark.parametrize("width,hidden,out,log2_t,n", [(64, 2, 4, 15, 4096), (128, 4, 16, 17, 8192)])
def test_training_step_matches_oracle_and_converges(width, hidden, out, log2_t, n):
    """create_from_config -> training_step in bfloat16; the second case is the stress shape of BASELINE configs[4]
    (128-wide x 4 hidden layers, 16 outputs) at an oracle-sized table."""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=log2_t, per_level_scale=1.5, n_neurons=width, n_hidden_layers=hidden)
    tm = T.create_from_config(3, out, cfg)
    g = O.grid_init(3, 16, 2, log2_t, 16, 1.5)
    md = O.model_init(3, out, g, width, hidden, O.LOSS_RELATIVE_L2, O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=1e-6))
    init = tm.params_full_precision.cpu().numpy().copy()
    nm = md.mlp.n_params
    init[nm:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))
    assert tm.params.dtype == BF and np.array_equal(h_np(tm.params), O.f2h(init))
    st = O.TrainState(md, init)
    pos = positions(n, 3, seed=21)
    tgt = targets_for(pos, out)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()

    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-2 * abs(loss_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(pred_ref)), 99) < 3e-2
    _, g_loss = O.loss(md.loss_type, h_np(ctx.output), tgt, out)
    assert np.array_equal(h_np(ctx.dL_doutput), g_loss)
    gq, gref = tm.param_gradients.float().cpu().numpy(), O.h2f(st.grads)
    assert np.isfinite(gq).all()
    assert np.percentile(rae(gq[:nm], gref[:nm]), 99) < 5e-2
    assert np.linalg.norm(gq[nm:] - gref[nm:]) < 5e-2 * np.linalg.norm(gref[nm:])

    losses = [tm.loss(tm.training_step(x, t)) for _ in range(30)]
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses
    w = tm.params_full_precision.cpu().numpy()
    assert np.array_equal(h_np(tm.params), O.f2h(w))  # Adam's 16-bit copy is the RNE bfloat16 of its fp32 master weights
    a, b = tm.inference(x), tm.inference(x)
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_torch_modules_and_snapshot_in_bf16():
    import msgpack
    T = tcnn()
    net = T.NetworkWithInputEncoding(3, 4, HASH_ENCODING_SMALL, MLP_64x2).cuda()
    assert net.params.dtype == torch.float32  # torch owns fp32 parameters, cast per call (modules.py:230)
    x = torch.rand(1000, 3, device="cuda")
    y = net(x)
    assert y.dtype == BF and y.shape == (1000, 4)
    y.float().square().mean().backward()
    assert net.params.grad is not None and torch.isfinite(net.params.grad).all() and net.params.grad.abs().max() > 0
    tm = T.create_from_config(3, 4, config_hash(log2_hashmap_size=12, per_level_scale=1.5))
    doc = msgpack.unpackb(tm.serialize(), raw=False)
    assert doc["params_type"] == "__nv_bfloat16" and len(doc["params_binary"]) == 2 * tm.n_params
    other = T.create_from_config(3, 4, config_hash(log2_hashmap_size=12, per_level_scale=1.5), seed=5)
    other.deserialize(tm.serialize())
    assert torch.equal(other.params.view(torch.int16), tm.params.view(torch.int16))


def test_stress_shape_training_step_at_its_stated_size():
    """BASELINE.json configs[4] AT ITS STATED SIZE: HashGrid(L=16, F=2, T=2^22, per_level_scale 1.5) + FullyFusedMLP 128 x 4,
    3-D -> 16, N = 2^18, bfloat16 -- one training step against the oracle's bfloat16 mode.  At this size the gather plan carries its
    L2-miss term (make_forward_plan), the 128-wide single-kernel training pass walks 8192 tiles, the bucketed backward holds 4096
    buckets per level and Adam streams its 2.7 GB of state (adam_streams_its_state): none of which the small cases reach.
      * encoded features (the module path on the same table): bit-exact;
      * prediction RAE p99 <= 3e-2, loss 2e-2 (bf16: 8 significant bits); loss gradient bit-exact on the GPU's own prediction;
      * network gradients: relative L2 <= 3e-2; grid gradients per level: relative L2 <= 5e-2 (bf16 records, exact sums);
      * one Adam step from the GPU's own gradients: moments and step counters bit-exact, master weights within 4 ulp,
        bf16 weights = RNE of the master weights."""
    import msgpack
    T = tcnn()
    n, out, log2_t = 1 << 18, 16, 22
    cfg = config_hash(log2_hashmap_size=log2_t, per_level_scale=1.5, n_neurons=128, n_hidden_layers=4)
    tm = T.create_from_config(3, out, cfg)
    g = O.grid_init(3, 16, 2, log2_t, 16, 1.5)
    md = O.model_init(3, out, g, 128, 4, O.LOSS_RELATIVE_L2, O.adam_defaults(learning_rate=1e-2, beta1=0.9, beta2=0.99, epsilon=1e-15, l2_reg=1e-6))
    assert tm.n_params == md.n_params
    init = tm.params_full_precision.cpu().numpy().copy()
    nm = md.mlp.n_params
    init[nm:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))
    st = O.TrainState(md, init)
    pos = positions(n, 3, seed=91)
    tgt = targets_for(pos, out)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()

    # the gather alone, through the encoding module on the trainer's table
    e = T._C.create_encoding(3, cfg["encoding"])
    _, enc = e.fwd(x, tm.params[nm:].contiguous())
    want = O.grid_forward(g, O.f2h(init[nm:]), pos)
    assert np.array_equal(h_np(enc), want)
    del enc, want

    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-2 * abs(loss_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(pred_ref)), 99) < 3e-2
    _, g_loss = O.loss(md.loss_type, h_np(ctx.output), tgt, out)
    assert np.array_equal(h_np(ctx.dL_doutput), g_loss)
    gq, gref = tm.param_gradients.float().cpu().numpy(), O.h2f(st.grads)
    assert np.isfinite(gq).all()
    rel = lambda a, b: np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b.astype(np.float64)), 1e-30)  # noqa: E731
    assert rel(gq[:nm], gref[:nm]) < 3e-2, rel(gq[:nm], gref[:nm])
    off = np.asarray(g.offsets[:17], np.int64) * 2
    for l in range(16):
        a, b = gq[nm + off[l]:nm + off[l + 1]], gref[nm + off[l]:nm + off[l + 1]]
        assert rel(a, b) < 5e-2, (l, rel(a, b))
        # Untouched entries stay exactly zero on both sides (the optimizer skips them, adam.h:79-82).  Touched ones: the owner pass sums bfloat16
        # records in fixed point at an exponent chosen per slice from the level's own |dL/dy| (OwnerScale, grid_backward_plan.h) -- 2^-28 on the
        # hashed levels of this step, so a sum survives unless it is below 2^-29 = 2.5e-5 of the level's rms (round 5: 2^-24 for every level,
        # i.e. everything below 8e-4 of the rms vanished, and the test accepted zeros up to 2 % of it).  Tables of 2^19 entries and more have
        # one owner per slice: a zero where the oracle holds more than 1e-4 of the rms is a sample whose dL/dy differs between the two sides
        # (a ReLU mask that flips on a pre-activation next to zero) -- fewer than one entry in 10^5.  The smaller tables are split over sample
        # chunks whose partial sums (~45 records each) meet in bfloat16 atomics: two of them can cancel to an exact zero where the exact sum
        # is a percent of a typical entry -- the 8-bit mantissa, not the fixed point.
        rms = float(np.sqrt(np.mean(b.astype(np.float64) ** 2)))
        assert np.mean((a != 0) & (b == 0)) < 1e-4 and np.mean((a == 0) != (b == 0)) < 1.5e-3, l
        floor = (1e-4 if off[l + 1] - off[l] >= 2 * (1 << 19) else 2e-2) * rms
        assert np.mean((a == 0) & (np.abs(b) > floor)) < 1e-5, (l, np.mean((a == 0) & (np.abs(b) > floor)))

    # one optimizer step (the streaming Adam variant) from the GPU's own gradients
    ref = O.TrainState(md, init)
    grads_h = h_np(tm.param_gradients)
    O.adam_step(md.adam, nm, 128.0, 1, ref.w32, ref.w16, grads_h, ref.m1, ref.m2, ref.steps)
    tm.optimizer_step()
    w = tm.params_full_precision.cpu().numpy()
    scale = np.maximum(np.maximum(np.abs(init), np.abs(ref.w32)), np.float32(0.03))
    assert bool((np.abs(w - ref.w32) <= 4 * np.spacing(scale)).all())
    assert np.array_equal(h_np(tm.params), O.f2h(w))
    m1, m2, steps, _ = tm.optimizer_state()
    assert np.array_equal(m1.cpu().numpy(), ref.m1) and np.array_equal(m2.cpu().numpy(), ref.m2)
    s = steps.cpu().numpy().view(np.uint32)
    deficits = tm.optimizer_state()[3]
    assert np.array_equal((np.uint32(1) - s) if deficits else s, ref.steps)


# ---------------------------------------------------------------------------------------------------------------------
# Grid backward and second order across bfloat16's range, in the bucketed mode (the library's default, set explicitly).  Bars as in
# tests/test_emu_bf16.py (helpers: tests/bf16_bars.py), per level from the plan rule the library documents (grid_backward_plan.h,
# make_backward_plan), restated here from the test's own sizes:
#   * a slice is the largest power-of-two number of entries whose 64-bit-per-value table fits the default 128 KiB of LDS;
#   * a level's samples are split into chunks only when a slice would see more than 65536 records (n * 2^D / slices):
#     then ceil(records per slice / 32768) of them at most;
#   * one owner per (slice, chunk) sums its records exactly in fixed point at the level's exponent k and rounds ONCE; the chunks
#     of a slice meet in packed bfloat16 atomics (one rounding each); records that overflow their queue, beyond 2^18 of them per
#     call, are added by global atomics (one rounding per record).
#   |got - ref| <= c * 2^-9 * (absacc + floor) + floor, c = 2 per rounding, floor = N_e * 2^-(k+1).
# ---------------------------------------------------------------------------------------------------------------------
from bf16_bars import ONE_ROUNDING, TINY, absf, level_k, max_abs_per_level, record_counts, second_order_magnitudes, spread  # noqa: E402

SLICE_BYTES = 128 * 1024


class bucketed_mode:
    """the bucketed backward with the given owner form, restored on the way out"""

    def __init__(self, owner=0):
        self.owner = owner

    def __enter__(self):
        C = tcnn()._C
        self.saved = (C.get_grid_backward_mode(), C.get_grid_owner_mode())
        C.set_grid_backward_mode(3)
        C.set_grid_owner_mode(self.owner)

    def __exit__(self, *exc):
        C = tcnn()._C
        C.set_grid_backward_mode(self.saved[0])
        C.set_grid_owner_mode(self.saved[1])


def plan_rule(og, n):
    """(slices, most chunks) per level by the rule above"""
    F = og.n_features_per_level
    corners = 1 if og.interpolation == O.INTERP_NEAREST else 1 << og.n_dims
    per_slice = 1
    while 2 * per_slice * F * 8 <= SLICE_BYTES:
        per_slice *= 2
    slices, chunks = [], []
    for l in range(og.n_levels):
        entries = og.offsets[l + 1] - og.offsets[l]
        nb = -(-entries // per_slice)
        records = n * corners // nb
        slices.append(nb)
        chunks.append(1 if records <= 65536 else -(-records // 32768))
    return np.array(slices), np.array(chunks)


def bucketed_bar(og, pos, per_sample, absacc, roundings_per_level, atomics_per_record=False):
    """(bar, floor).  k per level: the rule at the level's owners; where the chunk count is only bounded (1 ... most), the coarser k."""
    slices, chunks = plan_rule(og, pos.shape[0])
    counts = record_counts(og, pos)
    ks = [min(level_k(per_sample[:, l], int(slices[l])), level_k(per_sample[:, l], int(slices[l] * chunks[l]))) for l in range(og.n_levels)]
    floor = counts * spread(og, [2.0 ** -(k + 1) for k in ks])
    c = spread(og, np.asarray(roundings_per_level, np.float64)) + (counts if atomics_per_record else 0.0)
    return c * ONE_ROUNDING * (absacc + floor) + floor + TINY, floor, ks


def slices_that_must_go_wide(og, n, absacc, ks):
    """The packed owner (even F) keeps a slice only if the magnitudes of its records sum to less than 0.9375 * 2^(31-k) per feature
    (OwnerScale::safe_abs_sum); otherwise it redoes the slice with 64 bits per value at the same k.  Counted from the oracle's
    accumulated magnitudes: sole-owner slices whose sum for some feature is beyond 2^(31-k) -- clear of the bound's own rounding."""
    F = og.n_features_per_level
    if F % 2:
        return 0
    per_slice = 1
    while 2 * per_slice * F * 8 <= SLICE_BYTES:
        per_slice *= 2
    slices, chunks = plan_rule(og, n)
    count = 0
    for l in range(og.n_levels):
        if chunks[l] != 1:
            continue
        a = absacc[og.offsets[l] * F:og.offsets[l + 1] * F].reshape(-1, F)
        for b in range(int(slices[l])):
            count += bool((a[b * per_slice:(b + 1) * per_slice].sum(axis=0) > 2.0 ** (31 - ks[l])).any())
    return count


def bits_of(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16).copy()


GRID_TYPES = {"Dense": O.GRID_DENSE, "Tiled": O.GRID_TILED, "Hash": O.GRID_HASH}
BACKWARD_SHAPES = [(2, "Dense", 1), (2, "Dense", 4), (4, "Dense", 8), (2, "Tiled", 8), (4, "Tiled", 4), (4, "Tiled", 1), (3, "Hash", 2)]


@pytest.mark.parametrize("magnitude", [2.0 ** -100, 2.0 ** -40, 3e-3, 2.0, 300.0, 2.0 ** 12, 2.0 ** 20, "mixed"], ids=str)
@pytest.mark.parametrize("d,gtype,F", BACKWARD_SHAPES)
def test_grid_backward_across_the_range(d, gtype, F, magnitude):
    """Dense, Tiled and hashed tables, F = 1, 4, 8, D = 2 ... 4: dL/dy ~ N(0, 1) times 2^-100 ... 2^20 and a mixed batch (1 % of the
    samples at 2^10, the rest at 2^-20).  n * 2^D <= 65536: every slice has ONE owner, so c = 2 (one rounding) whatever N_e, the three
    owner forms give the same BITS, and a zero is legitimate only where the exact fixed-point sum is zero: |ref| inside the floor."""
    C = tcnn()._C
    L = 5 if d == 2 else 3
    enc = dict(otype="Grid", type=gtype, n_levels=L, n_features_per_level=F, log2_hashmap_size=14, base_resolution=4, per_level_scale=1.6)
    m = C.create_encoding(d, enc)
    og = O.grid_init(d, L, F, 14, 4, 1.6, GRID_TYPES[gtype], O.INTERP_LINEAR)
    assert m.n_params() == og.n_params
    n = 4096
    assert n * (1 << d) <= 65536 and np.all(plan_rule(og, n)[1] == 1)
    pos = positions(n, d, seed=7)
    z = np.random.default_rng(2).standard_normal((n, L * F))
    factor = np.where(np.arange(n) % 100 == 0, 2.0 ** 10, 2.0 ** -20)[:, None] if magnitude == "mixed" else magnitude
    dy = np.zeros((n, m.n_output_dims()), np.uint16)
    dy[:, :L * F] = O.f2h((z * factor).astype(np.float32))
    params = O.f2h(O.generate_random_uniform(O.pcg32(9), og.n_params, -1.0, 1.0))
    x, p = torch.from_numpy(pos).cuda(), h_t(params).requires_grad_(True)
    ctx, out = m.fwd(x, p)
    got, wide = [], []
    for owner in (0, 1, 2):
        with bucketed_mode(owner):
            before = C.grid_owner_wide_slices()
            _, grad = m.bwd(ctx, x, p, out, h_t(dy))
            torch.cuda.synchronize()
            wide.append(C.grid_owner_wide_slices() - before)
        got.append(bits_of(grad))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    gotf = O.h2f(got[0]).astype(np.float64)
    ref = O.grid_backward(og, pos, dy[:, :L * F])
    absacc = O.grid_backward(og, pos, absf(dy[:, :L * F]))
    bar, floor, ks = bucketed_bar(og, pos, max_abs_per_level(dy[:, :L * F], L, F), absacc, [1] * L)
    err = np.abs(gotf - ref)
    must = slices_that_must_go_wide(og, n, absacc, ks)
    print("worst |err| / bar:", float((err / bar).max()), "k:", ks, "wide slices:", wide[0], "of which the bound demands:", must)
    assert np.isfinite(gotf).all() and np.all(err <= bar)
    assert not np.any((gotf == 0) & (np.abs(ref) > floor + TINY))
    # the 64-bit redo at the level's own k really runs on the hardware where the bound says it must (2^12 and up, the mixed batch: k is at
    # its coarsest and still the slices' sums pass 2^(31-k)) -- and gave the bits of the other two forms above
    assert wide[0] >= must and (must > 0 or F % 2 or magnitude in (2.0 ** -100, 2.0 ** -40, 3e-3, 2.0))


def test_grid_backward_accumulates():
    """GradientMode::Accumulate in bfloat16 (mirrors test_gradient_modes_and_data_parallel_linearity): a second identical step on top of
    the first.  n * 2^D <= 65536: every grid slice has one owner, which adds its exactly summed, once-rounded result -- the same bits as
    the first step's -- to what is there: 2 x full, exact in any binary format.  The network's weight gradients are fp32 partial sums
    rounded once and added to the old value: one rounding of 2 x full, and one of full should the partial sums be grouped differently."""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=15, per_level_scale=1.5)
    tm = T.create_from_config(3, 4, cfg)
    n = 4096
    pos = positions(n, 3, seed=3)
    tgt = targets_for(pos, 4)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    w = tm.params_full_precision.clone()
    nm = tm.n_mlp_params
    w[nm:] *= 1.0e3
    tm.set_params_full_precision(w)
    with bucketed_mode():
        tm.training_step(x, t, run_optimizer=False, want_context=False)
        full = tm.param_gradients.float().cpu().numpy().astype(np.float64)
        tm.training_step(x, t, run_optimizer=False, gradient_mode=T._C.GradientMode.Accumulate, want_context=False)
        twice = tm.param_gradients.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(twice).all() and np.abs(full[nm:]).max() > 0
    assert np.array_equal(twice[nm:], 2 * full[nm:])
    assert np.all(np.abs(twice[:nm] - 2 * full[:nm]) <= 3 * ONE_ROUNDING * np.abs(full[:nm]) + TINY)


@pytest.mark.parametrize("clustered", [False, True])
def test_bucketed_grid_backward_full_size(clustered):
    """test_bucketed_grid_backward_full_size in bfloat16 (N = 2^18, T = 2^19).  Uniform inputs: nothing overflows beyond the inline
    list, every (slice, chunk) owner is exact: c = 2 x (1 + chunks where a level is chunked), and the three owner forms agree bit for
    bit on the levels with one owner per slice.  Clustered inputs (3/4 of the batch inside a 1 % cube): the slices under the cluster
    that fail the packed owner's int32 bound are redone with 64 bits per value at the level's data-dependent k, queues overflow and their records go through global atomics -- one more rounding per record of the entry, at the worst."""
    C = tcnn()._C
    enc = dict(HASH_ENCODING)
    m = C.create_encoding(3, enc)
    og = O.grid_init(3, enc["n_levels"], enc["n_features_per_level"], enc["log2_hashmap_size"], enc["base_resolution"], enc["per_level_scale"])
    L, F = og.n_levels, og.n_features_per_level
    n = 1 << 18
    pos = positions(n, 3, seed=21)
    if clustered:
        pos[n // 4:] = pos[:3 * n // 4] * 0.01 + 0.37
    rng = np.random.default_rng(3)
    dy = O.f2h((rng.standard_normal((n, m.n_output_dims())) * 0.02).astype(np.float32))
    x = torch.from_numpy(pos).cuda()
    p = torch.zeros(og.n_params, dtype=BF, device="cuda").requires_grad_(True)
    ctx, y = m.fwd(x, p)
    got = []
    wide = []
    for owner in (0, 1, 2):
        with bucketed_mode(owner):
            before = C.grid_owner_wide_slices()
            _, dp = m.bwd(ctx, x, p, y, h_t(dy))
            torch.cuda.synchronize()
            wide.append(C.grid_owner_wide_slices() - before)
        got.append(bits_of(dp))
    slices, chunks = plan_rule(og, n)
    ref = O.grid_backward(og, pos, dy[:, :L * F])
    absacc = O.grid_backward(og, pos, absf(dy[:, :L * F]))
    bar, floor, ks = bucketed_bar(og, pos, max_abs_per_level(dy[:, :L * F], L, F), absacc, [1 + (c if c > 1 else 0) for c in chunks], atomics_per_record=clustered)
    # (the hash spreads the cluster's records over a level's whole table, and a queue holds no more than its capacity -- the rest of a
    # clustered slice's records travel through the overflow list, past the owner's bound: the count of slices that must go wide is
    # known for uniform inputs only; test_grid_backward_across_the_range is where the redo is certain to run)
    if not clustered:
        assert wide[0] >= slices_that_must_go_wide(og, n, absacc, ks)
    for o in range(3):
        gotf = O.h2f(got[o]).astype(np.float64)
        err = np.abs(gotf - ref)
        print("owner form", o, "worst |err| / bar:", float((err / bar).max()), "wide slices:", wide[o])
        assert np.isfinite(gotf).all() and np.all(err <= bar)
    if not clustered:
        n_sole = 0
        for l in range(L):
            if chunks[l] == 1:
                lo, hi = og.offsets[l] * F, og.offsets[l + 1] * F
                assert np.array_equal(got[0][lo:hi], got[1][lo:hi]) and np.array_equal(got[0][lo:hi], got[2][lo:hi]), l
                assert not np.any((O.h2f(got[0][lo:hi]) == 0) & (np.abs(ref[lo:hi]) > floor[lo:hi] + TINY)), l
                n_sole += 1
        assert n_sole >= 8


@pytest.mark.parametrize("ddx_scale", [1.0, 1e-4])
@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
def test_grid_second_order_with_small_and_unit_ddx(interp, ddx_scale):
    """backward_backward_input in bfloat16 (mirrors test_grid_second_order_through_c_abi_and_double_backward of the fp16 suite) with
    ddx ~ N(0, 1) and N(0, 1) * 1e-4 (eikonal-sized).  The level sum that picks the owners' exponent is taken from the records the
    scatter emits (|dy| * sum over the corners of |weight|): with k from |dL/dy| alone the 1e-4 case lost every record below 2^-21.
    One owner per slice (n * 2^D <= 65536); five roundings of magnitudes bounded by absacc (tests/test_emu_bf16.py
    test_grid_second_order): c = 10.  A zero is legitimate where the kernel's exact sum is inside the floor: the oracle's then lies
    within the floor and the four roundings that separate the two sides' records.  d(dL_dx)/d(dL_dy) bit-exact."""
    C = tcnn()._C
    enc = dict(HASH_ENCODING_SMALL, interpolation=interp)
    d = 3
    m = C.create_encoding(d, enc)
    og = O.grid_init(d, enc["n_levels"], enc["n_features_per_level"], enc["log2_hashmap_size"], enc["base_resolution"], enc["per_level_scale"],
                     O.GRID_HASH, O.INTERP_SMOOTHSTEP if interp == "Smoothstep" else O.INTERP_LINEAR)
    n = 2048
    assert np.all(plan_rule(og, n)[1] == 1)
    pos = positions(n, d, seed=31)
    rng = np.random.default_rng(5)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    K = m.n_output_dims()
    dy = O.f2h(rng.standard_normal((n, K)).astype(np.float32))
    ddx = (rng.standard_normal((n, d)) * ddx_scale).astype(np.float32)
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    with bucketed_mode():
        d_dy, d_p, d_x = m.bwd_bwd_input(ctx, x, p, torch.from_numpy(ddx).cuda(), h_t(dy).requires_grad_(True))
        torch.cuda.synchronize()
    KF = og.n_levels * og.n_features_per_level
    _, dydx = O.grid_forward(og, params, pos, want_dy_dx=True)
    gp_ref, dLddy_ref, dx_ref = O.grid_backward_backward_input(og, params, pos, ddx, dy[:, :KF], dy_dx=dydx)
    assert np.array_equal(h_np(d_dy)[:, :KF], dLddy_ref[:, :KF])
    assert np.allclose(d_x.cpu().numpy(), dx_ref, rtol=1e-3, atol=1e-4 * max(ddx_scale, np.abs(dx_ref).max()))
    absacc, per_sample = second_order_magnitudes(og, pos, ddx, dy[:, :KF])
    bar, floor, ks = bucketed_bar(og, pos, per_sample, absacc * (1 + 1e-5), [5] * og.n_levels)
    got = d_p.float().cpu().numpy().astype(np.float64)
    err = np.abs(got - gp_ref)
    print("worst |err| / bar:", float((err / bar).max()))
    assert np.isfinite(got).all() and np.all(err <= bar)
    assert np.abs(gp_ref).max() > 0 and not np.any((got == 0) & (np.abs(gp_ref) > floor + 4 * ONE_ROUNDING * absacc + TINY))


@pytest.mark.parametrize("act,out_act", [("LeakyReLU", "None"), ("Exponential", "Sigmoid"), ("Sigmoid", "Exponential"), ("Squareplus", "Tanh"),
                                         ("Softplus", "Softplus"), ("Tanh", "Squareplus"), ("None", "ReLU")])
def test_network_activations(act, out_act):
    """test_network_activations of the fp16 suite in bfloat16, with this file's bars for the oracle comparisons (outputs RAE p99 < 3e-2,
    gradients relative L2 < 2e-2 and, two hidden layers, RAE p99 < 3e-2).  Fused training kernel against forward() + backward(): the
    fp16 suite's bars in units of the type's spacing, which is 8 x coarser here (rtol 4e-3 -> 3.2e-2, 2e-3 -> 1.6e-2, 2^-10 -> 2^-7)."""
    C = tcnn()._C
    IN, W, OUT, H = 32, 64, 4, 2
    m = C.create_network(IN, OUT, dict(MLP_64x2, activation=act, output_activation=out_act))
    om = O.mlp_init(IN, W, OUT, H, activation=O.ACTIVATION_NAMES.index(act), output_activation=O.ACTIVATION_NAMES.index(out_act))
    hp = m.hyperparams()["network"]
    assert hp["output_activation"] == out_act and hp["activation"] == act
    ph = O.f2h(O.mlp_init_params(om, O.pcg32(3)) * 0.5)
    n = 1024
    rng = np.random.default_rng(13)
    xin = rng.random((n, IN), dtype=np.float32) * 0.5
    x = torch.from_numpy(xin).cuda().requires_grad_(True)
    p = h_t(ph).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    torch.cuda.synchronize()
    enc = O.identity_forward(xin, IN)
    hid_ref, out_ref = O.mlp_forward(om, ph, enc)
    assert np.percentile(rae(O.h2f(h_np(y))[:, :OUT], O.h2f(out_ref)[:, :OUT]), 99) < 3e-2
    dy = np.zeros((n, 16), np.float32)
    dy[:, :OUT] = rng.standard_normal((n, OUT)).astype(np.float32) * 0.05
    dyh = O.f2h(dy)
    dx, dp = m.bwd(ctx, x, p, y, h_t(dyh))
    torch.cuda.synchronize()
    gref, dref = O.mlp_backward(om, ph, enc, hid_ref, out_ref, dyh)
    gq = dp.float().cpu().numpy()
    assert np.linalg.norm(gq - gref) < 2e-2 * np.linalg.norm(gref) and np.percentile(rae(gq, gref), 99) < 3e-2
    dx_ref = O.h2f(dref)[:, :IN].astype(np.float64)
    assert np.linalg.norm(dx.float().cpu().numpy() - dx_ref) < 2e-2 * np.linalg.norm(dx_ref)

    T = tcnn()
    cfg = config_hash(log2_hashmap_size=14)
    cfg["network"] = dict(cfg["network"], activation=act, output_activation=out_act)
    tm = T.create_from_config(3, 4, cfg, seed=3)
    w = tm.params_full_precision.clone()
    w[tm.n_mlp_params:] *= 1.0e3
    tm.set_params_full_precision(w)
    pos = positions(2048, 3, seed=4)
    xx, tt = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()
    ctx_f = tm.training_step(xx, tt, run_optimizer=False)
    g_fused, loss_fused = tm.param_gradients.clone(), tm.loss(ctx_f)
    c2 = tm.forward(xx, tt)
    tm.backward(c2, xx)
    g_pair, nm = tm.param_gradients, tm.n_mlp_params
    grid_pair, grid_fused = g_pair[nm:].float(), g_fused[nm:].float()
    assert (grid_pair != grid_fused).float().mean() < 0.02
    assert torch.allclose(grid_pair, grid_fused, rtol=3.2e-2, atol=1.6e-2 * float(grid_fused.abs().max()))
    assert (g_pair[:nm] != g_fused[:nm]).float().mean() < 0.05
    assert torch.allclose(g_pair[:nm].float(), g_fused[:nm].float(), rtol=1.6e-2, atol=1e-3 * float(g_fused[:nm].float().abs().max()) * 2.0 ** -7 + 1e-7)
    assert abs(tm.loss(c2) - loss_fused) <= 1e-5 * abs(loss_fused) + 1e-9
    assert torch.isfinite(g_fused.float()).all()


import exact_network_cases as E  # noqa: E402


@pytest.mark.parametrize("fused_passes", [True, False], ids=["single-kernel", "saved-activations"])
@pytest.mark.parametrize("case", E.BF16_CASES, ids=[c.name for c in E.BF16_CASES])
def test_exact_network_forward_backward(case, fused_passes):
    """tests/test_gpu_exact_network.py's module forward / backward of 64 x 2 and 128 x 4 with bfloat16 as the 16-bit type: inputs on which every
    fp32 sum is exact in any order (C1 and C2 re-audited for the type by tests/test_exact_network_reference.py), so prediction, dL/dinput
    and the parameter gradients equal the float64 restatement rounded to bfloat16 in every bit."""
    C = tcnn()._C
    data = E.generate(case, E.BF16)
    res = E.restate(case, data, E.BF16)
    to_t = lambda v: torch.from_numpy(E.to_bits(v, E.BF16).view(np.int16)).view(BF).cuda()  # noqa: E731
    m = C.create_network(case.IN, case.OUT, case.network())
    x = torch.from_numpy(data.x.astype(np.float32)).cuda().requires_grad_(True)
    p = to_t(data.params).requires_grad_(True)
    C.set_fused_network_passes(fused_passes)
    try:
        ctx, y = m.fwd(x, p)
        dx, dp = m.bwd(ctx, x, p, y, to_t(data.dy))
        torch.cuda.synchronize()
    finally:
        C.set_fused_network_passes(True)
    report = [E.mismatch("prediction", h_np(y), E.to_bits(res.out, E.BF16)),
              E.mismatch("dL/dinput", dx.cpu().numpy().view(np.uint32), res.dinput.astype(np.float32).view(np.uint32)),
              E.mismatch("parameter gradients", h_np(dp), E.to_bits(res.grads, E.BF16))]
    assert not any(report), "\n".join(r for r in report if r)

"""Parity of the HIP path (through the C ABI / the tinycudann modules) against the CPU oracle, on a real
MI355X.  Bars:
  * hash-grid indices and the offset table: bit-exact;
  * encoded features: bit-exact (the kernel reproduces the reference's fp16 fma chain, grid.h:144-163);
  * loss gradients: bit-exact given the same fp16 prediction (IEEE fp32 division on both sides);
  * MLP outputs / gradients: relative absolute error (tests/test_common.h:62-117) p99 <= 1e-2 is the
    reference's own bar; we require p99 <= 3e-3 against the fp32-accumulate oracle (fp16 tolerance: MFMA
    and the oracle sum the same fp16 products in a different order, results are rounded to fp16);
  * grid gradients: |gpu - exact| <= 2^-9 * sum|contributions| + 2e-3 (fp16 atomics round at every add).
"""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import ADAM_HASH, HASH_ENCODING, HASH_ENCODING_SMALL, MLP_64x2, ROOT, config_hash
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


def oracle_grid(enc, n_dims):
    default_type = {"DenseGrid": "Dense", "TiledGrid": "Tiled"}.get(enc.get("otype", "Grid"), "Hash")  # grid.h:1729-1731
    return O.grid_init(n_dims, enc.get("n_levels", 16), enc.get("n_features_per_level", 2), enc.get("log2_hashmap_size", 19),
                       enc.get("base_resolution", 16), enc.get("per_level_scale", 2.0),
                       {"Hash": O.GRID_HASH, "Dense": O.GRID_DENSE, "Tiled": O.GRID_TILED}[enc.get("type", default_type)],
                       {"Nearest": O.INTERP_NEAREST, "Linear": O.INTERP_LINEAR, "Smoothstep": O.INTERP_SMOOTHSTEP}[enc.get("interpolation", "Linear")])


def positions(n, d, seed=1337):
    rng = O.pcg32(seed)
    return O.generate_random_uniform(rng, n * d, 0.0, 1.0).reshape(n, d)


def test_native_library_is_loaded():
    tcnn()
    maps = open("/proc/self/maps").read()
    assert "libtcnn_hip.so" in maps, "the HIP extension is not mapped into this process"
    assert torch.cuda.is_available() and "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


ENCODINGS = [
    (3, HASH_ENCODING),
    (3, HASH_ENCODING_SMALL),
    (2, HASH_ENCODING_SMALL),
    (3, dict(HASH_ENCODING, n_levels=8, n_features_per_level=4, log2_hashmap_size=14, interpolation="Smoothstep")),
    (3, dict(HASH_ENCODING, n_levels=6, n_features_per_level=1, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.6)),
    (4, dict(HASH_ENCODING, n_levels=4, n_features_per_level=8, log2_hashmap_size=10, base_resolution=4, per_level_scale=1.5)),
    (3, {"otype": "DenseGrid", "n_levels": 5, "base_resolution": 4, "per_level_scale": 1.4}),
    (2, {"otype": "TiledGrid", "n_levels": 6, "base_resolution": 8, "per_level_scale": 2.0, "interpolation": "Nearest"}),
]


@pytest.mark.parametrize("d,enc", ENCODINGS)
def test_grid_indices_and_forward_bit_exact(d, enc):
    C = tcnn()._C
    m = C.create_encoding(d, enc)
    og = oracle_grid(enc, d)
    assert m.n_params() == og.n_params
    n = 2048
    pos = positions(n, d)
    pos[0] = 0.0
    pos[1] = 1.0  # cell coordinate == resolution -> wrap-around (common_device.h:1002-1007)
    x = torch.from_numpy(pos).cuda()
    assert np.array_equal(m.grid_indices(x).cpu().numpy().view(np.uint32), O.grid_indices(og, pos))
    rng = np.random.default_rng(0)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    _, y = m.fwd(x, h_t(params))
    torch.cuda.synchronize()
    assert y.shape == (n, m.n_output_dims())
    assert np.array_equal(h_np(y), O.grid_forward(og, params, pos))


@pytest.mark.parametrize("d,enc", ENCODINGS)
def test_grid_backward_and_input_gradient(d, enc):
    C = tcnn()._C
    m = C.create_encoding(d, enc)
    og = oracle_grid(enc, d)
    n = 4096
    pos = positions(n, d, seed=7)
    rng = np.random.default_rng(1)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    dy = O.f2h(rng.standard_normal((n, m.n_output_dims())).astype(np.float32))
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    ref = O.grid_backward(og, pos, dy)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))))
    default_mode = C.get_grid_backward_mode()
    try:
        for mode in (0, 2, 3, 1):  # fp32 LDS slices, the reference's global atomics (A/B), bucket-once, packed-fp16 LDS slices
            if mode == 2 and enc.get("n_features_per_level", 2) == 1:
                continue
            C.set_grid_backward_mode(mode)
            dx, dp = m.bwd(ctx, x, p, y, h_t(dy))
            torch.cuda.synchronize()
            got = dp.float().cpu().numpy().astype(np.float64)
            # modes 1 and 2 add up to hundreds of terms per entry in fp16, in hardware order: 2^-8 of the magnitude
            assert np.all(np.abs(got - ref) <= absacc * 2.0 ** (-9 if mode == 0 else -8) + 2e-3), f"grid backward mode {mode}"
    finally:
        C.set_grid_backward_mode(default_mode)
    if enc.get("interpolation", "Linear") != "Nearest":
        _, dy_dx = O.grid_forward(og, params, pos, want_dy_dx=True)
        dref = O.grid_backward_input(og, dy, dy_dx)
        assert np.allclose(dx.cpu().numpy(), dref, rtol=1e-4, atol=1e-3 * np.abs(dref).max())


@pytest.mark.parametrize("d,enc", [(3, dict(HASH_ENCODING, log2_hashmap_size=15, n_levels=8)),
                                   (2, {"otype": "DenseGrid", "n_levels": 4, "base_resolution": 8, "per_level_scale": 2.0, "interpolation": "Smoothstep"}),
                                   (3, dict(HASH_ENCODING, log2_hashmap_size=12, n_levels=6, n_features_per_level=1))])  # F == 1: packed atomic on the aligned pair
def test_grid_stochastic_interpolation(d, enc):
    """stochastic_interpolation (grid.h:284-299): the backward pass sends the whole gradient of (sample, level) to one corner
    picked by random_val(1337, i + level * n); the forward pass is the ordinary interpolation.  Same corner as the oracle
    for every sample (sums of up to a few hundred fp16 terms per entry), and the scatter conserves the gradient mass."""
    C = tcnn()._C
    enc = dict(enc, stochastic_interpolation=True)
    m = C.create_encoding(d, enc)
    og = oracle_grid(enc, d)
    n = 8192
    pos = positions(n, d, seed=9)
    rng = np.random.default_rng(2)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    dy = O.f2h(rng.standard_normal((n, m.n_output_dims())).astype(np.float32))
    x = torch.from_numpy(pos).cuda()
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    assert np.array_equal(h_np(y), O.grid_forward(og, params, pos))
    _, dp = m.bwd(ctx, x, p, y, h_t(dy))
    got = dp.float().cpu().numpy().astype(np.float64)
    ref = O.grid_backward(og, pos, dy, stochastic_interpolation=True)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))), stochastic_interpolation=True)
    assert np.all(np.abs(got - ref) <= absacc * 2.0 ** -8 + 2e-3)
    assert not np.allclose(ref, O.grid_backward(og, pos, dy), atol=1e-2)  # not the interpolating scatter
    F = enc.get("n_features_per_level", 2)
    for level in range(og.n_levels):
        lo, hi = og.offsets[level] * F, og.offsets[level + 1] * F
        want = O.h2f(dy)[:, level * F:(level + 1) * F].astype(np.float64).sum()
        assert abs(got[lo:hi].sum() - want) <= 1e-2 * np.abs(O.h2f(dy)[:, level * F:(level + 1) * F]).sum() * 2.0 ** -6 + 0.5


def test_grid_forward_full_size_bit_exact_and_checksum():
    """BASELINE size: N = 2^18, T = 2^19.  Bit-exact against the oracle, plus the size-independent scatter
    property sum_entries grad[level, f] == sum_i dL_dy[i, level, f] (interpolation weights sum to one)."""
    C = tcnn()._C
    m = C.create_encoding(3, HASH_ENCODING)
    og = oracle_grid(HASH_ENCODING, 3)
    n = 1 << 18
    pos = positions(n, 3)
    rng = np.random.default_rng(2)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    x = torch.from_numpy(pos).cuda()
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    assert np.array_equal(h_np(y), O.grid_forward(og, params, pos))
    dy = (torch.randn((n, 32), device="cuda") * 0.01).half()
    _, dp = m.bwd(ctx, x, p, y, dy)
    torch.cuda.synchronize()
    got = dp.float().view(-1, 2)
    sums = torch.stack([got[og.offsets[l]:og.offsets[l + 1]].double().sum(0) for l in range(16)]).cpu().numpy()  # [L][F]
    ref = dy.double().sum(0).view(16, 2).cpu().numpy()
    scale = dy.abs().double().sum(0).view(16, 2).cpu().numpy()
    assert np.all(np.abs(sums - ref) <= scale * 2.0 ** -8 + 1e-2)


MLP_CASES = [(32, 64, 4, 2), (16, 16, 3, 1), (48, 32, 16, 3), (32, 128, 16, 4), (128, 64, 5, 2), (64, 64, 16, 2), (16, 32, 2, 4),
             (32, 64, 4, 6), (32, 128, 8, 8),  # deeper than the register-resident kernels (layer-by-layer backward)
             (32, 64, 40, 2), (16, 32, 100, 3)]  # more than 16 outputs


@pytest.mark.parametrize("IN,W,OUT,H", MLP_CASES)
def test_network_forward_backward(IN, W, OUT, H):
    """tcnn.Network == identity encoding (padded with 1, identity.h:62-64) + FullyFusedMLP; reference
    tests/test_networks.cu:38-79 sweeps the same width / depth space."""
    C = tcnn()._C
    n_in = IN - 3  # exercises the padding of the identity encoding
    # deeper than 4 hidden layers (layer-by-layer backward): linear activations, so that a hidden value that is a tiny
    # positive number in one implementation and exactly zero in the other cannot flip a ReLU mask for the layers below
    # (measured: a handful of samples per batch at depth 8) -- the ReLU variant is covered by test_deep_network_trains
    act = "ReLU" if H <= 4 else "None"
    m = C.create_network(n_in, OUT, dict(MLP_64x2, n_neurons=W, n_hidden_layers=H, activation=act))
    om = O.mlp_init(IN, W, OUT, H, activation=O.ACTIVATION_NAMES.index(act))
    assert m.n_params() == om.n_params and m.n_output_dims() == om.padded_out == (OUT + 15) // 16 * 16
    p32 = m.initial_params(1337).cpu().numpy()
    assert np.array_equal(p32, O.mlp_init_params(om, O.pcg32(1337)))  # Xavier draw order, gpu_matrix.h:292-307
    ph = O.f2h(p32)
    n = 1024
    rng = np.random.default_rng(3)
    xin = rng.random((n, n_in), dtype=np.float32)
    x = torch.from_numpy(xin).cuda().requires_grad_(True)
    p = h_t(ph).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    _, y_inf = m.fwd(x.detach(), p.detach())
    torch.cuda.synchronize()
    enc = O.identity_forward(xin, IN)
    hid_ref, out_ref = O.mlp_forward(om, ph, enc)
    assert torch.equal(y, y_inf)                                       # inference == forward (test_common.h:160-165)
    bar = 3e-3 if H <= 4 else 1e-2                                     # eight fp16 roundings in a row: the reference's own bar
    assert np.percentile(rae(O.h2f(h_np(y)), O.h2f(out_ref)), 99) < bar
    assert np.max(np.abs(O.h2f(h_np(y)) - O.h2f(out_ref))) < 2e-2 * max(1.0, np.abs(O.h2f(out_ref)).max())

    dy = np.zeros((n, om.padded_out), np.float32)
    dy[:, :OUT] = rng.standard_normal((n, OUT)).astype(np.float32) * 0.05
    dyh = O.f2h(dy)
    dx, dp = m.bwd(ctx, x, p, y, h_t(dyh))
    torch.cuda.synchronize()
    gref, dref = O.mlp_backward(om, ph, enc, hid_ref, out_ref, dyh)
    g = dp.float().cpu().numpy()
    dx_ref = O.h2f(dref)[:, :n_in]
    # the reference's own bar (test_common.h:216-218) up to 4 hidden layers; deeper stacks compound one fp16 rounding per
    # layer in both implementations (measured p99.9: 1.6e-2 at depth 6, 2.4e-2 at depth 8), so the bar grows with depth
    assert np.percentile(rae(g, gref), 99.9) < 1.2e-2 * max(1.0, H / 3.0)
    assert np.percentile(rae(g, gref), 99) < bar
    assert np.allclose(dx.cpu().numpy(), dx_ref, rtol=2e-2, atol=(2e-3 if H <= 4 else 6e-3) * np.abs(dx_ref).max())


@pytest.mark.parametrize("d,n_bins", [(2, 64), (3, 16), (1, 4)])
def test_oneblob_encoding(d, n_bins):
    """OneBlob (encodings/oneblob.h:84-164, BASELINE configs[0]'s encoding) through the module API: the bin integrals are the
    oracle's bits, dL/dinput matches its restatement of kernel_one_blob_backward."""
    C = tcnn()._C
    m = C.create_encoding(d, {"otype": "OneBlob", "n_bins": n_bins})
    assert m.n_output_dims() == d * n_bins and m.n_params() == 0 and m.hyperparams() == {"otype": "OneBlob", "n_bins": n_bins}
    n = 1024
    rng = np.random.default_rng(21)
    xin = rng.random((n, d), dtype=np.float32)
    x = torch.from_numpy(xin).cuda().requires_grad_(True)
    p = torch.zeros(0, dtype=torch.float16, device="cuda")
    ctx, y = m.fwd(x, p)
    assert np.array_equal(h_np(y), O.oneblob_forward(xin, n_bins))
    dy = O.f2h(rng.standard_normal((n, d * n_bins)).astype(np.float32))
    dx, _ = m.bwd(ctx, x, p, y, h_t(dy))
    ref = O.oneblob_backward(xin, n_bins, dy)
    assert np.allclose(dx.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    with pytest.raises(RuntimeError, match="power of 2"):
        C.create_encoding(2, {"otype": "OneBlob", "n_bins": 48})


@pytest.mark.parametrize("d,n_frequencies", [(3, 12), (2, 6)])
def test_frequency_encoding(d, n_frequencies):
    """Frequency encoding (encodings/frequency.h:46-104) through the module API against the oracle: device sinf / cosf vs the
    host's differ in the last fp32 bit at most, i.e. in the fp16 output bit of a few entries; and as a network's input."""
    C = tcnn()._C
    m = C.create_encoding(d, {"otype": "Frequency", "n_frequencies": n_frequencies})
    assert m.n_output_dims() == 2 * d * n_frequencies and m.n_params() == 0
    assert m.hyperparams() == {"otype": "Frequency", "n_frequencies": n_frequencies}
    n = 2048
    rng = np.random.default_rng(22)
    xin = rng.random((n, d), dtype=np.float32)
    x = torch.from_numpy(xin).cuda().requires_grad_(True)
    p = torch.zeros(0, dtype=torch.float16, device="cuda")
    ctx, y = m.fwd(x, p)
    got, ref = h_np(y), O.frequency_forward(xin, n_frequencies)
    assert np.mean(got != ref) < 2e-3 and np.max(np.abs(O.h2f(got) - O.h2f(ref))) <= 2.0 ** -10
    dy = O.f2h(rng.standard_normal((n, 2 * d * n_frequencies)).astype(np.float32))
    dx, _ = m.bwd(ctx, x, p, y, h_t(dy))
    dref = O.frequency_backward(xin, n_frequencies, dy)
    assert np.allclose(dx.cpu().numpy(), dref, rtol=1e-4, atol=1e-4 * np.abs(dref).max())
    # NeRF-style: positional encoding + MLP trains (72 -> 80 padded inputs for d = 3: the tiled network kernels)
    T = tcnn()
    cfg = {"loss": {"otype": "RelativeL2"}, "optimizer": dict(ADAM_HASH), "encoding": {"otype": "Frequency", "n_frequencies": n_frequencies},
           "network": dict(MLP_64x2)}
    tm = T.create_from_config(d, 3, cfg, seed=5)
    pos = positions(1 << 13, d, seed=6)
    xx, tt = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 3)).cuda()
    first = tm.loss(tm.training_step(xx, tt))
    for _ in range(40):
        tm.training_step(xx, tt, want_context=False)
    assert tm.loss(tm.training_step(xx, tt)) < 0.5 * first


def test_config_oneblob_trains_and_matches_the_composed_oracle():
    """BASELINE configs[0]: data/config_oneblob.json as shipped (OneBlob 64 bins + FullyFusedMLP 128 x 5, RelativeL2, Adam) on
    2-D -> 3 data.  Inference equals oracle(one-blob) -> oracle(MLP) on the trained fp16 parameters; the loss drops."""
    T = tcnn()
    cfg = {"loss": {"otype": "RelativeL2"},
           "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-8, "l2_reg": 1e-8},
           "encoding": {"otype": "OneBlob", "n_bins": 64},
           "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 128, "n_hidden_layers": 5}}
    tm = T.create_from_config(2, 3, cfg, seed=1337)
    assert tm.n_params == 128 * 128 + 4 * 128 * 128 + 16 * 128
    n = 1 << 14
    pos = positions(n, 2, seed=5)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 3)).cuda()
    first = tm.loss(tm.training_step(x, t))
    for _ in range(60):
        tm.training_step(x, t, want_context=False)
    last = tm.loss(tm.training_step(x, t))
    assert np.isfinite(last) and last < 0.25 * first
    y = tm.inference(x).cpu().numpy()
    om = O.mlp_init(128, 128, 3, 5)
    ph = h_np(tm.params)
    _, out_ref = O.mlp_forward(om, ph, O.oneblob_forward(pos, 64))
    ref = O.h2f(out_ref)[:, :3]
    assert np.percentile(rae(y, ref), 99) < 1e-2 and np.max(np.abs(y - ref)) < 3e-2 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("d,enc,net,out", [
    (3, HASH_ENCODING_SMALL, MLP_64x2, 4),
    (2, HASH_ENCODING_SMALL, MLP_64x2, 3),
    (3, dict(HASH_ENCODING, log2_hashmap_size=17, n_levels=20), dict(MLP_64x2, n_neurons=128, n_hidden_layers=4), 16),  # cfg 5 shape
])
def test_network_with_input_encoding(d, enc, net, out):
    C = tcnn()._C
    m = C.create_network_with_input_encoding(d, out, enc, net)
    og = oracle_grid(enc, d)
    md = O.model_init(d, out, og, net["n_neurons"], net["n_hidden_layers"])
    assert m.n_params() == md.n_params
    p32 = m.initial_params(1337).cpu().numpy()
    assert np.array_equal(p32, O.model_init_params(md, 1337))          # MLP Xavier then grid U(-1e-4, 1e-4)
    p32[md.mlp.n_params:] *= 3.0e3                                      # make the encoding matter numerically
    ph = O.f2h(p32)
    n = 2048
    pos = positions(n, d, seed=11)
    x = torch.from_numpy(pos).cuda()
    p = h_t(ph).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    torch.cuda.synchronize()
    enc_ref = O.grid_forward(og, ph[md.mlp.n_params:], pos, out_stride=md.mlp.in_width)
    hid_ref, out_ref = O.mlp_forward(md.mlp, ph[:md.mlp.n_params], enc_ref)
    assert np.percentile(rae(O.h2f(h_np(y)), O.h2f(out_ref)), 99) < 3e-3
    rng = np.random.default_rng(5)
    dy = np.zeros((n, 16), np.float32)
    dy[:, :out] = rng.standard_normal((n, out)).astype(np.float32) * 0.05
    dyh = O.f2h(dy)
    _, dp = m.bwd(ctx, x, p, y, h_t(dyh))
    torch.cuda.synchronize()
    gref, denc = O.mlp_backward(md.mlp, ph[:md.mlp.n_params], enc_ref, hid_ref, out_ref, dyh)
    g = dp.float().cpu().numpy()
    assert np.percentile(rae(g[:md.mlp.n_params], gref), 99) < 3e-3
    ggrid = O.grid_backward(og, pos, denc)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(denc))))
    # dL/d(encoding) itself carries MLP fp16 noise: compare with the exact scatter of the ORACLE's dL/denc
    assert np.all(np.abs(g[md.mlp.n_params:] - ggrid) <= absacc * 2.0 ** -7 + 1e-3 * np.abs(ggrid).max())


def _trainer_and_oracle(cfg, d, out, seed=1337):
    T = tcnn()
    tm = T.create_from_config(d, out, cfg, seed=seed)
    og = oracle_grid(cfg["encoding"], d)
    adam = O.adam_defaults(**{k: v for k, v in (("learning_rate", 1e-2), ("beta1", 0.9), ("beta2", 0.99), ("epsilon", 1e-15), ("l2_reg", 1e-6))})
    md = O.model_init(d, out, og, cfg["network"]["n_neurons"], cfg["network"]["n_hidden_layers"],
                      O.LOSS_NAMES.index(cfg["loss"]["otype"]), adam)
    return tm, md


def targets_for(pos, out):
    return np.stack([0.5 + 0.5 * np.sin(2 * np.pi * (c + 1) * pos[:, 0]) * np.cos(2 * np.pi * pos[:, 1]) for c in range(out)], 1).astype(np.float32)


@pytest.mark.parametrize("width,hidden_layers,n_features,out,act,out_act,loss", [
    (128, 4, 2, 16, "ReLU", "None", "RelativeL2"),    # BASELINE configs[4]'s network: k_mlp_train_wide<3, 1>
    (128, 2, 4, 3, "LeakyReLU", "Sigmoid", "L1"),     # 64 inputs, out-of-line activations / loss: k_mlp_train_wide<1, 2, general>
    (128, 1, 2, 4, "ReLU", "None", "L2"),
    (64, 2, 4, 4, "ReLU", "None", "RelativeL2"),      # BASELINE configs[1]'s network shape (64 inputs, 64 x 2): k_mlp_train_wave<64, 64, 1> at one wave per SIMD
    (64, 1, 4, 16, "ReLU", "None", "L2"),             # k_mlp_train_wave<64, 64, 0>
])
def test_wide_network_fused_training_step(width, hidden_layers, n_features, out, act, out_act, loss):
    """128-neuron networks (and the 64-input instances of the register-resident kernel): training_step's single kernel (k_mlp_train_wide: weights resident in LDS, transpose reads, weight
    gradients in registers across eight 32-sample tiles per workgroup at this batch) against forward() + backward(), which run
    k_mlp_forward -> k_loss -> k_mlp_backward: same bits for prediction, loss gradient and everything that flows into the
    encoding; the fp32 weight-gradient sums are grouped per 32 instead of per 64 samples.  ReLU cases also against the oracle."""
    cfg = config_hash(log2_hashmap_size=15, per_level_scale=1.5, n_neurons=width, n_hidden_layers=hidden_layers, loss=loss)
    cfg["encoding"]["n_features_per_level"] = n_features
    cfg["network"].update(activation=act, output_activation=out_act)
    T = tcnn()
    tm = T.create_from_config(3, out, cfg)
    init = tm.params_full_precision.cpu().numpy().copy()
    nm = tm.n_mlp_params
    init[nm:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))
    n = 1 << 16  # 2048 tiles over 256 workgroups
    pos = positions(n, 3, seed=33)
    tgt = targets_for(pos, out)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    dx_f = torch.zeros((n, 3), device="cuda")
    ctx = tm.training_step(x, t, run_optimizer=False, dL_dinput=dx_f)
    loss_f = tm.loss(ctx)
    out_f, dy_f, g_f = h_np(ctx.output), h_np(ctx.dL_doutput), h_np(tm.param_gradients).copy()
    dx_u = torch.zeros((n, 3), device="cuda")
    T._C.set_fused_network_passes(False)  # forward() saves the activations, backward() is k_mlp_backward
    try:
        ctx_u = tm.forward(x, t, prepare_input_gradients=True)
        tm.backward(ctx_u, x, dL_dinput=dx_u)
    finally:
        T._C.set_fused_network_passes(True)
    g_u = h_np(tm.param_gradients)
    assert np.array_equal(out_f, h_np(ctx_u.output)) and np.array_equal(dy_f, h_np(ctx_u.dL_doutput))
    assert abs(loss_f - tm.loss(ctx_u)) <= 1e-5 * abs(loss_f)
    if width == 128:
        assert torch.equal(dx_f, dx_u)                             # dL/d(encoded input) has the same bits ...
    else:  # the register-resident kernel sums dL/d(encoded input) in another association order: a last fp16 bit in ~1e-5 of its entries
        assert torch.allclose(dx_f, dx_u, rtol=1e-2, atol=1e-3 * float(dx_u.abs().max()))
    ge_f, ge_u = O.h2f(g_f[nm:]), O.h2f(g_u[nm:])                  # ... the coarse levels' fp16 atomics add them in run-dependent order
    assert np.allclose(ge_f, ge_u, rtol=2e-2, atol=2e-3 * np.abs(ge_u).max())
    a, b = O.h2f(g_f[:nm]), O.h2f(g_u[:nm])
    ordered = lambda bits: np.where(bits & 0x8000, -(bits & 0x7FFF).astype(np.int32), (bits & 0x7FFF).astype(np.int32))  # monotonic in the value
    assert np.mean(g_f[:nm] != g_u[:nm]) < 0.05 and np.abs(ordered(g_f[:nm]) - ordered(g_u[:nm])).max() <= 2  # a last fp16 bit or two
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    if act != "ReLU":
        return
    og = oracle_grid(cfg["encoding"], 3)
    md = O.model_init(3, out, og, width, hidden_layers, O.LOSS_NAMES.index(loss), O.adam_defaults(learning_rate=1e-2, beta2=0.99, epsilon=1e-15, l2_reg=1e-6))
    assert md.n_params == tm.n_params
    st = O.TrainState(md, init)
    m = 4096  # the oracle's 128 x 4 step at the full batch takes a while; the first tiles are enough for it
    ctx = tm.training_step(x[:m].contiguous(), t[:m].contiguous(), run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos[:m], tgt[:m], run_optimizer=False, want_prediction=True)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-3 * abs(loss_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output))[:, :out], O.h2f(pred_ref)[:, :out]), 99) < 3e-3
    g, gref = tm.param_gradients.float().cpu().numpy(), O.h2f(st.grads)
    assert np.percentile(rae(g[:nm], gref[:nm]), 99) < 5e-3
    big = np.abs(gref[nm:]) > 1e-2 * np.abs(gref[nm:]).max()
    assert np.percentile(rae(g[nm:][big], gref[nm:][big]), 99) < 3e-2


@pytest.mark.parametrize("width,hidden_layers,n_features,out,act,out_act", [
    (64, 2, 2, 4, "ReLU", "None"),          # headline network: register-resident kernel
    (64, 3, 2, 16, "ReLU", "None"),         # workgroup-tiled kernel
    (128, 4, 2, 16, "ReLU", "None"),        # LDS-resident weights
    (64, 2, 4, 3, "Tanh", "Sigmoid"),       # 64 inputs, out-of-line activations, output activation transfer inside the kernel
    (64, 2, 4, 4, "ReLU", "None"),          # 64 inputs, 64 x 2: the one-wave-per-SIMD instance of the register-resident kernel (external dL/doutput)
    (32, 4, 2, 5, "LeakyReLU", "None"),
    # instances whose register allocation spills (k_mlp_train<64, 3>, k_mlp_train_wide<3, 1, general>): the resource report is not
    # a proof of anything either way -- results are
    (64, 4, 2, 4, "ReLU", "None"),
    (64, 4, 2, 4, "Tanh", "None"),
    (128, 4, 2, 16, "LeakyReLU", "Softplus"),
])
def test_backward_recomputing_the_forward_pass_matches_saved_activations(width, hidden_layers, n_features, out, act, out_act):
    """Module forward + backward (what the PyTorch binding runs): with single-kernel network passes the context keeps the encoded
    input only and the backward kernel recomputes the activations; against the path that saves them and runs k_mlp_backward."""
    T = tcnn()
    C = T._C
    enc = dict(HASH_ENCODING_SMALL, n_features_per_level=n_features)
    net = dict(MLP_64x2, n_neurons=width, n_hidden_layers=hidden_layers, activation=act, output_activation=out_act)
    m = C.create_network_with_input_encoding(3, out, enc, net)
    p32 = m.initial_params(1337)
    nm = m.n_params() - oracle_grid(enc, 3).n_params
    p32[nm:] *= 3.0e3
    n = 1 << 15
    x = torch.from_numpy(positions(n, 3, seed=5)).cuda().requires_grad_(True)  # input gradients too
    rng = np.random.default_rng(9)
    dy = np.zeros((n, 16), np.float32)
    dy[:, :out] = rng.standard_normal((n, out)).astype(np.float32) * 0.05
    dyh = h_t(O.f2h(dy))
    results = []
    for fused in (True, False):
        C.set_fused_network_passes(fused)
        try:
            p = p32.half().cuda().requires_grad_(True)
            ctx, y = m.fwd(x, p)
            dx, dp = m.bwd(ctx, x, p, y, dyh)
            torch.cuda.synchronize()
            results.append((h_np(y), None if dx is None else dx.float().cpu().numpy(), h_np(dp)))
        finally:
            C.set_fused_network_passes(True)
    (y_f, dx_f, g_f), (y_u, dx_u, g_u) = results
    assert np.array_equal(y_f, y_u)
    close = lambda a, b: np.abs(O.h2f(a) - O.h2f(b)).max() <= 2.0 ** -9 * np.abs(O.h2f(b)).max()
    assert np.isfinite(O.h2f(g_f)).all() and np.abs(O.h2f(g_f[:nm])).max() > 0
    assert np.mean(g_f[:nm] != g_u[:nm]) < 0.05 and close(g_f[:nm], g_u[:nm])
    ge_f, ge_u = O.h2f(g_f[nm:]), O.h2f(g_u[nm:])
    assert np.allclose(ge_f, ge_u, rtol=2e-2, atol=2e-3 * np.abs(ge_u).max())
    if dx_f is not None:
        assert np.allclose(dx_f, dx_u, rtol=1e-2, atol=1e-3 * np.abs(dx_u).max())


@pytest.mark.parametrize("loss", ["RelativeL2", "L2", "L1", "RelativeL1", "Mape", "Smape", "RelativeL2Luminance"])
def test_training_step_matches_oracle(loss):
    """create_from_config -> trainer.training_step -> trainer.loss -> network.inference against the oracle's
    whole-step restatement, starting from identical fp32 master parameters."""
    cfg = config_hash(log2_hashmap_size=15, per_level_scale=1.5, loss=loss)
    tm, md = _trainer_and_oracle(cfg, 3, 4)
    # Trainer seed path: std::seed_seq{1337} -> pcg32 (trainer.h:53-56)
    rng = O.pcg32(O.seed_seq_first(1337))
    init = np.concatenate([O.mlp_init_params(md.mlp, rng), O.generate_random_uniform(rng, md.grid.n_params, -1e-4, 1e-4)])
    assert np.array_equal(tm.params_full_precision.cpu().numpy(), init)
    assert np.array_equal(h_np(tm.params), O.f2h(init))
    init[md.mlp.n_params:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))
    st = O.TrainState(md, init)
    n = 4096
    pos = positions(n, 3, seed=21)
    tgt = targets_for(pos, 4)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()

    # step 0 without the optimizer: loss, prediction, gradients
    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    assert abs(tm.loss(ctx) - loss_ref) <= 2e-3 * abs(loss_ref)
    assert np.percentile(rae(O.h2f(h_np(ctx.output)), O.h2f(pred_ref)), 99) < 3e-3
    v_ref, g_ref = O.loss(md.loss_type, h_np(ctx.output), tgt, 4)
    assert np.array_equal(h_np(ctx.dL_doutput), g_ref)                 # loss gradient: bit-exact on the GPU's own prediction
    g = tm.param_gradients.float().cpu().numpy()
    gref = O.h2f(st.grads)
    nm = md.mlp.n_params
    assert np.percentile(rae(g[:nm], gref[:nm]), 99) < 5e-3
    big = np.abs(gref[nm:]) > 1e-2 * np.abs(gref[nm:]).max()
    assert np.percentile(rae(g[nm:][big], gref[nm:][big]), 99) < 3e-2

    # three optimizer steps: parameters track the oracle, the loss goes down
    losses, losses_ref = [], []
    for _ in range(3):
        ctx = tm.training_step(x, t)
        losses.append(tm.loss(ctx))
        losses_ref.append(O.training_step(st, pos, tgt))
    assert tm.optimizer_step_count == 3
    assert np.allclose(losses, losses_ref, rtol=2e-2)
    assert losses[-1] < losses[0]
    w = tm.params_full_precision.cpu().numpy()
    # Adam normalises the update to ~lr per step, so after 3 steps |w - w_ref| stays well below 3*lr except
    # where a near-zero gradient flips sign between the two implementations
    assert np.mean(np.abs(w - st.w32) > 1e-2) < 2e-3
    out = tm.inference(x).cpu().numpy()
    ref = O.inference(md, pos, st.w16)
    assert out.shape == (n, 4)
    assert np.percentile(np.abs(out - ref), 99) < 5e-2


def test_gradient_modes_and_data_parallel_linearity():
    """GradientMode::Accumulate adds; and with the global-batch normalisation the gradients of two half
    batches SUM to the gradient of the whole batch (what the RCCL all-reduce relies on), at BASELINE size."""
    T = tcnn()
    cfg = config_hash()
    tm = T.create_from_config(3, 4, cfg)
    n = 1 << 18
    pos = positions(n, 3, seed=3)
    tgt = targets_for(pos, 4)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    w = tm.params_full_precision.clone()
    w[tm.n_mlp_params:] *= 1.0e3
    tm.set_params_full_precision(w)
    tm.training_step(x, t, run_optimizer=False, want_context=False)
    full = tm.param_gradients.float().clone()
    tm.training_step(x, t, run_optimizer=False, gradient_mode=T._C.GradientMode.Accumulate, want_context=False)
    twice = tm.param_gradients.float().clone()
    assert torch.allclose(twice, 2 * full, rtol=2e-2, atol=2e-3 * full.abs().max().item())
    tm.set_global_batch_size(n)
    h = n // 2
    tm.training_step(x[:h].contiguous(), t[:h].contiguous(), run_optimizer=False, want_context=False)
    tm.training_step(x[h:].contiguous(), t[h:].contiguous(), run_optimizer=False, gradient_mode=T._C.GradientMode.Accumulate, want_context=False)
    halves = tm.param_gradients.float().clone()
    nm = tm.n_mlp_params
    assert torch.allclose(halves[:nm], full[:nm], rtol=2e-2, atol=2e-3 * full[:nm].abs().max().item())
    err = (halves[nm:] - full[nm:]).abs()
    assert (err > 2e-2 * full[nm:].abs().max()).float().mean().item() < 1e-4
    assert torch.isfinite(full).all()


def test_full_size_training_converges():
    """BASELINE config 3 at N = 2^18: loss decreases over a short run; inference is deterministic."""
    T = tcnn()
    tm = T.create_from_config(3, 4, config_hash())
    n = 1 << 18
    pos = positions(n, 3, seed=5)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()
    losses = []
    for i in range(30):
        ctx = tm.training_step(x, t)
        if i % 5 == 0 or i == 29:
            losses.append(tm.loss(ctx))
    assert all(np.isfinite(losses)) and losses[-1] < 0.6 * losses[0], losses
    a, b = tm.inference(x), tm.inference(x)
    assert torch.equal(a, b)


@pytest.fixture(params=["compiled", "ctypes"])
def binding(request, monkeypatch):
    """Both bindings behind the tinycudann modules: the compiled extension (tinycudann/ext/torch_module.cpp -> _tcnn_ext.so: pybind11 Module + the
    autograd function pair in C++, what the reference ships) and the ctypes classes of _C.py (the fallback when the extension is not built)."""
    C = tcnn()._C
    if request.param == "compiled":
        assert C.EXT is not None, "the compiled binding is missing: __graft_entry__.build() builds tiny-cuda-nn_amd/tinycudann/_tcnn_ext.so"
        assert "_tcnn_ext" in open("/proc/self/maps").read()
    else:
        monkeypatch.setattr(C, "EXT", None)
    return request.param


def test_torch_modules_autograd_and_padding(binding):
    """modules.py surface: batch padding to 256, output slicing, loss-scale handling, two forwards then one
    backward (scripts/test_torch_bindings.py), pickling."""
    T = tcnn()
    model = T.NetworkWithInputEncoding(3, 4, HASH_ENCODING_SMALL, MLP_64x2, seed=1337)
    assert type(model.native_tcnn_module).__name__ == ("ExtModule" if binding == "compiled" else "Module")
    assert model.params.dtype == torch.float32 and model.params.shape[0] == model.native_tcnn_module.n_params()
    with torch.no_grad():
        model.params[7168:] *= 1.0e3  # lift the U(-1e-4, 1e-4) grid init out of the fp16 subnormal range
    n = 1000  # not a multiple of 256
    pos = positions(n, 3, seed=9)
    x = torch.from_numpy(pos).cuda()
    y1 = model(x)
    y2 = model(x)
    assert y1.shape == (n, 4) and y1.dtype == torch.half and torch.equal(y1, y2)
    tgt = torch.from_numpy(targets_for(pos, 4)).cuda()
    loss = ((y2.float() - tgt) ** 2).mean()
    loss.backward()
    g = model.params.grad
    assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all() and g.abs().sum() > 0
    # oracle gradient of the same objective
    og = oracle_grid(HASH_ENCODING_SMALL, 3)
    md = O.model_init(3, 4, og, 64, 2)
    ph = h_np(model.params.detach().half())
    npad = 1024
    pos_p = np.zeros((npad, 3), np.float32)
    pos_p[:n] = pos
    enc = O.grid_forward(og, ph[md.mlp.n_params:], pos_p, out_stride=32)
    hid, out = O.mlp_forward(md.mlp, ph[:md.mlp.n_params], enc)
    dy = np.zeros((npad, 16), np.float32)
    dy[:n, :4] = (2.0 * (O.h2f(out)[:n, :4] - tgt.cpu().numpy()) / (n * 4)) * 128.0
    gref, _ = O.mlp_backward(md.mlp, ph[:md.mlp.n_params], enc, hid, out, O.f2h(dy))
    # the binding divides the fp16 gradient by the loss scale IN fp16 (modules.py:170): 2^-24 quantisation
    gm, ref = g[:md.mlp.n_params].cpu().numpy(), gref / 128.0
    assert np.all(np.abs(gm - ref) <= 1.2e-7 + 1e-2 * np.abs(ref))
    assert np.abs(ref).max() > 1e-5
    # Network and Encoding modules
    net = T.Network(5, 3, dict(MLP_64x2, n_neurons=32))
    assert net(torch.rand(300, 5, device="cuda")).shape == (300, 3)
    enc_m = T.Encoding(3, HASH_ENCODING_SMALL)
    assert enc_m.n_output_dims == 32 and enc_m(x).shape == (n, 32)
    clone = pickle.loads(pickle.dumps(model))
    assert torch.equal(clone(x), y1)


def test_fp32_encoding_module(binding):
    """tcnn.Encoding(..., dtype=torch.float32) = create_encoding(Precision::Fp32) -> Encoding<float> (cpp_api.cu:165-174): fp32 parameters,
    features and gradients, COMPUTED in fp32 as the reference's instantiation does -- against the oracle's fp32 restatement (pinned to the
    reference's kernel_grid<float> / kernel_grid_backward<float, float> / kernel_grid_backward_input<float>, tests/test_oracle_ref.py).
    Bars (fp32, stated here): encoded features and dy_dx-based input gradients bit for bit; parameter gradients within the rounding of a
    running fp32 sum (hits x 2^-24 x sum of the magnitudes); a gradient of magnitude 1e4 -- beyond anything the 16-bit path could hold
    after its loss scale -- comes through exactly linear."""
    T = tcnn()
    og = O.grid_init(3, 16, 2, 15, 16, 1.5)
    enc_f = T.Encoding(3, HASH_ENCODING_SMALL, seed=5, dtype=torch.float32)
    assert enc_f.params.dtype == torch.float32 and enc_f.native_tcnn_module.param_precision() == T._C.Precision.Fp32
    rng = np.random.default_rng(2)
    params = (rng.standard_normal(og.n_params) * 0.3).astype(np.float32)  # values that are no 16-bit numbers
    with torch.no_grad():
        enc_f.params.copy_(torch.from_numpy(params))
    n = 2048
    pos = positions(n, 3, seed=12)
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = enc_f(x)
    want, dy_dx = O.grid_forward_f32(og, params, pos, want_dy_dx=True)
    assert y.dtype == torch.float32 and np.array_equal(y.detach().cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(want, O.h2f(O.f2h(want)))  # ... which a 16-bit computation could not have produced
    for magnitude in (1.0e-3, 1.0e4):
        w = (rng.standard_normal((n, 32)) * magnitude).astype(np.float32)
        x.grad, enc_f.params.grad = None, None
        (enc_f(x) * torch.from_numpy(w).cuda()).sum().backward()
        g, dx = enc_f.params.grad.cpu().numpy(), x.grad.cpu().numpy()
        g_want, mag = O.grid_backward_f32(og, pos, w), O.grid_backward_f32(og, pos, np.abs(w))
        idx = O.grid_indices(og, pos)
        hits = np.zeros(og.n_params // 2, np.int64)
        for l in range(16):
            np.add.at(hits, og.offsets[l] + idx[:, l, :].reshape(-1), 1)
        hits = np.repeat(hits, 2)
        assert np.isfinite(g).all() and np.all(np.abs(g - g_want) <= np.maximum(hits, 1) * 2.0 ** -24 * mag * 1.001), magnitude
        assert not g[hits == 0].any() and np.array_equal(g[hits == 1], g_want[hits == 1].astype(np.float32))
        assert np.array_equal(dx, O.grid_backward_input_f32(og, w, dy_dx)), magnitude
    # the element-wise encodings with float values: nothing is rounded to 16 bits on the way
    xs = pos.astype(np.float64)
    freq = T.Encoding(3, {"otype": "Frequency", "n_frequencies": 6}, dtype=torch.float32)
    yf = freq(x).detach().cpu().numpy()
    want_f = np.stack([np.sin(xs[:, j // 12] * 2.0 ** ((j // 2) % 6) * np.pi + (j % 2) * np.pi / 2) for j in range(36)], axis=1)
    assert yf.dtype == np.float32 and np.abs(yf - want_f).max() < 2e-5 and np.abs(yf - O.h2f(O.f2h(yf))).max() > 1e-5
    blob = T.Encoding(3, {"otype": "OneBlob", "n_bins": 16}, dtype=torch.float32)
    yb = blob(x).detach().cpu().numpy()
    assert np.abs(yb - O.h2f(O.oneblob_forward(pos, 16))).max() <= 2.0 ** -11 and np.abs(yb.reshape(n, 3, 16).sum(-1) - 1.0).max() < 1e-5  # bin integrals of a unit blob
    ident = T.Encoding(3, {"otype": "Identity"}, dtype=torch.float32)
    assert np.array_equal(ident(x).detach().cpu().numpy()[:, :3], pos)


def test_golden_fixture():
    """tests/golden/hotpath_small.npz (made by tests/golden/make_golden.py): the GPU path reproduces the
    frozen vectors without the oracle library in the loop."""
    C = tcnn()._C
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hotpath_small.npz"))
    m = C.create_network_with_input_encoding(3, 4, HASH_ENCODING_SMALL, MLP_64x2)
    p32 = m.initial_params(1337)
    assert np.array_equal(p32[:7168].cpu().numpy(), gold["params_fp32"])
    p32[7168:] *= 1.0e4
    assert np.array_equal(p32[7168:7168 + 4096].cpu().numpy(), gold["grid_params_first"])
    p = p32.half()
    assert int(h_np(p).astype(np.uint64).sum()) == int(gold["params_checksum"][0])
    x = torch.from_numpy(gold["positions"]).cuda()
    idx = m.grid_indices(x).cpu().numpy().view(np.uint32)
    assert np.array_equal(idx[:, 0], gold["indices_level0"]) and np.array_equal(idx[:, 15], gold["indices_level15"])
    assert int(idx.astype(np.uint64).sum()) == int(gold["indices_checksum"][0])
    e = C.create_encoding(3, HASH_ENCODING_SMALL)
    _, enc = e.fwd(x, p[7168:].contiguous())
    assert np.array_equal(h_np(enc), gold["encoded"])
    _, y = m.fwd(x, p)
    torch.cuda.synchronize()
    assert np.percentile(rae(O.h2f(h_np(y)), O.h2f(gold["output"])), 99) < 3e-3


def test_reference_golden_fixture():
    """tests/golden/reference_small.npz -- made by THE REFERENCE'S OWN kernel_grid / pcg32 / generate_random_kernel compiled for the
    host (tests/golden/make_ref_golden.py, oracle/build_ref.py): the HIP gather and the HIP generator reproduce the reference's
    output bit for bit, no oracle in the loop.  (encodings/grid.h:48-212, random.h:39-69)"""
    T = tcnn()
    C = T._C
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_small.npz"))
    n = gold["positions"].shape[0]
    x = C.Pcg32(1337).uniform_(torch.empty((n, 3), device="cuda"))
    assert np.array_equal(x.cpu().numpy(), gold["positions"])
    e = C.create_encoding(3, HASH_ENCODING_SMALL)
    u = C.Pcg32(int(gold["grid_seed"][0])).uniform_(torch.empty(e.n_params(), device="cuda"))
    grid = (2.0 * u - 1.0).half()  # exactly the fixture's fp32 arithmetic: 2u and 2u - 1 are single IEEE operations
    _, enc = e.fwd(x, grid)
    assert np.array_equal(h_np(enc), gold["encoded"])
    xg = x.clone().requires_grad_(True)
    ctx, enc2 = e.fwd(xg, grid)
    # dy_dx through the input gradient: dL_dx = sum_k dL_dy[k] dy_dx[k] with dL_dy = one-hot on feature k (kernel_grid_backward_input, grid.h:322-349)
    for k in (0, 13, 31):
        dy = torch.zeros_like(enc2)
        dy[:, k] = 1.0
        dx, _ = e.bwd(ctx, xg, grid, enc2, dy)
        assert np.array_equal(dx.cpu().numpy()[:16], gold["dy_dx_first"][:, k, :]), k


def test_reference_golden_fixture_loss_and_adam():
    """The loss and optimizer part of tests/golden/reference_small.npz -- made by THE REFERENCE'S OWN relative_l2_loss
    (losses/relative_l2.h:39-76) and adam_step (optimizers/adam.h:47-127) compiled for the host (tests/golden/make_ref_golden.py): the HIP
    loss kernel and the HIP Adam kernel against those vectors through the C ABI, no oracle in the loop.
    Bars: loss values and gradients bit for bit; Adam's first / second moments and per-parameter step counters bit for bit, the 16-bit
    weights equal to the rounded master weights of the run itself, the fp32 master weights within 4 ulp per step of the reference's (powf of
    the bias correction is not correctly rounded on either side; the same bar as the oracle-based Adam tests)."""
    T = tcnn()
    C = T._C
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_small.npz"))
    # ---- RelativeL2 on a [n][16] prediction with 4 live outputs, loss scale 128
    pred, targets = h_t(gold["prediction"]), torch.from_numpy(gold["targets"]).cuda()
    values, grads = C.loss_evaluate("RelativeL2", pred, targets, loss_scale=128.0)
    assert np.array_equal(h_np(grads), gold["loss_gradients"])
    assert np.array_equal(values.cpu().numpy().view(np.uint32), gold["loss_values"].view(np.uint32))
    # ---- three Adam steps (data/config_hash.json hyper-parameters), 1024 matrix weights + 3072 table entries of which some are skipped
    from tinycudann import native
    m, nm = gold["adam_w0"].size, 1024
    opt = native.Optimizer({"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}, m, nm)
    w = torch.from_numpy(gold["adam_w0"].copy()).cuda()
    h = w.half()
    for step in (1, 2, 3):
        opt.step(w, h, h_t(gold[f"adam_grad{step}"]), loss_scale=128.0)
    m1, m2, steps = opt.state()
    assert np.array_equal(steps.cpu().numpy().view(np.uint32), gold["adam_steps"])
    assert np.array_equal(m1.cpu().numpy().view(np.uint32), gold["adam_m1"].view(np.uint32))
    assert np.array_equal(m2.cpu().numpy().view(np.uint32), gold["adam_m2"].view(np.uint32))
    wg, wr = w.cpu().numpy(), gold["adam_w"]
    ulp = np.spacing(np.maximum(np.maximum(np.abs(wr), np.abs(gold["adam_w0"])), np.abs(wr - gold["adam_w0"])).astype(np.float32))
    # 4 ulp per step, three steps (measured on MI355X: 6 ulp after the third)
    assert np.all(np.abs(wg.astype(np.float64) - wr) <= 12 * ulp), float(np.max(np.abs(wg.astype(np.float64) - wr) / ulp))
    assert np.array_equal(h_np(h), O.f2h(wg))  # the 16-bit weights are the GPU's own master weights rounded to nearest even
    agree = np.mean(h_np(h) == gold["adam_h"])
    assert agree > 0.999, agree  # and thereby the reference's, up to the few whose master weight sits within 4 ulp of a rounding boundary


@pytest.mark.parametrize("tag", ["net_a", "net_b"])
def test_reference_golden_fixture_network(tag):
    """The network part of tests/golden/reference_small.npz: the output of THE REFERENCE'S OWN kernel_mlp_fused /
    kernel_mlp_fused_backward (src/fully_fused_mlp.cu:46-557 compiled for the host, tests/golden/make_ref_golden.py) for the bench's
    network and BASELINE configs[1]'s.  The HIP kernels against it through the C ABI, no oracle in the loop; bars and their
    measured values: tests/reference_fixture.py (the emulator leg runs the same check on the kernel sources)."""
    import reference_fixture as RF
    C = tcnn()._C
    gold = RF.load()
    in_w, out_w = RF.NETWORKS[tag]
    m = C.create_network(in_w, out_w, MLP_64x2)
    params, xh, dyh = gold[tag + "_params"], gold[tag + "_input"], gold[tag + "_dL_doutput"]
    assert m.n_params() == params.size and m.n_output_dims() == RF.PADDED_OUT
    x = torch.from_numpy(O.h2f(xh)).cuda().requires_grad_(True)  # fp16 values: the identity encoding's cast is exact
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    dx, dp = m.bwd(ctx, x, p, y, h_t(dyh))
    torch.cuda.synchronize()
    RF.check(gold, tag, O.h2f(h_np(y)), dp.float().cpu().numpy(), dx.float().cpu().numpy())


def test_error_behaviour_on_device():
    C = tcnn()._C
    m = C.create_network_with_input_encoding(3, 4, HASH_ENCODING_SMALL, MLP_64x2)
    p = m.initial_params(1).half()
    with pytest.raises(RuntimeError, match="multiple of 256"):     # object.h:170
        m.fwd(torch.rand(100, 3, device="cuda"), p)
    with pytest.raises(RuntimeError, match="wrong size"):
        m.fwd(torch.rand(256, 2, device="cuda"), p)
    with pytest.raises(RuntimeError, match="invalid context"):
        ctx, y = m.fwd(torch.rand(256, 3, device="cuda"), p)          # inference mode: no context
        m.bwd(ctx, torch.rand(256, 3, device="cuda"), p, y, y)


def test_mlp_keeps_fp16_subnormal_inputs():
    """The hash grid is initialised in U(-1e-4, 1e-4) (grid.h:1076-1079), i.e. mostly fp16 SUBNORMAL encodings:
    the MFMA path must not flush them (NVIDIA tensor cores do not), or early training differs from the reference."""
    C = tcnn()._C
    m = C.create_network(16, 4, MLP_64x2)
    om = O.mlp_init(16, 64, 4, 2)
    ph = O.f2h(m.initial_params(1337).cpu().numpy())
    rng = np.random.default_rng(11)
    xin = (rng.random((1024, 16), dtype=np.float32) * 2 - 1) * 3e-5     # |x| < 6.1e-5: subnormal in fp16
    x = torch.from_numpy(xin).cuda()
    _, y = m.fwd(x, h_t(ph))
    torch.cuda.synchronize()
    _, out_ref = O.mlp_forward(om, ph, O.identity_forward(xin, 16))
    ref = O.h2f(out_ref)[:, :4]
    assert np.abs(ref).max() > 1e-6
    assert np.max(np.abs(O.h2f(h_np(y))[:, :4] - ref)) <= 2.0 ** -23  # within two fp16 subnormal ulps


def test_snapshot_round_trip_resumes_training_bit_exactly():
    """Trainer::serialize/deserialize (trainer.h:442-481, adam.h:304-325): a model restored from a snapshot with
    optimizer state continues EXACTLY like the original; the bytes decode as the reference's document."""
    import msgpack
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=14)
    n = 1 << 12
    pos = positions(n, 3, seed=11)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()
    a = T.create_from_config(3, 4, cfg, seed=7)
    for _ in range(5):
        a.training_step(x, t, want_context=False)
    blob = a.serialize(serialize_optimizer=True)
    doc = msgpack.unpackb(blob, raw=False)
    assert doc["n_params"] == a.n_params and doc["params_type"] == "__half"
    assert doc["params_binary"] == a.params.cpu().numpy().tobytes()
    assert doc["optimizer"]["current_step"] == 5 and len(doc["optimizer"]["param_steps_binary"]) == 4 * a.n_params
    assert set(msgpack.unpackb(a.serialize(), raw=False)) == {"n_params", "params_type", "params_binary"}

    b = T.create_from_config(3, 4, cfg, seed=99)  # different init, then restored
    b.deserialize(blob)
    assert b.optimizer_step_count == 5 and torch.equal(a.params, b.params)
    # the fp16 snapshot drops the fp32 master's low bits (as in the reference, which stores params_inference): align a with it
    a.deserialize(blob)
    for _ in range(3):
        a.training_step(x, t, want_context=False)
        b.training_step(x, t, want_context=False)
    assert torch.equal(a.params_full_precision, b.params_full_precision)
    assert torch.equal(a.inference(x), b.inference(x))
    # fp32 parameter snapshots written by a reference build with fp32 params are accepted too (trainer.h:459-461)
    p32 = a.params_full_precision.cpu().numpy()
    b.deserialize(msgpack.packb({"n_params": int(a.n_params), "params_type": "float", "params_binary": p32.tobytes()}, use_bin_type=True))
    assert torch.equal(b.params_full_precision, a.params_full_precision)
    with pytest.raises(RuntimeError, match="wrong size"):
        b.deserialize(msgpack.packb({"n_params": 4, "params_type": "__half", "params_binary": b"12345678"}, use_bin_type=True))


@pytest.mark.parametrize("exe_name", ["learn_function", "learn_function_minijson"])
def test_cpp_facade_sample(exe_name):
    """The header-only C++ facade (include/tiny-cuda-nn/*.h) over the C ABI, with nlohmann::json and with the built-in
    JSON value: the sample application trains, infers, round-trips a snapshot, feeds row-major / strided GPUMatrixDynamic
    views (same bits as the dense column-major batch) and sees the reference's error for a bad batch size."""
    import subprocess
    exe = os.path.join(ROOT, "samples", exe_name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "samples"), "-s"])
    r = subprocess.run([exe, "150", "16384"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert "restored_inference_identical=1" in r.stdout and "layouts_identical=1" in r.stdout
    assert "loss_evaluate_matches_training_step=1" in r.stdout  # Loss<T>::evaluate on its own == the fused step's dL/doutput
    assert "optimizer_on_its_own=1" in r.stdout                  # Optimizer<T>::allocate + step over the host's own buffers
    assert "arena_block_reused=1" in r.stdout                    # GPUMatrix(m, n, stream): blocks of the stream-ordered cache


@pytest.mark.parametrize("name,with_pdf", [("RelativeL2", False), ("L2", True), ("L1", False), ("RelativeL1", True), ("Mape", False), ("Smape", False),
                                           ("RelativeL2Luminance", False)])
def test_loss_evaluate_on_its_own(name, with_pdf):
    """tcnn_loss_evaluate / Loss<T>::evaluate (loss.h:42-50): values and gradients of a padded prediction matrix against the oracle
    (itself pinned bit for bit against the reference's loss kernels, tests/test_oracle_ref.py): gradients bit-exact."""
    C = tcnn()._C
    rng = np.random.default_rng(3)
    n, stride, dims = 4096, 16, 5
    pred = O.f2h((rng.standard_normal((n, stride)) * 0.7).astype(np.float32))
    tgt = rng.random((n, dims), dtype=np.float32)
    pdf = (0.25 + rng.random((n, dims), dtype=np.float32)) if with_pdf else None
    v_ref, g_ref = O.loss(getattr(O, "LOSS_" + {"RelativeL2": "RELATIVE_L2", "L2": "L2", "L1": "L1", "RelativeL1": "RELATIVE_L1", "Mape": "MAPE", "Smape": "SMAPE",
                                                "RelativeL2Luminance": "RELATIVE_L2_LUMINANCE"}[name]), pred, tgt, dims, data_pdf=pdf)
    p = torch.from_numpy(pred.view(np.int16)).cuda().view(torch.half)
    values, grads = C.loss_evaluate(name, p, torch.from_numpy(tgt).cuda(), 128.0, None if pdf is None else torch.from_numpy(pdf).cuda())
    assert np.array_equal(grads.cpu().view(torch.int16).numpy().view(np.uint16), g_ref)
    assert np.allclose(values.cpu().numpy(), v_ref, rtol=1e-6, atol=1e-9)
    with pytest.raises(RuntimeError, match="not found"):
        C.loss_evaluate("NoSuchLoss", p, torch.from_numpy(tgt).cuda())


@pytest.mark.parametrize("clustered", [False, True])
def test_bucketed_grid_backward_full_size(clustered):
    """Bucket-once backward at BASELINE size (N = 2^18, T = 2^19): every bucketed level equals the exact sum rounded
    once (fixed-point accumulation) -- checked against the oracle on the levels, and against the fp32-slice
    formulation everywhere.  Clustered inputs overflow the bucket queues and take the atomic overflow pass."""
    C = tcnn()._C
    enc = dict(HASH_ENCODING)
    m = C.create_encoding(3, enc)
    og = oracle_grid(enc, 3)
    n = 1 << 18
    pos = positions(n, 3, seed=21)
    if clustered:
        pos[n // 4:] = pos[:3 * n // 4] * 0.01 + 0.37  # 3/4 of the batch inside a 1% cube
    rng = np.random.default_rng(3)
    dy = O.f2h((rng.standard_normal((n, m.n_output_dims())) * 0.02).astype(np.float32))
    x = torch.from_numpy(pos).cuda()
    p = torch.zeros(og.n_params, dtype=torch.half, device="cuda").requires_grad_(True)
    ctx, y = m.fwd(x, p)
    out = {}
    default_mode = C.get_grid_backward_mode()
    try:
        for mode in (0, 3):
            C.set_grid_backward_mode(mode)
            _, dp = m.bwd(ctx, x, p, y, h_t(dy))
            torch.cuda.synchronize()
            out[mode] = dp.float().cpu().numpy().astype(np.float64)
    finally:
        C.set_grid_backward_mode(default_mode)
    ref = O.grid_backward(og, pos, dy)
    absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))))
    assert np.all(np.abs(out[3] - ref) <= absacc * 2.0 ** -8 + 1e-3)
    assert np.all(np.abs(out[3] - out[0]) <= absacc * 2.0 ** -8 + 1e-3)
    if not clustered:  # no queue overflow: levels above 65536 entries are exact
        F = 2
        for l in range(og.n_levels):
            lo, hi = og.offsets[l] * F, og.offsets[l + 1] * F
            if og.offsets[l + 1] - og.offsets[l] > 65536:
                # (x-neighbour pairs straddling two slices -- about one in 2^13 -- take the overflow path: fp16 atomics)
                assert np.mean(out[3][lo:hi].astype(np.float32) == O.h2f(O.f2h(ref[lo:hi].astype(np.float32)))) > 0.998, f"level {l}"


@pytest.mark.parametrize("log2_t,scale", [(15, 1.5), (19, 2.0)])
def test_owner_pass_hand_pipelined_stream_at_every_queue_length(log2_t, scale):
    """The packed owner pass streams its queues through loads the compiler does not see (inline asm into registers that keep their
    identity, counted s_waitcnt: csrc/grid_backward_owner.hip bucket_level_packed).  That path is compiled out of the host
    emulator, so it is pinned here: batch sizes from 256 to 2^17 + 768 give the queues of the sixteen levels every kind of length -- empty
    (fine levels at small batches), shorter than one round of a lane, a few records more or less than whole rounds of 4 x NG x 512
    records -- and the gradients must equal, BIT FOR BIT, the 64-bit-per-value owner kernel's (mode 1: plain C++ loads, no pipelining)
    and the packed kernel's own 64-bit redo of every slice (mode 2) wherever a slice has a sole owner (chunked coarse levels sum the
    owners' results with fp16 atomics in either form and are compared within that rounding); the sole-owner levels are also exact
    against the oracle's sum rounded once."""
    C = tcnn()._C
    enc = dict(HASH_ENCODING, log2_hashmap_size=log2_t, per_level_scale=scale)
    m = C.create_encoding(3, enc)
    og = oracle_grid(enc, 3)
    rng = np.random.default_rng(5)
    default_owner = C.get_grid_owner_mode()
    try:
        for n in (256, 512, 1024, 3840, 4096 + 256, 1 << 14, (1 << 16) - 256, (1 << 17) + 768):
            pos = positions(n, 3, seed=100 + n % 97)
            dy = O.f2h((rng.standard_normal((n, m.n_output_dims())) * 0.05).astype(np.float32))
            x = torch.from_numpy(pos).cuda()
            p = torch.zeros(og.n_params, dtype=torch.half, device="cuda").requires_grad_(True)
            ctx, y = m.fwd(x, p)
            out = {}
            for owner in (0, 1, 2):
                C.set_grid_owner_mode(owner)
                _, dp = m.bwd(ctx, x, p, y, h_t(dy))
                torch.cuda.synchronize()
                out[owner] = dp.cpu().view(torch.int16).numpy().view(np.uint16).copy()
            ref = O.grid_backward(og, pos, dy)
            absacc = O.grid_backward(og, pos, O.f2h(np.abs(O.h2f(dy))))
            n_exact = 0
            for l in range(og.n_levels):
                lo, hi = og.offsets[l] * 2, og.offsets[l + 1] * 2
                same = np.array_equal(out[0][lo:hi], out[1][lo:hi]) and np.array_equal(out[0][lo:hi], out[2][lo:hi])
                if og.offsets[l + 1] - og.offsets[l] > 65536 or same:
                    assert same, (n, l)
                    n_exact += 1
                else:  # several owners per slice (sample chunks of a small table): their exact sums meet in fp16 atomics, one rounding per owner
                    a, b = O.h2f(out[0][lo:hi]).astype(np.float64), O.h2f(out[1][lo:hi]).astype(np.float64)
                    assert np.all(np.abs(a - b) <= absacc[lo:hi] * 2.0 ** -8 + 1e-3), (n, l)
            # (a small table at a large batch splits the SAMPLES of a slice over several owners -- per-bucket records beyond 65536 -- and no level is
            # exact then; the sole-owner regime is what the other cases pin bit for bit)
            if log2_t == 19 or n <= (1 << 14):
                assert n_exact >= 10, (n, n_exact)
            got = O.h2f(out[0]).astype(np.float64)
            assert np.all(np.abs(got - ref) <= absacc * 2.0 ** -8 + 1e-3), n
    finally:
        C.set_grid_owner_mode(default_owner)


@pytest.mark.parametrize("act,out_act", [("LeakyReLU", "None"), ("Exponential", "Sigmoid"), ("Sigmoid", "Exponential"), ("Squareplus", "Tanh"),
                                         ("Softplus", "Softplus"), ("Tanh", "Squareplus"), ("None", "ReLU")])
def test_network_activations(act, out_act):
    """Hidden / output activations of FullyFusedMLP (common_device.h:108-186, 363-418; fully_fused_mlp.cu:690-697,
    760-763) through tcnn.Network and through a trained model (fused training kernel) against the oracle."""
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
    scale = max(1.0, np.abs(O.h2f(out_ref)).max())
    assert np.max(np.abs(O.h2f(h_np(y)) - O.h2f(out_ref))) < 4e-3 * scale
    dy = np.zeros((n, 16), np.float32)
    dy[:, :OUT] = rng.standard_normal((n, OUT)).astype(np.float32) * 0.05
    dyh = O.f2h(dy)
    dx, dp = m.bwd(ctx, x, p, y, h_t(dyh))
    torch.cuda.synchronize()
    gref, dref = O.mlp_backward(om, ph, enc, hid_ref, out_ref, dyh)
    assert np.percentile(rae(dp.float().cpu().numpy(), gref), 99) < 6e-3
    dx_ref = O.h2f(dref)[:, :IN]
    assert np.allclose(dx.cpu().numpy(), dx_ref, rtol=3e-2, atol=4e-3 * np.abs(dx_ref).max())

    # the fused training kernel and the forward()+backward() pair give the same parameter gradients
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
    # ... up to the association order of fp32 sums: the register-resident kernel holds output 4r+g (not 4g+r) in k slot
    # (g, r) of the output layer's backward MFMA and groups the weight-gradient partial sums per wavefront, not per workgroup
    g_pair, nm = tm.param_gradients, tm.n_mlp_params
    grid_pair, grid_fused = g_pair[nm:].float(), g_fused[nm:].float()
    assert (grid_pair != grid_fused).float().mean() < 0.02
    assert torch.allclose(grid_pair, grid_fused, rtol=4e-3, atol=2e-3 * float(grid_fused.abs().max()))
    assert (g_pair[:nm] != g_fused[:nm]).float().mean() < 0.05
    assert torch.allclose(g_pair[:nm].float(), g_fused[:nm].float(), rtol=2e-3, atol=1e-3 * float(g_fused[:nm].float().abs().max()) * 2.0 ** -10 + 1e-7)
    assert abs(tm.loss(c2) - loss_fused) <= 1e-5 * abs(loss_fused) + 1e-9
    assert torch.isfinite(g_fused.float()).all()


@pytest.mark.parametrize("loss", ["CrossEntropy", "Variance"])
def test_losses_for_positive_predictions(loss):
    """CrossEntropy / Variance (cross_entropy.h:66-76, variance_is.h:66-76) need positive predictions: an Exponential
    output layer provides them.  Loss gradients are the oracle's bits on the GPU's own prediction."""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=14, loss=loss)
    cfg["network"] = dict(cfg["network"], output_activation="Exponential")
    tm = T.create_from_config(3, 4, cfg, seed=5)
    assert tm.hyperparams()["loss"]["otype"] == loss
    pos = positions(2048, 3, seed=8)
    tgt = targets_for(pos, 4)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    for fused in (True, False):
        ctx = tm.training_step(x, t, run_optimizer=False) if fused else tm.forward(x, t)
        pred = h_np(ctx.output)
        assert (O.h2f(pred)[:, :4] > 0).all()
        v_ref, g_ref = O.loss(O.LOSS_NAMES.index(loss), pred, tgt, 4)
        got, ref = O.h2f(h_np(ctx.dL_doutput)), O.h2f(g_ref)
        assert np.allclose(got, ref, rtol=2e-3, atol=1e-7)              # 1 / x and log on the device vs libm: an fp16 ulp at most
        assert np.mean(h_np(ctx.dL_doutput) == g_ref) > 0.99
        assert abs(tm.loss(ctx) - float(v_ref.sum(dtype=np.float64))) <= 1e-4 * abs(float(v_ref.sum(dtype=np.float64)))


def test_wrapper_optimizers_ema_and_exponential_decay():
    """instant-ngp style optimizer: Ema(ExponentialDecay(Adam)) -- optimizers/ema.h:45-141, exponential_decay.h:59-70.
    The learning-rate schedule is checked through the oracle's Adam, the EMA bit-exactly on the GPU's own weights."""
    import msgpack
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=14)
    adam = dict(cfg["optimizer"])
    cfg["optimizer"] = {"otype": "Ema", "decay": 0.9, "nested": {"otype": "ExponentialDecay", "decay_start": 2, "decay_interval": 2, "decay_base": 0.5,
                                                                 "nested": adam}}
    tm, md = _trainer_and_oracle(dict(cfg, optimizer=adam), 3, 4)
    del tm
    tm = T.create_from_config(3, 4, cfg)
    hp = tm.hyperparams()["optimizer"]
    assert hp["otype"] == "EMA" and hp["nested"]["otype"] == "ExponentialDecay" and hp["nested"]["nested"]["otype"] == "Adam"
    init = tm.params_full_precision.cpu().numpy().copy()
    init[md.mlp.n_params:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(init))
    st = O.TrainState(md, init)
    n = 2048
    pos = positions(n, 3, seed=2)
    tgt = targets_for(pos, 4)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    ema = np.zeros(tm.n_params, np.float32)   # fp16 average, held as the fp32 value of the half
    lr0, factor = adam["learning_rate"], 1.0
    for step in range(6):
        if step >= 2 and (step - 2) % 2 == 0:
            factor *= 0.5
        st.md.adam.learning_rate = np.float32(lr0) * np.float32(factor)
        tm.training_step(x, t, want_context=False)
        O.training_step(st, pos, tgt)
        w16 = O.h2f(h_np(tm.params))
        k = step + 1
        d = float(np.float32(0.9))  # std::pow(float, unsigned) runs in double on the FLOAT value of the decay (ema.h:113-114)
        old = np.float32(1 - np.float32(d ** (k - 1)))
        new = np.float32(1.0) / np.float32(1 - np.float32(d ** k))
        ema = O.h2f(O.f2h((ema * np.float32(0.9) * old + w16 * np.float32(1 - np.float32(0.9))) * new))
        assert np.array_equal(O.h2f(h_np(tm.params_inference)), ema), f"EMA after step {k}"
    assert abs(tm.hyperparams()["optimizer"]["nested"]["nested"]["learning_rate"] - lr0 * 0.25) < 1e-8
    m, ref = tm.params_full_precision.cpu().numpy(), st.w32
    assert np.percentile(np.abs(m - ref)[:md.mlp.n_params], 99) < 2e-3
    # inference uses the EMA weights by default (object.h:214-271 use_inference_params = true), training the raw ones
    y_ema = tm.inference(x)
    raw = tm.params.clone()
    assert not torch.equal(tm.params_inference, raw)
    # snapshot: params_binary holds the INFERENCE parameters (trainer.h:448), the optimizer state nests like the reference's
    doc = msgpack.unpackb(tm.serialize(serialize_optimizer=True), raw=False)
    assert doc["params_binary"] == tm.params_inference.cpu().numpy().tobytes()
    opt = doc["optimizer"]
    assert set(opt) == {"nested", "weights_ema_binary"} and set(opt["nested"]) == {"learning_rate", "learning_rate_factor", "nested"}
    assert opt["nested"]["learning_rate_factor"] == 0.25 and opt["nested"]["nested"]["current_step"] == 6
    other = T.create_from_config(3, 4, cfg, seed=5)
    other.deserialize(tm.serialize(serialize_optimizer=True))
    assert torch.equal(other.params_inference, tm.params_inference) and other.optimizer_step_count == 6
    assert torch.equal(other.inference(x), y_ema)
    tm.update_hyperparams({"optimizer": {"decay": 0.5, "nested": {"decay_base": 0.1}}})
    assert tm.hyperparams()["optimizer"]["decay"] == 0.5 and abs(tm.hyperparams()["optimizer"]["nested"]["decay_base"] - 0.1) < 1e-7


def test_bucketed_optimizer_step_equals_the_whole_step():
    """Data-parallel hosts step each gradient bucket as soon as its all-reduce finished (tinycudann.parallel.
    reduce_and_step): stepping [0, n) in ranges gives exactly the parameters of one whole optimizer step."""
    T = tcnn()
    from tinycudann import parallel as par
    cfg = config_hash(log2_hashmap_size=14)
    cfg["optimizer"] = {"otype": "Ema", "decay": 0.9, "nested": cfg["optimizer"]}
    a, b = T.create_from_config(3, 4, cfg, seed=3), T.create_from_config(3, 4, cfg, seed=3)
    pos = positions(2048, 3, seed=6)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(targets_for(pos, 4)).cuda()
    assert par.bucket_ranges(1000, 3) == [(0, 336), (336, 672), (672, 1000)]
    for _ in range(3):
        a.training_step(x, t, want_context=False)
        b.training_step(x, t, run_optimizer=False, want_context=False)
        par.reduce_and_step(b, b.param_gradients, n_buckets=5)
    assert a.optimizer_step_count == b.optimizer_step_count == 3
    assert torch.equal(a.params_full_precision, b.params_full_precision) and torch.equal(a.params, b.params)
    assert torch.equal(a.params_inference, b.params_inference)
    assert torch.equal(a.inference(x), b.inference(x))


def test_deep_network_trains():
    """8 hidden ReLU layers (the reference's FullyFusedMLP has no depth limit; its default is 5): the layer-by-layer
    backward trains, matches forward()+backward(), and the oracle's gradients in distribution."""
    T = tcnn()
    cfg = config_hash(log2_hashmap_size=14, n_hidden_layers=8)
    tm, md = _trainer_and_oracle(cfg, 3, 4)
    w = tm.params_full_precision.cpu().numpy().copy()
    w[md.mlp.n_params:] *= 1.0e3
    tm.set_params_full_precision(torch.from_numpy(w))
    st = O.TrainState(md, w)
    pos = positions(4096, 3, seed=9)
    tgt = targets_for(pos, 4)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    ctx = tm.training_step(x, t, run_optimizer=False)
    loss_ref = O.training_step(st, pos, tgt, run_optimizer=False)
    assert abs(tm.loss(ctx) - loss_ref) <= 5e-3 * abs(loss_ref)
    g, gref = tm.param_gradients.float().cpu().numpy()[:md.mlp.n_params], O.h2f(st.grads)[:md.mlp.n_params]
    assert np.percentile(rae(g, gref), 90) < 1e-2
    losses = [tm.loss(tm.training_step(x, t)) for _ in range(30)]
    assert np.isfinite(losses).all() and losses[-1] < 0.7 * losses[0]


@pytest.mark.parametrize("interp", ["Linear", "Smoothstep"])
def test_grid_second_order_through_c_abi_and_double_backward(interp, binding):
    """backward_backward_input of the grid encoding (grid.h:352-655, 910-1042): the three native outputs against the
    oracle, and torch double backward (an eikonal-style loss on d(encoding)/dx) against torch.autograd.gradcheck-free
    finite differences."""
    C = tcnn()._C
    enc = dict(HASH_ENCODING_SMALL, interpolation=interp)
    d = 3
    m = C.create_encoding(d, enc)
    og = oracle_grid(enc, d)
    n = 2048
    pos = positions(n, d, seed=31)
    rng = np.random.default_rng(5)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    K = m.n_output_dims()
    dy = O.f2h(rng.standard_normal((n, K)).astype(np.float32))
    ddx = (rng.standard_normal((n, d)) * 1e-3).astype(np.float32)  # the finest level's scale is ~7e3: keep fp16 gradients in range
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    dyt = h_t(dy).requires_grad_(True)
    d_dy, d_p, d_x = m.bwd_bwd_input(ctx, x, p, torch.from_numpy(ddx).cuda(), dyt)
    torch.cuda.synchronize()
    _, dydx = O.grid_forward(og, params, pos, want_dy_dx=True)
    gp_ref, dLddy_ref, dx_ref = O.grid_backward_backward_input(og, params, pos, ddx, dy, dy_dx=dydx)
    assert np.array_equal(h_np(d_dy)[:, :og.n_levels * og.n_features_per_level], dLddy_ref[:, :og.n_levels * og.n_features_per_level])
    assert np.allclose(d_x.cpu().numpy(), dx_ref, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(dx_ref).max()))
    mag = np.abs(O.grid_backward_backward_input(og, params, pos, np.abs(ddx), O.f2h(np.abs(O.h2f(dy))))[0]) + np.abs(gp_ref)
    assert np.all(np.abs(d_p.float().cpu().numpy().astype(np.float64) - gp_ref) <= 2.0 ** -8 * mag + 1e-3 * max(1.0, np.abs(gp_ref).max()))

    # torch: loss = sum(|d(sum of features)/dx|^2) -- needs the double backward through the encoding
    coarse = dict(enc, n_levels=4, base_resolution=4, per_level_scale=1.5)  # scales <= 13.5: an eikonal term that fits fp16 with loss scale 128
    tcnn_mod = tcnn().Encoding(d, coarse, dtype=torch.half)
    with torch.no_grad():
        tcnn_mod.params.copy_((torch.rand_like(tcnn_mod.params) - 0.5) * 0.5)
    xt = torch.from_numpy(pos[:512]).cuda().requires_grad_(True)
    feat = tcnn_mod(xt).float().sum()
    (gx,) = torch.autograd.grad(feat, xt, create_graph=True)
    loss = (gx ** 2).sum() * 1e-3  # small enough for the fp16 parameter gradient (x loss scale 128) of the coarsest table
    loss.backward()
    assert torch.isfinite(tcnn_mod.params.grad).all() and float(tcnn_mod.params.grad.abs().max()) > 0
    # finite difference of the loss with respect to a few touched parameters (the loss is quadratic in them)
    g = tcnn_mod.params.grad.float().clone()
    idx = torch.topk(g.abs(), 4).indices.tolist()

    def loss_at(pvec):
        with torch.no_grad():
            tcnn_mod.params.copy_(pvec)
        xq = xt.detach().clone().requires_grad_(True)
        (gq,) = torch.autograd.grad(tcnn_mod(xq).float().sum(), xq, create_graph=False)
        return float((gq.double() ** 2).sum()) * 1e-3

    base = tcnn_mod.params.detach().clone()
    for j in idx:
        step = max(abs(float(base[j])) * 2.0 ** -4, 2.0 ** -6)
        hi, lo = base.clone(), base.clone()
        hi[j] += step
        lo[j] -= step
        fd = (loss_at(hi) - loss_at(lo)) / (float(hi[j]) - float(lo[j]))
        assert abs(fd - float(g[j])) <= 0.1 * abs(float(g[j])) + 1e-3 * float(g.abs().max()), (j, fd, float(g[j]))


def test_grid_second_order_beyond_the_bucket_limits():
    """backward_backward_input for a legal reference configuration the bucketed scatter cannot hold (40 levels > 32 bucketed
    levels): the parameter gradient falls back to the reference's atomic formulation with the second-order corner weight."""
    C = tcnn()._C
    enc = {"otype": "HashGrid", "n_levels": 40, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4, "per_level_scale": 1.1}
    d = 2
    m = C.create_encoding(d, enc)
    og = oracle_grid(enc, d)
    n = 1024
    pos = positions(n, d, seed=3)
    rng = np.random.default_rng(6)
    params = O.f2h((rng.random(og.n_params, dtype=np.float32) * 2 - 1) * 0.5)
    dy = O.f2h(rng.standard_normal((n, m.n_output_dims())).astype(np.float32))
    ddx = (rng.standard_normal((n, d)) * 1e-2).astype(np.float32)
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    p = h_t(params).requires_grad_(True)
    ctx, y = m.fwd(x, p)
    _, d_p, _ = m.bwd_bwd_input(ctx, x, p, torch.from_numpy(ddx).cuda(), h_t(dy).requires_grad_(True))
    gp_ref = O.grid_backward_backward_input(og, params, pos, ddx, dy)[0]
    mag = np.abs(O.grid_backward_backward_input(og, params, pos, np.abs(ddx), O.f2h(np.abs(O.h2f(dy))))[0]) + np.abs(gp_ref)
    assert np.abs(gp_ref).max() > 0
    assert np.all(np.abs(d_p.float().cpu().numpy().astype(np.float64) - gp_ref) <= 2.0 ** -7 * mag + 2e-3 * max(1.0, np.abs(gp_ref).max()))


def test_cpp_sample_learns_an_image(tmp_path):
    """The reference's demo (samples/mlp_learning_an_image.cu: its training loop is spliced from /root/reference into this repository's
    template at build time by oracle/make_image_sample.py and oracle/Makefile; source and binary land in oracle/_ref/ and travel) against the C++ facade:
    2-D hash grid + MLP learn a test card from random pixel lookups drawn by the library's pcg32 kernel; the rendered image reaches a PSNR that
    only a working training path gives."""
    import subprocess
    from oracle import build_ref
    exe = build_ref.IMAGE
    if not os.path.exists(exe):
        build_ref.build(verbose=False)  # builds it where the reference tree is present
    if not os.path.exists(exe):
        pytest.skip("the sample is generated from the reference tree at build time (oracle/make_image_sample.py); neither that tree nor a prebuilt binary is here")
    r = subprocess.run([exe, "-", "-", "300"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    psnr = float(r.stdout.split("psnr=")[1].split()[0])
    assert psnr > 25.0, r.stdout
    assert (tmp_path / "learned_image.ppm").read_bytes().startswith(b"P6\n512 512\n255\n")


@pytest.mark.gpu
@pytest.mark.parametrize("out_dims", [3, 16])
def test_inference_writes_the_callers_matrix_in_every_layout(out_dims):
    """Network::inference (object.h:214-271) into a GPUMatrixDynamic<float> of either layout and any stride (tcnn_network_inference_matrices).
    Where the register-resident inference kernel runs the network it stores the fp32 elements itself instead of a padded 16-bit matrix that
    trim_and_cast would read back: the elements must be bit for bit the cast of the 16-bit outputs the training pass's forward produces,
    in the dense column-major form, row-major, and with padded leading dimensions whose padding stays untouched."""
    import ctypes as C
    T = tcnn()
    tm = T.create_from_config(3, out_dims, config_hash(), seed=1337)
    n = 1024
    pos = positions(n, 3, seed=3)
    x = torch.from_numpy(pos).cuda()
    tgt = torch.zeros((n, out_dims), dtype=torch.float32, device="cuda")
    ctx = tm.training_step(x, tgt, run_optimizer=False)  # its context holds the padded 16-bit prediction of the same parameters
    want = ctx.output[:, :out_dims].float()

    class Matrix(C.Structure):
        _fields_ = [("data", C.c_void_p), ("m", C.c_uint32), ("n", C.c_uint32), ("stride", C.c_uint32), ("layout", C.c_int)]

    lib = T._C._lib
    fn = lib.tcnn_network_inference_matrices
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Matrix), C.POINTER(Matrix), C.c_int]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inp = Matrix(x.data_ptr(), 3, n, 3, 1)  # the batch as the library's callers hold it: column-major n_dims x batch
    dense = tm.inference(x)
    assert torch.equal(dense, want)
    for layout, stride in ((1, out_dims), (1, out_dims + 5), (0, n), (0, n + 24)):
        rows, cols = (n, stride) if layout == 1 else (out_dims, stride)
        buf = torch.full((rows, cols), -7.0, dtype=torch.float32, device="cuda")
        out = Matrix(buf.data_ptr(), out_dims, n, stride, layout)
        assert fn(tm._h, stream, C.byref(inp), C.byref(out), 0) == 0, lib.tcnn_last_error().decode()
        torch.cuda.synchronize()
        got = buf[:, :out_dims] if layout == 1 else buf[:, :n].t()
        assert torch.equal(got, want), (layout, stride)
        pad = buf[:, out_dims:] if layout == 1 else buf[:, n:]
        assert bool((pad == -7.0).all()), (layout, stride)

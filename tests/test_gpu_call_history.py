"""A call's result must not depend on the calls before it (cases, inputs and the CPU-side arithmetic: tests/call_history_cases.py).

The host layer keeps state between calls: the scratch cache recycles blocks per (device, stream) -- up to twice the size asked for, never
cleared --, the bucketed grid backward's queue and overflow counters are cleared once and handed back zeroed by the kernels, a forward
context owns blocks while later calls allocate around it, and the process-wide switches change which kernels run.  Every test here takes a
PROBE -- one fixed call on fixed inputs --
  1. on clean state, right after free_temporary_memory() (which drops every free list and every counter buffer), checked against the
     oracle / the float64 restatement with the bars of the kernel's existing test (test_clean_state_against_the_oracle);
  2. after a HISTORY, a short fixed list of other calls chosen to dirty that state, run once;
  3. and asserts that 2 equals 1 bit for bit.
Bit equality is claimed where the project claims determinism: grid forward, network kernels, losses, input gradients, 16-bit grid parameter
gradients in backward mode 3 (exact owner sums, rounded once), fp32 grid parameter gradients on exact-sum data.  Every probe therefore runs
in mode 3.  The calls of history 5 that run in modes 0 to 2 add packed halves in hardware order: G16's are held to the oracle bar
|got - ref| <= 2^-8 * sum|terms| + 2e-3, NE's to the bar of test_network_with_input_encoding (its reference is the oracle's dL/d(encoding)).

One side stream serves the whole module (torch hands streams out of a pool: a "new" stream is no clean state).  The last test but one
runs this file once more in a child process under TCNN_DEBUG_ALLOC=canary -- exact-size blocks filled with 0xFF on every acquisition, the
complement of history 1 --, the last one verifies the allocator's guards."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import call_history_cases as H
import exact_f32_network_cases as F
import exact_mlp_second_order_cases as X
import exact_network_cases as E
import scatter_owner_cases as K
import second_order_f32_cases as SK
from conftest import HASH_ENCODING_SMALL, MLP_64x2, ROOT, config_hash
from oracle import oracle as O
from test_gpu_parity import _trainer_and_oracle, h_t, oracle_grid, positions, rae, tcnn

pytestmark = pytest.mark.gpu
CHILD_GUARD = "TCNN_CALL_HISTORY_CHILD"
# this file measured 9 s of wall time on an MI355X, interpreter start and the canary child (4.7 s) included: the child's limit is three times that
PLAIN_RUN_SECONDS = 9
CHILD_TIMEOUT = 3 * PLAIN_RUN_SECONDS


def _C():
    return tcnn()._C


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16).numpy().view(np.uint16).copy() if t.element_size() == 2 else t.numpy().view(np.uint32).copy()


def f_t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64).astype(np.float32)).cuda()


class switches:
    """grid backward mode / owner mode for the calls inside, the defaults restored on the way out"""

    def __init__(self, backward=3, owner=None):
        self.backward, self.owner = backward, owner

    def __enter__(self):
        C = _C()
        self.saved = (C.get_grid_backward_mode(), C.get_grid_owner_mode())
        C.set_grid_backward_mode(self.backward)
        if self.owner is not None:
            C.set_grid_owner_mode(self.owner)

    def __exit__(self, *exc):
        C = _C()
        C.set_grid_backward_mode(self.saved[0])
        C.set_grid_owner_mode(self.saved[1])


# ---- probes ----------------------------------------------------------------------------------------------------------------------------
class ModuleProbe:
    """a module of the C ABI with its inputs: fwd() -> state, bwd(state) -> {tensor name: bits}; which = "probe" (the fixed call), "big"
    (n = 4096), "near" (256 rows more than the probe: blocks of at most twice the probe's, which the cache does hand to the probe) or "other"
    (the probe's size, other values)"""
    levels = None  # first value of every level in dL_dparams, for grid probes

    def __init__(self):
        self.cache = {}

    def inputs(self, which="probe"):
        if which not in self.cache:
            self.cache[which] = self.make(which)
        return self.cache[which]

    def fwd(self, which="probe"):
        d = self.inputs(which)
        x, p = d["x"].detach().requires_grad_(True), d["p"].detach().requires_grad_(True)
        ctx, y = self.m.fwd(x, p)
        return d, x, p, ctx, y

    def bwd(self, state, between=None):
        d, x, p, ctx, y = state
        dx, dp = self.m.bwd(ctx, x, p, y, d["dy"])
        torch.cuda.synchronize()
        return {"output": bits(y), "dL_dinput": bits(dx), "dL_dparams": bits(dp)}

    def run(self, which="probe"):
        with switches(backward=3):
            return self.bwd(self.fwd(which))

    def accumulate_into_garbage(self):
        """a GradientMode::Accumulate backward of the probe's inputs into a garbage-filled buffer"""
        C = _C()
        d, x, p, ctx, y = self.fwd()
        garbage = torch.full_like(d["p"], 3.0e4)
        with switches(backward=3):
            self.m.bwd_into(ctx, x, p, y, d["dy"], garbage, C.GradientMode.Accumulate, want_dL_dinput=False)
        torch.cuda.synchronize()


class G16(ModuleProbe):
    name = "G16"

    def __init__(self):
        super().__init__()
        self.m = _C().create_encoding(H.GRID_D, K.encoding_config(H.GRID_TABLE))
        self.og = K.oracle_grid(H.GRID_D, H.GRID_TABLE)
        self.levels = [int(o) * K.F for o in self.og.offsets[:self.og.n_levels + 1]]

    def make(self, which):
        n, seed = {"probe": (H.GRID_N, 3), "big": (H.BIG, 13), "near": (H.GRID_NEAR, 33), "other": (H.GRID_N, 23)}[which]
        og, pos, dy, params = H.grid_half_data(n, seed=seed)
        return {"x": torch.from_numpy(pos).cuda(), "p": h_t(params), "dy": h_t(dy), "host": (pos, dy, params)}


class G32(ModuleProbe):
    name = "G32"

    def __init__(self):
        super().__init__()
        C = _C()
        self.m = C.create_encoding(H.GRID_D, K.encoding_config(H.GRID_TABLE), C.Precision.Fp32)
        self.og = K.oracle_grid(H.GRID_D, H.GRID_TABLE)
        self.levels = [int(o) * K.F for o in self.og.offsets[:self.og.n_levels + 1]]

    def make(self, which):
        n, seed = {"probe": (H.GRID_N, 5), "big": (H.BIG, 15), "near": (H.GRID_NEAR, 35), "other": (H.GRID_N, 25)}[which]
        og, pos, dy, ddx, params = H.grid_exact_data(n, seed=seed)
        return {"x": torch.from_numpy(pos).cuda(), "p": torch.from_numpy(params).cuda(), "dy": torch.from_numpy(dy).cuda(), "ddx": torch.from_numpy(ddx).cuda(),
                "host": (pos, dy, ddx, params)}


class G2(G32):
    """G32's grid, the second-order pass (Linear interpolation)"""
    name = "G2"

    def bwd(self, state, between=None):
        """between: a first-order backward of the context, then between(), then the second-order pass"""
        d, x, p, ctx, y = state
        if between:
            self.m.bwd(ctx, x, p, y, d["dy"])
            between()
        ddy, dp, dx = self.m.bwd_bwd_input(ctx, x, p, d["ddx"], d["dy"].detach().requires_grad_(True))
        torch.cuda.synchronize()
        return {"dL_ddLdoutput": bits(ddy), "dL_dinput": bits(dx), "dL_dparams": bits(dp)}


class NE(ModuleProbe):
    name = "NE"

    def __init__(self):
        super().__init__()
        self.m = _C().create_network_with_input_encoding(3, 4, HASH_ENCODING_SMALL, MLP_64x2)
        self.og = oracle_grid(HASH_ENCODING_SMALL, 3)
        self.md = O.model_init(3, 4, self.og, 64, 2)
        nm = self.md.mlp.n_params
        self.levels = [0] + [nm + int(o) * 2 for o in self.og.offsets[1:self.og.n_levels + 1]]  # (the network's weights count to level 0)
        p32 = self.m.initial_params(1337).cpu().numpy()
        p32[nm:] *= 3.0e3
        self.params = O.f2h(p32)

    def make(self, which):
        n, seed = {"probe": (H.NE_N, 11), "big": (H.BIG, 12), "near": (H.NE_N + 256, 13), "other": (H.NE_N, 14)}[which]
        pos = positions(n, 3, seed=seed)
        dy = np.zeros((n, 16), np.float32)
        dy[:, :4] = np.random.default_rng(seed).standard_normal((n, 4)).astype(np.float32) * 0.05
        dyh = O.f2h(dy)
        return {"x": torch.from_numpy(pos).cuda(), "p": h_t(self.params), "dy": h_t(dyh), "host": (pos, dyh)}


class ExactNetwork(ModuleProbe):
    """W and L16: the dyadic cases of tests/exact_network_cases.py"""

    def __init__(self, name, case):
        super().__init__()
        self.name, self.case = name, case
        self.m = _C().create_network(case.IN, case.OUT, case.network())
        assert self.m.hyperparams()["network"]["otype"] == case.otype

    def make(self, which):
        case = {"probe": self.case, "big": H.other(self.case, H.BIG), "near": H.other(self.case, self.case.n + 256), "other": H.other(self.case)}[which]
        data = E.generate(case)
        to_half = lambda v: torch.from_numpy(E.to_bits(v).view(np.int16)).view(torch.half).cuda()  # noqa: E731
        return {"x": f_t(data.x), "p": to_half(data.params), "dy": to_half(data.dy), "host": (case, data)}


class L32(ModuleProbe):
    """the fp32 network: first- and second-order pass on one context"""
    name = "L32"

    def __init__(self):
        super().__init__()
        C = _C()
        self.case = H.L32_CASE
        self.m = C.create_network_precision(self.case.IN, self.case.OUT, self.case.network(), C.Precision.Fp32)

    def make(self, which):
        case = {"probe": self.case, "big": H.other(self.case, H.BIG), "near": H.other(self.case, self.case.n + 256), "other": H.other(self.case)}[which]
        data = X.generate(case)
        return {"x": f_t(data.x), "p": f_t(data.params), "dy": f_t(data.dy), "v": f_t(data.v), "host": (case, data)}

    def bwd(self, state, between=None):
        d, x, p, ctx, y = state
        dx, dp = self.m.bwd(ctx, x, p, y, d["dy"])
        if between:
            between()
        ddy, dp2, dx2 = self.m.bwd_bwd_input(ctx, x, p, d["v"], d["dy"].detach().requires_grad_(True))
        torch.cuda.synchronize()
        return {"output": bits(y), "dL_dinput": bits(dx), "dL_dparams": bits(dp), "second order dL_ddLdoutput": bits(ddy),
                "second order dL_dparams": bits(dp2), "second order dL_dinput": bits(dx2)}


class Trainer:
    """T: create_from_config(config_hash(log2_hashmap_size=15)), training_step(run_optimizer=False), n = 1024"""
    name = "T"

    def __init__(self):
        self.cfg = config_hash(log2_hashmap_size=15)
        self.tm, self.md = _trainer_and_oracle(self.cfg, 3, 4)
        self.og = oracle_grid(self.cfg["encoding"], 3)
        self.nm = self.md.mlp.n_params
        self.init = self.tm.params_full_precision.cpu().numpy().copy()
        self.init[self.nm:] *= 1.0e3
        self.tm.set_params_full_precision(torch.from_numpy(self.init))
        self.grid_levels = [int(o) * 2 for o in self.og.offsets[:self.og.n_levels + 1]]
        self.cache = {}

    def batch(self, n=H.TRAINER_N):
        if n not in self.cache:
            pos, tgt = H.trainer_batch(n)
            self.cache[n] = (torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda(), pos, tgt)
        return self.cache[n]

    def step(self, x, t, tm=None):
        tm = tm or self.tm
        with switches(backward=3):
            ctx = tm.training_step(x, t, run_optimizer=False)
            loss = tm.loss(ctx)
        torch.cuda.current_stream().synchronize()
        g = bits(tm.param_gradients)
        return {"output": bits(ctx.output), "dL_doutput": bits(ctx.dL_doutput), "network gradients": g[:self.nm], "grid gradients": g[self.nm:],
                "loss": np.array([loss], np.float32).view(np.uint32)}

    def run(self, n=H.TRAINER_N):
        x, t = self.batch(n)[:2]
        return self.step(x, t)


PROBES = {"G16": G16, "G32": G32, "G2": G2, "NE": NE, "W": lambda: ExactNetwork("W", H.W_CASE), "L16": lambda: ExactNetwork("L16", H.L16_CASE),
          "L32": L32, "T": Trainer}
MODULE_PROBES = ["G16", "G32", "G2", "NE", "W", "L16", "L32"]


@pytest.fixture(scope="module")
def probes():
    """every probe once per module: its module, its inputs on the GPU and its result on CLEAN state, shared and left unchanged"""
    class Made:
        def __init__(self):
            self.made, self.extra = {}, {}

        def __call__(self, name):
            if name not in self.made:
                probe = PROBES[name]()
                _C().free_temporary_memory()
                self.made[name] = (probe, probe.run())
            return self.made[name]
    return Made()


@pytest.fixture(scope="module")
def side_stream():
    return torch.cuda.Stream()


def levels_of(probe, name):
    if isinstance(probe, Trainer):
        return probe.grid_levels if name == "grid gradients" else None
    return probe.levels if name == "dL_dparams" else None


def same_bits(history, probe, got, want):
    report = [H.difference(history, probe.name, name, got[name], want[name], levels_of(probe, name)) for name in want]
    assert not any(report), "\n".join(r for r in report if r)


# ---- the clean results against the oracle ----------------------------------------------------------------------------------------------
def _check_G16(p, clean):
    pos, dy, params = p.inputs()["host"]
    n = H.GRID_N
    same_bits("none: against the oracle's bits", p, {"output": clean["output"]}, {"output": O.grid_forward(p.og, params, pos)})
    got = O.h2f(clean["dL_dparams"]).astype(np.float64)
    ref = O.grid_backward(p.og, pos[:n], dy[:n])
    absacc = O.grid_backward(p.og, pos[:n], O.f2h(np.abs(O.h2f(dy[:n]))))
    assert np.all(np.abs(got - ref) <= absacc * 2.0 ** -8 + 1e-3) and got.any()  # test_bucketed_backward_bits
    with switches(backward=3, owner=2):  # ... and bit for bit the wide owner form
        wide = p.bwd(p.fwd())
    same_bits("owner mode 2 on the same records", p, {"dL_dparams": wide["dL_dparams"]}, {"dL_dparams": clean["dL_dparams"]})
    _, dy_dx = O.grid_forward(p.og, params, pos, want_dy_dx=True)
    dref = O.grid_backward_input(p.og, dy, dy_dx)
    assert np.allclose(clean["dL_dinput"].view(np.float32), dref, rtol=1e-4, atol=1e-3 * np.abs(dref).max())  # test_grid_backward_and_input_gradient


def _check_G32(p, clean):
    pos, dy, ddx, params = p.inputs()["host"]
    unit, figure, _ = H.exact_grid_sums(p.og, pos, dy)
    assert figure < 2.0 ** 24
    out, dy_dx = O.grid_forward_f32(p.og, params, pos, want_dy_dx=True)
    want = O.grid_backward_f32(p.og, pos, dy)  # float64 sums of terms whose every partial sum is an fp32 number: no rounding anywhere
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    as_bits = lambda v: (np.ascontiguousarray(v, np.float32) + np.float32(0.0)).view(np.uint32)  # noqa: E731  (values: -0 counts as +0)
    want = {"output": as_bits(out), "dL_dinput": as_bits(O.grid_backward_input_f32(p.og, dy, dy_dx)), "dL_dparams": as_bits(want)}
    same_bits("none: against the oracle's values", p, {k: as_bits(clean[k].view(np.float32)) for k in want}, want)
    assert clean["dL_dparams"].any()


def _check_G2(p, clean):
    pos, dy, ddx, params = p.inputs()["host"]
    ref = H.second_order_reference(p.og, pos, dy, ddx, params)
    assert H.exact_second_order_sums(p.og, ref) < 2.0 ** 24
    d_p, d_y, d_x = (clean[k].view(np.float32) for k in ("dL_dparams", "dL_ddLdoutput", "dL_dinput"))
    r = SK.ratios(p.og, ref, d_p, d_y, None)  # the bars of tests/second_order_f32_cases.py; K_x at this grid's 8 levels
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(d_x.astype(np.float64) - ref.dL_dinput)
        r["dL_dinput"] = float(np.max(np.where(err == 0, 0.0, err / (H.k_x(p.og) * SK.U * ref.mag_x))))
    print(f"G2 max |got - ref| / bar: {r}")
    assert np.abs(ref.dL_dparams).max() > 0 and np.abs(ref.dL_dinput).max() > 0 and np.abs(ref.dL_ddLdoutput).max() > 0
    assert not d_p[ref.hits == 0].any() and not d_y[:, p.og.n_levels * K.F:].any()
    assert all(v <= 1.0 for v in r.values()), r


def _ne_bars(p, result, grid_only=False):
    """test_network_with_input_encoding's bars"""
    pos, dyh = p.inputs()["host"]
    md, nm = p.md, p.md.mlp.n_params
    if not hasattr(p, "reference"):
        enc_ref = O.grid_forward(p.og, p.params[nm:], pos, out_stride=md.mlp.in_width)
        hid_ref, out_ref = O.mlp_forward(md.mlp, p.params[:nm], enc_ref)
        gref, denc = O.mlp_backward(md.mlp, p.params[:nm], enc_ref, hid_ref, out_ref, dyh)
        p.reference = (out_ref, gref, O.grid_backward(p.og, pos, denc), O.grid_backward(p.og, pos, O.f2h(np.abs(O.h2f(denc)))))
    out_ref, gref, ggrid, absacc = p.reference
    g = O.h2f(result["dL_dparams"])
    assert np.all(np.abs(g[nm:] - ggrid) <= absacc * 2.0 ** -7 + 1e-3 * np.abs(ggrid).max())
    if grid_only:
        return
    assert np.percentile(rae(O.h2f(result["output"]), O.h2f(out_ref)), 99) < 3e-3
    assert np.percentile(rae(g[:nm], gref), 99) < 3e-3
    dx = result["dL_dinput"].view(np.float32)
    assert np.isfinite(dx).all() and dx.any()


def _check_exact_network(p, clean):
    case, data = p.inputs()["host"]
    res = E.restate(case, data)
    want = {"output": E.to_bits(res.out), "dL_dinput": np.ascontiguousarray(res.dinput).astype(np.float32).view(np.uint32), "dL_dparams": E.to_bits(res.grads)}
    same_bits("none: against the float64 restatement", p, clean, want)


def _check_L32(p, clean):
    case, data = p.inputs()["host"]
    first, second = F.restate(case, data), X.restate(case, data)
    want = {"output": F.bits32(first.out), "dL_dinput": F.bits32(first.dinput), "dL_dparams": F.bits32(first.grads),
            "second order dL_ddLdoutput": X.bits32(second.ddy), "second order dL_dparams": X.bits32(second.grads)}
    same_bits("none: against the float64 restatement", p, {k: clean[k] for k in want}, want)
    assert not clean["second order dL_dinput"].any(), "dL/dinput of a network without curvature is +0 everywhere"


def _check_T(p, clean):
    """test_training_step_matches_oracle's bars for the step without the optimizer"""
    _, _, pos, tgt = p.batch()
    st = O.TrainState(p.md, p.init)
    loss_ref, pred_ref = O.training_step(st, pos, tgt, run_optimizer=False, want_prediction=True)
    loss = float(clean["loss"].view(np.float32)[0])
    assert abs(loss - loss_ref) <= 2e-3 * abs(loss_ref)
    assert np.percentile(rae(O.h2f(clean["output"]), O.h2f(pred_ref)), 99) < 3e-3
    _, g_ref = O.loss(p.md.loss_type, clean["output"], tgt, 4)
    assert np.array_equal(clean["dL_doutput"], g_ref)
    gref = O.h2f(st.grads)
    nm = p.nm
    assert np.percentile(rae(O.h2f(clean["network gradients"]), gref[:nm]), 99) < 5e-3
    big = np.abs(gref[nm:]) > 1e-2 * np.abs(gref[nm:]).max()
    assert np.percentile(rae(O.h2f(clean["grid gradients"])[big], gref[nm:][big]), 99) < 3e-2


CHECKS = {"G16": _check_G16, "G32": _check_G32, "G2": _check_G2, "NE": _ne_bars, "W": _check_exact_network, "L16": _check_exact_network,
          "L32": _check_L32, "T": _check_T}


@pytest.mark.parametrize("name", list(PROBES))
def test_clean_state_against_the_oracle(probes, name):
    probe, clean = probes(name)
    CHECKS[name](probe, clean)


# ---- histories -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PROBES))
def test_big_then_small(probes, name):
    """history 1: the same module at n = 4096 and at 256 rows more than the probe, then the probe.  The cache serves a request from a block
    of up to TWICE its size: the blocks that scale with the batch are recycled from the second call (at most twice the probe's), the
    batch-independent ones (weight-gradient slabs at their cap, transposed weights) from the first -- every block of the probe is a
    recycled, larger, dirty one"""
    probe, clean = probes(name)
    _C().free_temporary_memory()
    for which in ("big", "near"):
        probe.run({"big": H.BIG, "near": H.TRAINER_N + 256}[which]) if name == "T" else probe.run(which)
    same_bits("1 big then small", probe, probe.run(), clean)


def test_batch_size_ladder_through_the_trainer(probes):
    """history 2, default stream: n = 256, 4096, 1024, 4096, 1024 -- every repeat of a size equals the first run of that size"""
    probe, clean = probes("T")
    _C().free_temporary_memory()
    first = {}
    with switches(backward=3):
        for i, n in enumerate(H.LADDER):
            got = probe.run(n)
            if n == H.TRAINER_N:
                same_bits(f"2 ladder, rung {i} (n = {n}) against the clean run", probe, got, clean)
            if n in first:
                same_bits(f"2 ladder, rung {i} (n = {n}) against the first run of the size", probe, got, first[n])
            first.setdefault(n, got)


def test_batch_size_ladder_as_graph_launches(probes, side_stream):
    """history 2 on a side stream with set_graph_capture(True).  The library launches a graph only for a step whose shape equals the step
    before it (the first step of a shape runs plainly and fills the stream's scratch cache, another shape forgets the graph), so every rung
    from the third on is taken twice in a row: once plainly, once as a graph launch -- which must leave the bits of the plain first run of
    that size in the deterministic parts (prediction, loss gradient, network gradients, mode-3 grid gradients)."""
    probe, clean = probes("T")
    _C().free_temporary_memory()
    tm = probe.tm
    first, launched = {}, tm.graph_capture_stats()[0]
    tm.set_graph_capture(True)
    try:
        with torch.cuda.stream(side_stream), switches(backward=3):  # (one mode throughout: nothing but the batch size changes between steps)
            for i, n in enumerate(H.LADDER):
                for take in range(1 if i < 2 else 2):
                    got = probe.run(n)
                    if n == H.TRAINER_N:
                        same_bits(f"2 ladder under graph capture, rung {i} take {take} (n = {n}) against the clean run", probe, got, clean)
                    if n in first:
                        same_bits(f"2 ladder under graph capture, rung {i} take {take} (n = {n}) against the first run of the size", probe, got, first[n])
                    first.setdefault(n, got)
    finally:
        tm.set_graph_capture(False)
        torch.cuda.synchronize()
    assert tm.graph_capture_stats()[0] - launched == 3, "the second take of rungs 2, 3 and 4 is a graph launch each"


def _other_plan(probes):
    """the mode-3 backward of the "dense" table at D = 2 (3 levels, one queue each: another counter layout) and its result on clean state"""
    key = "other plan"
    made = probes.extra
    if key not in made:
        c = H.OTHER_PLAN
        og, pos, dy, params = H.grid_half_data(c["n"], c["D"], c["table"])
        p = G16.__new__(G16)
        ModuleProbe.__init__(p)
        p.name, p.og = "dense table at D = 2", og
        p.m = _C().create_encoding(c["D"], K.encoding_config(c["table"]))
        p.levels = [int(o) * K.F for o in og.offsets[:og.n_levels + 1]]
        p.cache["probe"] = {"x": torch.from_numpy(pos).cuda(), "p": h_t(params), "dy": h_t(dy), "host": (pos, dy, params)}
        _C().free_temporary_memory()
        made[key] = (p, p.run())
    return made[key]


@pytest.mark.parametrize("order", ["before", "after"])
@pytest.mark.parametrize("name", ["G16", "NE", "T"])
def test_another_plan_in_between(probes, name, order):
    """history 3: a bucketed backward with another queue count and another overflow-counter index shares the stream's counter buffer and
    queue block with the probe's.  "before": the other plan, then the probe.  "after": the probe on clean state, then the other plan -- which
    must give ITS clean bits on what the probe's plan left behind -- and the probe once more."""
    probe, clean = probes(name)
    other, other_clean = _other_plan(probes)
    _C().free_temporary_memory()
    if order == "before":
        same_bits("3 another plan before, the other plan itself on clean state", other, other.run(), other_clean)
        same_bits("3 another plan before", probe, probe.run(), clean)
    else:
        same_bits("3 another plan after, the probe on clean state", probe, probe.run(), clean)
        same_bits("3 another plan after, the other plan", other, other.run(), other_clean)
        same_bits("3 another plan after, the probe again", probe, probe.run(), clean)


def _grow_plan(probes):
    """a grid whose bucketed plan needs more counters than the smallest counter buffer holds (call_history_cases.GROW_PLAN; the arithmetic is
    asserted in tests/test_call_history_cases.py): module and inputs, made once -> run(), one mode-3 backward, held to the scatter's
    conservation property with the bar of test_grid_forward_full_size_bit_exact_and_checksum"""
    made = probes.extra
    if "grow plan" not in made:
        c = H.GROW_PLAN
        og = H.grow_plan_grid()
        assert H.n_counters(og) > H.COUNTER_BUFFER_FLOOR
        m = _C().create_encoding(c["D"], H.grow_plan_config())
        assert m.n_params() == og.n_params
        x = torch.from_numpy(H.positions(c["n"], c["D"], seed=77)).cuda()
        p = torch.zeros(og.n_params, dtype=torch.half, device="cuda").requires_grad_(True)
        dy = h_t(K.make_dy(c["n"], og.n_levels * K.F, seed=78))
        offsets = [int(o) for o in og.offsets[:og.n_levels + 1]]

        def run():
            with switches(backward=3):
                ctx, y = m.fwd(x, p)
                _, dp = m.bwd(ctx, x, p, y, dy)
            torch.cuda.synchronize()
            got = dp.float().view(-1, K.F)
            sums = torch.stack([got[offsets[l]:offsets[l + 1]].double().sum(0) for l in range(og.n_levels)]).cpu().numpy()
            ref = dy.double().sum(0).view(og.n_levels, K.F).cpu().numpy()
            scale = dy.abs().double().sum(0).view(og.n_levels, K.F).cpu().numpy()
            assert np.all(np.abs(sums - ref) <= scale * 2.0 ** -8 + 1e-2) and np.abs(sums).max() > 0, "the grow plan's own gradients do not conserve dL/dy"
        made["grow plan"] = run
    return made["grow plan"]


@pytest.mark.parametrize("order", ["grown after", "grown before"])
@pytest.mark.parametrize("name", ["G16", "T"])
def test_counter_buffer_grown_in_between(probes, name, order):
    """history 3, the counter buffer regrown: the probe's plan and the dense plan need fewer counters than the smallest buffer (4096), the grow
    plan needs 4610.  "grown after": the probe on clean state allocates the smallest buffer, the grow plan makes ZeroedCounters::get free it
    and allocate a larger one, then the probe and the dense plan run on that one.  "grown before": the grow plan first, on clean state, so
    that the probe and the dense plan meet a buffer and queue blocks laid out by 4096 queues."""
    probe, clean = probes(name)
    other, other_clean = _other_plan(probes)
    grow = _grow_plan(probes)
    _C().free_temporary_memory()
    if order == "grown after":
        same_bits("3 counter buffer grown after, the probe on clean state", probe, probe.run(), clean)
    grow()
    same_bits(f"3 counter buffer {order}, the probe", probe, probe.run(), clean)
    same_bits(f"3 counter buffer {order}, the dense plan", other, other.run(), other_clean)
    same_bits(f"3 counter buffer {order}, the probe again", probe, probe.run(), clean)


@pytest.mark.parametrize("name", ["G16", "T"])
def test_overflow_before(probes, name):
    """history 4: a batch that provably sends pairs through the overflow list (asserted from the plan arithmetic before anything is launched)"""
    probe, clean = probes(name)
    og, pos, dy, params, spilled = H.overflow_case()
    assert spilled > 0
    m = _C().create_encoding(H.OVERFLOW["D"], K.encoding_config(H.OVERFLOW["table"]))
    x, p = torch.from_numpy(pos).cuda(), h_t(params).requires_grad_(True)
    _C().free_temporary_memory()
    with switches(backward=3):
        ctx, y = m.fwd(x, p)
        _, dp = m.bwd(ctx, x, p, y, h_t(dy))
    torch.cuda.synchronize()
    assert bits(dp).any()
    same_bits(f"4 overflow before ({spilled} pairs past their queue)", probe, probe.run(), clean)


@pytest.mark.parametrize("name", ["G16", "NE"])
def test_other_modes_before(probes, name):
    """history 5: the probe's own inputs through backward modes 0, 1, 2 and owner modes 0 / 2, then the mode-3 probe"""
    probe, clean = probes(name)
    C = _C()
    defaults = (C.get_grid_backward_mode(), C.get_grid_owner_mode())
    _C().free_temporary_memory()
    try:
        for mode in (0, 1, 2):
            with switches(backward=mode):
                got = probe.bwd(probe.fwd())
            same_bits(f"5 other modes before, mode {mode}: the parts that do not depend on the mode", probe,
                      {k: got[k] for k in ("output", "dL_dinput")}, {k: clean[k] for k in ("output", "dL_dinput")})
            if name == "G16":  # packed halves added in hardware order: the oracle bar
                pos, dy, params = probe.inputs()["host"]
                if not hasattr(probe, "sums"):
                    probe.sums = (O.grid_backward(probe.og, pos, dy), O.grid_backward(probe.og, pos, O.f2h(np.abs(O.h2f(dy)))))
                ref, absacc = probe.sums
                assert np.all(np.abs(O.h2f(got["dL_dparams"]).astype(np.float64) - ref) <= absacc * 2.0 ** -8 + 2e-3), f"history 5, probe G16, mode {mode}"
            else:
                _ne_bars(probe, got, grid_only=True)
        for owner in (0, 2):
            with switches(backward=3, owner=owner):
                same_bits(f"5 other modes before, owner mode {owner}", probe, probe.bwd(probe.fwd()), clean)
        assert (C.get_grid_backward_mode(), C.get_grid_owner_mode()) == defaults
        same_bits("5 other modes before", probe, probe.run(), clean)
    finally:
        C.set_grid_backward_mode(defaults[0])
        C.set_grid_owner_mode(defaults[1])


@pytest.mark.parametrize("name", ["G16", "T"])
def test_all_zero_gradient_before(probes, name):
    """history 6: an all-zero dL/dy queues nothing (the zero-record drop path), then the probe.  The trainer's zero gradient comes from
    targets equal to its own prediction."""
    probe, clean = probes(name)
    _C().free_temporary_memory()
    if name == "G16":
        d, x, p, ctx, y = probe.fwd()
        with switches(backward=3):
            _, dp = probe.m.bwd(ctx, x, p, y, torch.zeros_like(d["dy"]))
        torch.cuda.synchronize()
        assert not bits(dp).any()
    else:
        x = probe.batch()[0]
        t = torch.from_numpy(O.h2f(clean["output"])[:, :4].astype(np.float32)).cuda().contiguous()
        got = probe.step(x, t)
        assert not (got["dL_doutput"] & 0x7FFF).any() and not (got["grid gradients"] & 0x7FFF).any()
    same_bits("6 all-zero dL/dy before", probe, probe.run(), clean)


@pytest.mark.parametrize("name", ["G16", "T"])
def test_max_level_before(probes, name):
    """history 7: a backward with max_level 0.25, one with a per-sample max_level array, then max_level 1.0 and the probe"""
    probe, clean = probes(name)
    _C().free_temporary_memory()
    n = H.GRID_PADDED if name == "G16" else H.TRAINER_N
    per_sample = torch.from_numpy(np.tile(np.array([0.25, 0.625, 1.0], np.float32), n // 3 + 1)[:n].copy()).cuda()
    if name == "G16":
        m = probe.m
        try:
            m.set_max_level(0.25)
            low = probe.run()
            m.set_max_level(1.0)
            m.set_max_level_gpu(per_sample)
            probe.run()
        finally:
            m.set_max_level_gpu(None)
            m.set_max_level(1.0)
        assert not np.array_equal(low["dL_dparams"], clean["dL_dparams"])  # (levels were off)
    else:
        tm = probe.tm
        try:
            tm.max_level = 0.25
            low = probe.run()
            tm.max_level = 1.0
            tm.set_max_level_gpu(per_sample)
            probe.run()
        finally:
            tm.set_max_level_gpu(None)
            tm.max_level = 1.0
        assert not np.array_equal(low["grid gradients"], clean["grid gradients"])
    same_bits("7 max_level before", probe, probe.run(), clean)


@pytest.mark.parametrize("name", ["G16", "L16", "L32"])
def test_accumulate_before(probes, name):
    """history 8: a GradientMode::Accumulate backward into a garbage-filled buffer, then the overwrite probe"""
    probe, clean = probes(name)
    _C().free_temporary_memory()
    probe.accumulate_into_garbage()
    same_bits("8 accumulate before", probe, probe.run(), clean)


def _clean_other(probes, name):
    """the clean result of the probe's module on its "other" inputs"""
    made = probes.extra
    if ("other", name) not in made:
        probe, _ = probes(name)
        _C().free_temporary_memory()
        made[("other", name)] = probe.run("other")
    return made[("other", name)]


@pytest.mark.parametrize("name", ["G16", "L16"])
def test_contexts_of_one_module_out_of_order(probes, name):
    """history 9: fwd(x1), fwd(x2), bwd(ctx2), bwd(ctx1) -- each backward equals its own clean result"""
    probe, clean = probes(name)
    clean_other = _clean_other(probes, name)
    _C().free_temporary_memory()
    with switches(backward=3):
        s1 = probe.fwd("probe")
        s2 = probe.fwd("other")
        got2 = probe.bwd(s2)
        got1 = probe.bwd(s1)
    same_bits("9 contexts out of order, the second context's backward", probe, got2, clean_other)
    same_bits("9 contexts out of order, the first context's backward", probe, got1, clean)


def test_contexts_of_two_modules_interleaved(probes):
    """history 9, two modules: fwd A, fwd B, bwd A, bwd B"""
    (a, clean_a), (b, clean_b) = probes("G16"), probes("L16")
    _C().free_temporary_memory()
    with switches(backward=3):
        sa = a.fwd()
        sb = b.fwd()
        got_a = a.bwd(sa)
        got_b = b.bwd(sb)
    same_bits("9 two modules interleaved", a, got_a, clean_a)
    same_bits("9 two modules interleaved", b, got_b, clean_b)


@pytest.mark.parametrize("name", MODULE_PROBES)
def test_free_temporary_memory_between_forward_and_backward(probes, name):
    """history 10: the context's blocks stay owned, the free lists and the counters are gone"""
    probe, clean = probes(name)
    probe.run("big")  # (so that there are free lists and counters to drop)
    with switches(backward=3):
        state = probe.fwd()
        _C().free_temporary_memory()
        got = probe.bwd(state)
    same_bits("10 free_temporary_memory() between forward and backward", probe, got, clean)


@pytest.mark.parametrize("name", ["L32", "G2"])
def test_free_temporary_memory_between_the_first_and_the_second_order_pass(probes, name):
    """history 10 on one context: forward, first-order backward, free_temporary_memory(), second-order pass"""
    probe, clean = probes(name)
    probe.run("big")
    state = probe.fwd()
    with switches(backward=3):
        got = probe.bwd(state, between=_C().free_temporary_memory)
    same_bits("10 free_temporary_memory() between the first- and the second-order pass", probe, got, clean)


@pytest.mark.parametrize("name", list(PROBES))
def test_another_stream(probes, side_stream, name):
    """history 11: default stream, side stream, default stream again, synchronised in between: three equal results"""
    probe, clean = probes(name)
    _C().free_temporary_memory()
    same_bits("11 another stream, default stream first", probe, probe.run(), clean)
    torch.cuda.synchronize()
    with torch.cuda.stream(side_stream):
        got = probe.run()
        side_stream.synchronize()
    torch.cuda.synchronize()
    same_bits("11 another stream, side stream", probe, got, clean)
    same_bits("11 another stream, default stream again", probe, probe.run(), clean)


def test_level_groups_over_one_workspace(probes):
    """history 12: with the gradient-ready hook the grid backward runs per group of levels over one shared workspace and one counter
    buffer: the same gradient bits as the ungrouped pass on identical parameters and batch"""
    probe, clean = probes("T")
    tm, _ = _trainer_and_oracle(probe.cfg, 3, 4)
    tm.set_params_full_precision(torch.from_numpy(probe.init))
    x, t = probe.batch()[:2]
    _C().free_temporary_memory()
    for n_groups in (3, 16):
        ranges = []
        tm.set_backward_level_groups(n_groups)
        tm.set_gradient_ready_callback(lambda b, e: ranges.append((b, e)))
        try:
            got = probe.step(x, t, tm=tm)
        finally:
            tm.set_gradient_ready_callback(None)
        assert len(ranges) > 2 and ranges[0] == (0, probe.nm) and ranges[-1][1] == tm.n_params, ranges
        same_bits(f"12 level groups ({n_groups} asked for, {len(ranges) - 1} made)", probe, got, clean)


# ---- the same file under the canary allocator ------------------------------------------------------------------------------------------
def test_this_file_under_the_canary_allocator():
    """one child process with TCNN_DEBUG_ALLOC=canary: exact-size blocks, filled with 0xFF (NaN) on every acquisition, guards verified by the
    file's last test.  A probe that reads scratch it did not write turns into NaN bits and fails its bit comparison there."""
    if os.environ.get(CHILD_GUARD) or _C().debug_alloc_mode() != 0:
        return  # this IS the child (or the parent already runs a checking allocator): no grandchild
    env = dict(os.environ, TCNN_DEBUG_ALLOC="canary")
    env[CHILD_GUARD] = "1"
    start = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True)
    print(f"canary child: exit status {r.returncode}, {time.time() - start:.1f} s")
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]


def test_allocations_were_not_overrun():
    """the last test of the file: under a checking allocator, every block's guards are intact after everything above"""
    if os.environ.get(CHILD_GUARD):
        assert _C().debug_alloc_mode() == 1, "the child does not run the canary allocator"
    _C().debug_check_allocations()

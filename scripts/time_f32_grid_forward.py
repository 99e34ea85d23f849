"""A/B timing of the fp32 grid forward (tcnn_set_fp32_grid_forward): the forward call of a bare fp32 grid encoding, without dy_dx (an
inference call) and with it (the input requires a gradient), with the tiled gather on and off in one run.

Protocol (one MI355X, HIP events): both settings give the same bits at the timed size (features, and the dL_dinput a backward call forms
from dy_dx; asserted first), 10 warm-up calls of every arm, then 7 blocks of 100 calls per arm, alternating arm by arm inside each
block; per arm the median block with minimum and maximum, in ms per call.  Shapes: the headline grid (16 levels x 2 features, T = 2^19,
base 16, per_level_scale 2.0, D = 3) and data/config_hash.json's grid as shipped (T = 2^15, per_level_scale 1.5, D = 2), 2^18 samples.
A form counts as faster where the two arms' [min, max] ranges do not overlap.

    python scripts/time_f32_grid_forward.py [--out profiles/f32_grid_forward_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tiny-cuda-nn_amd"))
import tinycudann  # noqa: E402

C = tinycudann._C
N, BLOCKS, CALLS, WARMUP = 1 << 18, 7, 100, 10
SHAPES = {"headline_T19_D3": (3, 19, 2.0), "config_hash_T15_D2": (2, 15, 1.5)}


def arm(m, x, p, dy_dx, tiled):
    x = x.clone().requires_grad_(dy_dx)

    def block(calls):
        C.set_fp32_grid_forward(tiled)
        assert m.fp32_grid_forward(N) == int(tiled)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            m.fwd(x, p)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls
    return block


def same_bits(m, x, p, dy):
    got = []
    for tiled in (True, False):
        C.set_fp32_grid_forward(tiled)
        xg = x.clone().requires_grad_(True)
        ctx, y = m.fwd(xg, p)
        got.append((y, m.bwd(ctx, xg, p, y, dy)[0], m.fwd(x, p)[1]))
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*got))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "f32_grid_forward_timing.json"))
    args = ap.parse_args()
    result = {"protocol": __doc__.split("Protocol")[1].split("\n\n")[0].strip(" ():\n"), "ms_per_call": {}, "faster": {}}
    try:
        for name, (d, log2_t, scale) in SHAPES.items():
            cfg = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": log2_t, "base_resolution": 16, "per_level_scale": scale}
            m = C.create_encoding(d, cfg, C.Precision.Fp32)
            rng = np.random.default_rng(1)
            x = torch.from_numpy(rng.random((N, d), dtype=np.float32)).cuda()
            p = torch.from_numpy(rng.uniform(-0.5, 0.5, m.n_params()).astype(np.float32)).cuda()
            dy = torch.from_numpy(rng.standard_normal((N, m.n_output_dims())).astype(np.float32)).cuda()
            assert same_bits(m, x, p, dy), name
            arms = {f"{form}_{kernel}": arm(m, x, p, form == "with_dy_dx", kernel == "tiled") for form in ("features_only", "with_dy_dx") for kernel in ("tiled", "reference")}
            for block in arms.values():
                block(WARMUP)
            times = {k: [] for k in arms}
            for _ in range(BLOCKS):
                for k, block in arms.items():
                    times[k].append(block(CALLS))
            result["ms_per_call"][name] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
            result["faster"][name] = {form: max(times[form + "_tiled"]) < min(times[form + "_reference"]) for form in ("features_only", "with_dy_dx")}
            print(name, json.dumps(result["ms_per_call"][name]), json.dumps(result["faster"][name]), flush=True)
    finally:
        C.set_fp32_grid_forward(True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

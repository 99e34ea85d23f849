"""A/B timing of the fp32 grid backward (tcnn_set_fp32_grid_backward): the backward call of a bare fp32 grid encoding, parameter gradients
only, with the owner pass on and off, and the 16-bit bucketed backward of the same grid next to them, in one run.

Protocol (one MI355X, HIP events): 10 warm-up calls of every arm, then 7 blocks of 20 calls per arm, alternating arm by arm inside each
block; per arm the median block with minimum and maximum, in ms per call.  Shapes: the headline grid (16 levels x 2 features, T = 2^19,
base 16, per_level_scale 2.0, D = 3) and data/config_hash.json's grid as shipped (T = 2^15, per_level_scale 1.5, D = 2), 2^18 samples.

    python scripts/time_f32_grid_backward.py [--out profiles/f32_grid_backward_timing.json]
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
N, BLOCKS, CALLS, WARMUP = 1 << 18, 7, 20, 10
SHAPES = {"headline_T19_D3": (3, 19, 2.0), "config_hash_T15_D2": (2, 15, 1.5)}


def arm(d, cfg, fp32, owner_pass):
    m = C.create_encoding(d, cfg, *([C.Precision.Fp32] if fp32 else []))
    dtype = torch.float32 if fp32 else (torch.bfloat16 if os.environ.get("TCNN_PRECISION") == "bf16" else torch.half)
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.random((N, d), dtype=np.float32)).cuda()
    p = torch.from_numpy(rng.uniform(-0.5, 0.5, m.n_params()).astype(np.float32)).cuda().to(dtype).requires_grad_(True)
    dy = torch.from_numpy(rng.standard_normal((N, m.n_output_dims())).astype(np.float32)).cuda().to(dtype)
    ctx, y = m.fwd(x, p)

    def block(calls):
        C.set_fp32_grid_backward(owner_pass)
        assert m.fp32_grid_backward(N) == int(fp32 and owner_pass)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            m.bwd(ctx, x, p, y, dy)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls
    return block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "f32_grid_backward_timing.json"))
    args = ap.parse_args()
    result = {"protocol": __doc__.split("Protocol")[1].split("\n\n")[0].strip(" ():\n"), "ms_per_call": {}}
    try:
        for name, (d, log2_t, scale) in SHAPES.items():
            cfg = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": log2_t, "base_resolution": 16, "per_level_scale": scale}
            arms = {"fp32_owner_pass": arm(d, cfg, True, True), "fp32_atomic": arm(d, cfg, True, False), "half_bucketed": arm(d, cfg, False, True)}
            for block in arms.values():
                block(WARMUP)
            times = {k: [] for k in arms}
            for _ in range(BLOCKS):
                for k, block in arms.items():
                    times[k].append(block(CALLS))
            result["ms_per_call"][name] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
            print(name, json.dumps(result["ms_per_call"][name]), flush=True)
    finally:
        C.set_fp32_grid_backward(True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

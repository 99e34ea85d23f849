"""A/B timing of the second-order pass of a bare fp32 grid encoding (tcnn_set_fp32_grid_second_order): the bwd_bwd_input call with only
dL_dparams (mask 1 against 0), with only dL_dinput (mask 2 against 0) and with all three results (the default, mask 1, and mask 3 against 0),
in one run.  Mask 0 is the atomic scatter behind a memset of the table and one thread per sample walking the levels.

Protocol (one MI355X, HIP events): 10 warm-up calls of every arm, then 7 blocks of 20 calls per arm, alternating arm by arm inside each
block; per arm the median block with minimum and maximum, in ms per call.  Shapes: the headline grid (16 levels x 2 features, T = 2^19,
base 16, per_level_scale 2.0, D = 3) and data/config_hash.json's grid as shipped (T = 2^15, per_level_scale 1.5, D = 2), 2^18 samples.
Before the timing, per shape: the results of mask 3 and mask 0 on the timed inputs are compared (dL_dinput bit for bit, dL_dparams by its
largest difference relative to the largest value).

    python scripts/time_f32_grid_second_order.py [--out profiles/f32_grid_second_order_timing.json]
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
WANTS = {"dL_dparams": (False, True, False), "dL_dinput": (True, False, False), "all_three": (True, True, True)}  # input, params, dL_doutput require a gradient
MASKS = {"dL_dparams": (1, 0), "dL_dinput": (2, 0), "all_three": (3, 1, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "f32_grid_second_order_timing.json"))
    args = ap.parse_args()
    result = {"protocol": __doc__.split("Protocol")[1].split("\n\n")[0].strip(" ():\n"), "ms_per_call": {}, "mask_3_against_0": {}}
    try:
        for name, (d, log2_t, scale) in SHAPES.items():
            cfg = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": log2_t, "base_resolution": 16, "per_level_scale": scale}
            m = C.create_encoding(d, cfg, C.Precision.Fp32)
            rng = np.random.default_rng(1)
            x = torch.from_numpy(rng.random((N, d), dtype=np.float32)).cuda()
            p = torch.from_numpy(rng.uniform(-0.5, 0.5, m.n_params()).astype(np.float32)).cuda()
            dy = torch.from_numpy(rng.standard_normal((N, m.n_output_dims())).astype(np.float32)).cuda()
            ddx = torch.from_numpy((rng.standard_normal((N, d)) * 1e-2).astype(np.float32)).cuda()

            def arm(want, mask):
                xs, ps, gs = x.clone().requires_grad_(want[0]), p.clone().requires_grad_(want[1]), dy.clone().requires_grad_(want[2])
                ctx, _ = m.fwd(xs, ps)

                def block(calls, keep=False):
                    C.set_fp32_grid_second_order(mask)
                    assert m.fp32_grid_second_order(N) == mask
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(calls):
                        out = m.bwd_bwd_input(ctx, xs, ps, ddx, gs)
                    b.record()
                    b.synchronize()
                    return out if keep else a.elapsed_time(b) / calls
                return block

            arms = {f"{k}_mask_{mask}": arm(WANTS[k], mask) for k in WANTS for mask in MASKS[k]}
            _, p3, x3 = arms["all_three_mask_3"](1, keep=True)
            _, p0, x0 = arms["all_three_mask_0"](1, keep=True)
            result["mask_3_against_0"][name] = {"dL_dinput_bit_equal": bool(torch.equal(x3, x0)),
                                                "dL_dparams_max_difference_over_max_value": float((p3 - p0).abs().max() / p0.abs().max())}
            print(name, json.dumps(result["mask_3_against_0"][name]), flush=True)
            for block in arms.values():
                block(WARMUP)
            times = {k: [] for k in arms}
            for _ in range(BLOCKS):
                for k, block in arms.items():
                    times[k].append(block(CALLS))
            result["ms_per_call"][name] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
            print(name, json.dumps(result["ms_per_call"][name]), flush=True)
    finally:
        C.set_fp32_grid_second_order(1)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

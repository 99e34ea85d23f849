#!/usr/bin/env python
"""Counts, per grid level, the pair records the record scatter derives and those whose payload words are all +-0, at chosen steps of the
headline run (bench.py's `hash` workload: the same model, seed, batch stream and regenerated batches).

Needs the counting build of the scatter (csrc/exp_diag.h, an EXPERIMENT build -- its kernel times mean nothing):
    scripts/build_variant_one.sh count_zero grid_backward_scatter "-DTCNN_EXP_COUNT_ZERO_PAIRS=1"
    TCNN_HIP_LIBRARY=tiny-cuda-nn_amd/lib/variants/count_zero.so python scripts/exp_zero_records.py --out profiles/zero_records.json
The count is taken over ONE step each (the counters are reset before it)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401

import bench  # noqa: E402
import tinycudann as tcnn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="hash")
    ap.add_argument("--steps", default="1,5,20,25,50,150,500,1000", help="1-based steps to count at")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = C.CDLL(tcnn._C.library_path())
    if not hasattr(lib, "tcnn_exp_zero_pair_counts"):
        raise SystemExit("the loaded library is not the counting build (see this script's docstring)")
    fn = lib.tcnn_exp_zero_pair_counts
    fn.restype = C.c_int
    w = bench.WORKLOADS[args.workload]
    torch.cuda.set_device(0)
    tm = tcnn.create_from_config(w["n_in"], w["n_out"], w["config"], seed=1337)
    rng = tcnn._C.Pcg32(1337)
    bench.make_batches(w, bench.BATCH, 4, rng, device=torch.device("cuda", 0), tcnn=tcnn)  # (the stream position bench.py starts its steps from)
    x, t = bench.make_batches(w, bench.BATCH, 1, rng, device=torch.device("cuda", 0), tcnn=tcnn)[0]
    n_levels = w["config"]["encoding"]["n_levels"]
    wanted = sorted(int(s) for s in args.steps.split(","))
    rows = []
    for step in range(1, wanted[-1] + 1):
        rng.uniform_(x)
        tcnn._C.sinusoid_targets_(x, t)
        if step in wanted:
            assert fn(None, 1) > 0
        tm.training_step(x, t, want_context=False)
        if step in wanted:
            n = fn(None, 0)
            buf = (C.c_ulonglong * (2 * n))()
            assert fn(buf, 0) == n
            pairs = [int(buf[2 * l]) for l in range(n_levels)]
            zero = [int(buf[2 * l + 1]) for l in range(n_levels)]
            g = tm.param_gradients
            row = {"step": step, "pairs": pairs, "zero_pairs": zero, "zero_fraction": sum(zero) / max(1, sum(pairs)),
                   "zero_fraction_per_level": [round(z / max(1, p), 4) for z, p in zip(zero, pairs)],
                   "nonzero_gradient_fraction": float(torch.count_nonzero(g).item()) / g.numel()}
            rows.append(row)
            print(f"step {step:5d}: {sum(zero)} of {sum(pairs)} pairs all zero ({100 * row['zero_fraction']:.1f} %), "
                  f"non-zero parameter gradients {100 * row['nonzero_gradient_fraction']:.1f} %; per level "
                  + " ".join(f"{100 * f:.0f}" for f in row["zero_fraction_per_level"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"workload": args.workload, "batch": bench.BATCH, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()

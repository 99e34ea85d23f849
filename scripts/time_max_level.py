"""Times what switching levels off with max_level saves on the headline grid (HashGrid, 16 levels x 2 features, T = 2^19, base 16, scale 2.0;
N = 2^18): the bare encoding's inference and one training step of the grid + 64 x 2 FullyFusedMLP, at the scalar max_level 1.0 / 0.5 /
0.25 and with the per-sample array whose first half of the batch is coarse (0.25) and whose second half is full (1.0).  The claim to
check: time falls as levels are switched off -- an off (sample, level) costs no gathers in the forward pass and no record in the
backward pass.  HIP event pairs around the timed loop, warm-up first.

usage: python scripts/time_max_level.py [--steps 1000] [--warmup 50] [--n 262144] [--out results.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import tinycudann as T

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    n = args.n
    rng = np.random.default_rng(0)
    enc = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    adam = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    x_np = rng.random((n, 3), dtype=np.float32)
    tgt = np.stack([0.5 + 0.5 * np.sin(6.2831853 * (c + 1) * x_np[:, 0]) * np.cos(6.2831853 * x_np[:, 1]) for c in range(4)], 1).astype(np.float32)
    x, t = torch.from_numpy(x_np).cuda(), torch.from_numpy(tgt).cuda()
    half_coarse = torch.from_numpy(np.where(np.arange(n) < n // 2, 0.25, 1.0).astype(np.float32)).cuda()
    settings = [("max_level_1.0", 1.0, None), ("max_level_0.5", 0.5, None), ("max_level_0.25", 0.25, None), ("array_half_coarse_half_full", 1.0, half_coarse),
                ("array_all_1.0", 1.0, torch.ones(n, device="cuda"))]

    bare = T._C.create_encoding(3, enc)
    params = bare.initial_params(1337).to(T._C.TORCH_DTYPE[bare.param_precision()])
    tm = T.create_from_config(3, 4, {"loss": {"otype": "RelativeL2"}, "optimizer": adam, "encoding": enc, "network": net}, seed=1337)
    C = T._C
    out = torch.empty((n, bare.n_output_dims()), dtype=params.dtype, device="cuda")
    stream, x_ptr, out_ptr, params_ptr = C._stream(), C._ptr(x), C._ptr(out), C._ptr(params)
    result = {"n": n, "steps": args.steps, "warmup": args.warmup}
    for name, scalar, array in settings:
        bare.set_max_level(scalar)
        bare.set_max_level_gpu(array)
        tm.max_level = scalar
        tm.set_max_level_gpu(array)
        # the encoding's inference through the C ABI into a preallocated matrix: no allocation and no Python wrapper per call, so the kernels
        # dominate (through Module.fwd the figure was one host call, ~0.1 ms whatever the setting)
        result[name] = {"encoding_inference_ms": round(timed(lambda: C._check(C._lib.tcnn_module_inference(bare._h, stream, n, x_ptr, out_ptr, params_ptr))), 5),
                        "training_step_ms": round(timed(lambda: tm.training_step(x, t, want_context=False)), 5)}
        # per-stage times of the same step (HIP events around each stage; the profiled steps are slower as a whole): the encoding's forward
        # here is the feature-major gather the network reads, whose stores are coalesced -- the sample-major matrix of the bare encoding above
        # is written 4 bytes per (sample, level) into 64-byte rows, zeros for off levels included
        tm.set_profiling(True)
        for _ in range(200):
            tm.training_step(x, t, want_context=False)
        result[name]["stage_ms"] = {k: round(v[0] / max(v[1], 1), 5) for k, v in tm.stage_times().items() if v[1] and "grid" in k}
        tm.set_profiling(False)
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

"""Times the second-order pass of an fp32 grid encoding: one forward + backward + double backward of
tcnn.Encoding(3, HashGrid 16 levels x 2 features, T = 2^19, base 16, scale 2.0, dtype=float32) at N = 2^18, with the fp32 kernels (mode 0, the
default) and with the 16-bit stand-ins (mode 1, tcnn_set_fp32_second_order), in one process, the two modes interleaved round by round.
The step goes through the ctypes Module (fwd, bwd, bwd_bwd_input: the C ABI plus torch's caching allocator for the results), HIP event
pairs around each timed loop, warm-up first.  per_call_ms_median times the same C-ABI calls one by one: forward, backward, and the
second-order call asked for one result at a time (dL_ddLdoutput, dL_dparams, dL_dinput).  These are times of CALLS -- the kernels each
one launches plus the binding's allocation of the result -- not a per-kernel profile; in mode 1 every call also pays the casts of all
parameters, so its pieces do not add up to the step.

usage: python scripts/time_second_order_f32.py [--steps 200] [--warmup 20] [--rounds 3] [--n 262144] [--out profiles/second_order_f32_timing.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import tinycudann as T

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    C = T._C
    n = args.n
    rng = np.random.default_rng(0)
    enc = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
    h = ctypes.c_void_p()
    C._check(C._lib.tcnn_create_encoding(3, C._dumps(enc), int(C.Precision.Fp32), ctypes.byref(h)))
    m = C.Module(h.value)
    x = torch.from_numpy(rng.random((n, 3), dtype=np.float32)).cuda().requires_grad_(True)
    params = m.initial_params(1337).requires_grad_(True)  # (the times do not depend on the values)
    dy = torch.from_numpy(rng.standard_normal((n, m.n_output_dims())).astype(np.float32)).cuda()
    ddx = torch.from_numpy((rng.standard_normal((n, 3)) * 1e-2).astype(np.float32)).cuda()
    plain = {"x": x.detach(), "params": params.detach(), "dy": dy}

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

    def step():
        ctx, y = m.fwd(x, params)
        m.bwd(ctx, x, params, y, dy)
        m.bwd_bwd_input(ctx, x, params, ddx, dy.requires_grad_(True))

    ctx, y = m.fwd(x, params)

    def only(want):  # the second-order call asked for one result: the binding allocates and the library computes what requires a gradient
        xs = x if want == "dL_dinput" else plain["x"]
        ps = params if want == "dL_dparams" else plain["params"]
        return lambda: m.bwd_bwd_input(ctx, xs, ps, ddx, dy.requires_grad_(want == "dL_ddLdoutput"))

    pieces = {"forward": lambda: m.fwd(x, params), "backward": lambda: m.bwd(ctx, x, params, y, dy.requires_grad_(False)),
              "dL_ddLdoutput": only("dL_ddLdoutput"), "dL_dparams": only("dL_dparams"), "dL_dinput": only("dL_dinput")}
    names = {0: "mode_0_fp32_kernels", 1: "mode_1_16_bit_stand_ins"}
    runs = {0: [], 1: []}
    calls = {0: {k: [] for k in pieces}, 1: {k: [] for k in pieces}}
    try:
        for _ in range(args.rounds):
            for mode in (0, 1):
                C.set_fp32_second_order(mode)
                runs[mode].append(timed(step))
                for k, fn in pieces.items():
                    calls[mode][k].append(timed(fn))
    finally:
        C.set_fp32_second_order(0)
    result = {"n": n, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "encoding": enc}
    for mode in (0, 1):
        result[names[mode]] = {"step_ms_median": round(statistics.median(runs[mode]), 5), "step_ms_rounds": [round(v, 5) for v in runs[mode]],
                               "per_call_ms_median": {k: round(statistics.median(v), 5) for k, v in calls[mode].items()}}
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

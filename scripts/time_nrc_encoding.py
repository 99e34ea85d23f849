"""Times what the NRC input encoding (Composite: TriangleWave x3, OneBlob x5, Identity on the rest; 14 inputs -> 64 features) costs in
front of a 64 x 2 FullyFusedMLP at N = 2^18: the training step with it against the same network behind a 64-wide Identity input (no
encoding kernel: the network reads the fp32 matrix itself) -- the difference is the encoding's cost -- and the fused parameter-free
forward kernel on its own (the bare encoding's inference into a feature-major-equivalent matrix), as a fraction of the HBM roof
(bytes per sample: 56 B of fp32 input + 128 B of 16-bit features).  HIP event pairs around the timed loop, warm-up first.

usage: python scripts/time_nrc_encoding.py [--steps 1000] [--warmup 50] [--n 262144] [--out results.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))

PEAK_HBM = 8.0e12  # B/s, the chip's specification


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

    result = {"n": n, "steps": args.steps, "warmup": args.warmup}
    for name, d, enc in (("nrc", 14, {"otype": "NRC"}), ("identity64", 64, {"otype": "Identity"})):
        x_np = rng.random((n, d), dtype=np.float32)
        tgt = np.stack([0.5 + 0.5 * np.sin(6.2831853 * (c + 1) * x_np[:, 0]) * np.cos(6.2831853 * x_np[:, 1]) for c in range(3)], 1).astype(np.float32)
        x, t = torch.from_numpy(x_np).cuda(), torch.from_numpy(tgt).cuda()
        tm = T.create_from_config(d, 3, {"loss": {"otype": "RelativeL2"}, "optimizer": adam, "encoding": enc, "network": net}, seed=1337)
        result[name + "_training_step_ms"] = round(timed(lambda: tm.training_step(x, t, want_context=False)), 5)
        dx = torch.zeros((n, d), device="cuda")
        result[name + "_training_step_with_dL_dinput_ms"] = round(timed(lambda: tm.training_step(x, t, want_context=False, dL_dinput=dx)), 5)
        result[name + "_inference_ms"] = round(timed(lambda: tm.inference(x)), 5)
        if name == "nrc":
            tm.set_profiling(True)
            for _ in range(min(args.steps, 200)):
                tm.training_step(x, t, want_context=False)
            result["nrc_stage_ms"] = {k: round(v[0] / max(v[1], 1), 5) for k, v in tm.stage_times().items() if v[1]}
            tm.set_profiling(False)
            # the fused parameter-free forward kernel alone: the bare encoding behind the network's alignment writes the same 64 rows
            bare = T._C.create_encoding(14, {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "TriangleWave"}, {"n_dims_to_encode": 5, "otype": "OneBlob", "n_bins": 4},
                                                                             {"n_dims_to_encode": 6, "otype": "Identity"}]})
            p = torch.zeros(0, dtype=tm.params.dtype, device="cuda")
            ms = timed(lambda: bare.fwd(x, p))
            result["bare_encoding_forward_sample_major_ms"] = round(ms, 5)
        del tm
    result["encoding_cost_ms"] = round(result["nrc_training_step_ms"] - result["identity64_training_step_ms"], 5)
    enc_ms = result.get("nrc_stage_ms", {}).get("grid_forward")
    if enc_ms:
        result["fused_forward_kernel_ms"] = enc_ms
        result["fused_forward_fraction_of_hbm_roof"] = round(n * (56 + 128) / (enc_ms * 1e-3) / PEAK_HBM, 4)
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

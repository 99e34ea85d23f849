"""Times the layer-by-layer network (widths outside 16/32/64/128, csrc/mlp_general.hip) behind the hash-grid encoding at N = 2^18:
inference, the whole training step, and the network's share of the step (the trainer's own stage events), for 256 x 2 and 256 x 4 --
and, for comparison, the 128 x 2 / 128 x 4 networks on the three-pass route of the fused widths (tcnn_set_fused_network_passes(0):
forward with saved activations -> loss -> backward), per FLOP.  HIP events, warm-up, then --steps timed steps.

--activation Sine / SiLU times the same networks with a hidden activation that keeps its pre-activations (accurate sinf / cosf, a second
16-bit store per hidden layer; every width then runs layer by layer); --shapes picks a subset, e.g. 256x2.

usage: python scripts/time_general_mlp.py [--steps 200] [--warmup 20] [--n 262144] [--activation ReLU] [--shapes 256x2,256x4,128x2,128x4] [--out results.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))

PEAK_FP16_MFMA = 2.5e15  # dense FLOP/s, the chip's specification


def network_flops(n, in_width, width, hidden_layers, padded_out=16):
    """(forward, training) FLOP of the network alone: 2 per multiply-add; training = forward + dL/d(activation) + dL/d(weight) products"""
    macs = in_width * width + (hidden_layers - 1) * width * width + padded_out * width
    forward = 2.0 * n * macs
    return forward, 3.0 * forward  # (dL/dinput of the first matrix is computed too: the encoding needs it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--activation", default="ReLU", help="hidden activation of the timed networks")
    ap.add_argument("--shapes", default="256x2,256x4,128x2,128x4", help="comma-separated WIDTHxHIDDEN_LAYERS out of the four")
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import tinycudann as T

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    n = args.n
    enc = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
    rng = np.random.default_rng(0)
    pos = rng.random((n, 3), dtype=np.float32)
    tgt = np.stack([0.5 + 0.5 * np.sin(6.2831853 * (c + 1) * pos[:, 0]) * np.cos(6.2831853 * pos[:, 1]) for c in range(4)], 1).astype(np.float32)
    x, t = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()

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

    results = []
    keeps_pre = args.activation.lower() in ("sine", "silu")
    wanted = set(args.shapes.split(","))
    for width, hidden, fused_passes in ((256, 2, 1), (256, 4, 1), (128, 2, 0), (128, 4, 0)):
        if f"{width}x{hidden}" not in wanted:
            continue
        T._C.set_fused_network_passes(bool(fused_passes))
        try:
            cfg = {"loss": {"otype": "RelativeL2"},
                   "optimizer": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6},
                   "encoding": enc, "network": {"otype": "MLP", "activation": args.activation, "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}}
            tm = T.create_from_config(3, 4, cfg, seed=1337)
            step_ms = timed(lambda: tm.training_step(x, t, want_context=False))
            infer_ms = timed(lambda: tm.inference(x))
            tm.set_profiling(True)
            for _ in range(args.steps):
                tm.training_step(x, t, want_context=False)
            stages = {k: v[0] / max(v[1], 1) for k, v in tm.stage_times().items() if v[1]}
            tm.set_profiling(False)
        finally:
            T._C.set_fused_network_passes(True)
        fwd_flop, train_flop = network_flops(n, 32, width, hidden)
        mlp_ms = stages.get("mlp_forward", 0.0) + stages.get("mlp_backward", 0.0) + stages.get("mlp_train_fused", 0.0)
        n_params = width * 32 + (hidden - 1) * width * width + 16 * width
        general = width == 256 or keeps_pre
        r = {"network": f"{width}x{hidden}", "activation": args.activation, "route": "layer-by-layer" if general else "fused kernels, three passes", "n": n,
             "training_step_ms": round(step_ms, 4), "inference_ms": round(infer_ms, 4),
             "stage_ms": {k: round(v, 4) for k, v in stages.items()},
             "network_train_ms": round(mlp_ms, 4), "network_train_gflop": round(train_flop / 1e9, 2),
             "network_train_tflops": round(train_flop / (mlp_ms * 1e-3) / 1e12, 1) if mlp_ms else None,
             "fraction_of_mfma_roof": round(train_flop / (mlp_ms * 1e-3) / PEAK_FP16_MFMA, 4) if mlp_ms else None,
             "ns_per_gflop_training": round(mlp_ms * 1e6 / (train_flop / 1e9), 1) if mlp_ms else None,
             "saved_activations_mb": round((2 if keeps_pre else 1) * hidden * n * width * 2 / 2 ** 20, 1),
             "backward_workspace_mb": round(hidden * n * width * 2 / 2 ** 20, 1) if general else 0.0,
             "inference_ping_pong_mb": round(2 * n * width * 2 / 2 ** 20, 1) if general else 0.0,
             "n_mlp_params": n_params}
        results.append(r)
        print(json.dumps(r), flush=True)
        del tm
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

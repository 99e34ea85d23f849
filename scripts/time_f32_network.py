"""Times the fp32 network (csrc/mlp_general_fp32.hip, tcnn_create_network_precision with TCNN_PRECISION_FP32) against the 16-bit network the
library makes of the same shape, through the module entry points (no trainer: fp32 networks are modules): forward + backward (dL/dinput
and parameter gradients) and inference of 64 -> 64 x 2 -> 16 and 32 -> 256 x 4 -> 16 at N = 2^18.

The 16-bit column is the parent commit's code, untouched, measured in the same run.  With the default ReLU the 16-bit 64-wide network is
the FUSED one (the JSON says which `otype` was timed); --activation SiLU makes both precisions run layer by layer at either width.

HIP events around --steps calls after --warmup calls, repeated --repeats times: the median of the repeats is reported with their minimum
and maximum (the spread).  Buffers are allocated once, outside the timed region.

usage: python scripts/time_f32_network.py [--steps 50] [--warmup 10] [--repeats 5] [--n 262144] [--activation ReLU] [--out results.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))

PEAK_FP32_MFMA = 157.3e12  # dense FLOP/s of v_mfma_f32_*_f32, the chip's specification
PEAK_FP16_MFMA = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--activation", default="ReLU")
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    import torch
    import tinycudann as T

    C = T._C
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    n = args.n

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        samples = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            samples.append(a.elapsed_time(b) / args.steps)
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    results = []
    for in_width, width, hidden in ((64, 64, 2), (32, 256, 4)):
        cfg = {"otype": "MLP", "activation": args.activation, "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}
        macs = in_width * width + (hidden - 1) * width * width + 16 * width
        forward_flop = 2.0 * n * macs
        for precision in (C.Precision.Fp32, C.preferred_precision()):
            m = C.create_network_precision(in_width, 16, cfg, precision)
            dtype = C.TORCH_DTYPE[precision]
            x = (torch.rand((n, in_width), device="cuda") * 2 - 1).requires_grad_(True)
            p = m.initial_params(1337).to(dtype).requires_grad_(True)
            dy = (torch.rand((n, 16), device="cuda") * 2 - 1).to(dtype)
            x_inf, p_inf = x.detach(), p.detach()

            def forward_backward():
                ctx, y = m.fwd(x, p)
                m.bwd(ctx, x, p, y, dy)

            fb = timed(forward_backward)
            inf = timed(lambda: m.fwd(x_inf, p_inf))
            peak = PEAK_FP32_MFMA if precision == C.Precision.Fp32 else PEAK_FP16_MFMA
            r = {"network": f"{in_width}->{width}x{hidden}->16", "activation": args.activation, "precision": precision.name, "otype": m.hyperparams()["network"]["otype"], "n": n,
                 "forward_backward": fb, "inference": inf,
                 "forward_backward_tflops": round(3.0 * forward_flop / (fb["median_ms"] * 1e-3) / 1e12, 2),
                 "inference_tflops": round(forward_flop / (inf["median_ms"] * 1e-3) / 1e12, 2),
                 "forward_backward_fraction_of_mfma_roof": round(3.0 * forward_flop / (fb["median_ms"] * 1e-3) / peak, 4),
                 "inference_fraction_of_mfma_roof": round(forward_flop / (inf["median_ms"] * 1e-3) / peak, 4)}
            results.append(r)
            print(json.dumps(r), flush=True)
            del m, x, p, dy
            C.free_temporary_memory()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

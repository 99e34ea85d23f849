"""Times the fp32 network (csrc/mlp_general_fp32.hip, tcnn_create_network_precision with TCNN_PRECISION_FP32) against the 16-bit network the
library makes of the same shape, through the module entry points (no trainer: fp32 networks are modules): forward + backward (dL/dinput
and parameter gradients) and inference of 64 -> 64 x 2 -> 16 and 32 -> 256 x 4 -> 16 at N = 2^18.

The 16-bit column is the parent commit's code, untouched, measured in the same run.  With the default ReLU the 16-bit 64-wide network is
the FUSED one (the JSON says which `otype` was timed); --activation SiLU makes both precisions run layer by layer at either width.

HIP events around --steps calls after --warmup calls, repeated --repeats times: the median of the repeats is reported with their minimum
and maximum (the spread).  Buffers are allocated once, outside the timed region.

--fused-ab: instead, the fp32 network's fused forward / inference kernel (csrc/mlp_f32_fused.hip) against the layer-by-layer kernels in the
same run, toggled by tcnn_set_fp32_fused_network: 64 -> 64 x 2 -> 16 and 32 -> 32 x 3 -> 32, inference and the forward pass that saves
activations (no backward).  The two settings alternate block by block (--repeats blocks of --steps calls each, after --warmup calls of
both); per setting the median block with the minimum and maximum.  Beside each: the bytes per sample the pass has to move (input, output,
saved activations) and the fraction of the HBM roof the median implies.

--fused-backward-ab: the same protocol and networks for the fused backward kernels (csrc/mlp_f32_fused_backward.hip), toggled by
tcnn_set_fp32_fused_backward with the forward switch on in both arms: forward + backward (dL/dinput and parameter gradients), and the
backward call alone on one saved context.

usage: python scripts/time_f32_network.py [--steps 50] [--warmup 10] [--repeats 5] [--n 262144] [--activation ReLU] [--fused-ab | --fused-backward-ab]
       [--out results.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))

PEAK_FP32_MFMA = 157.3e12  # dense FLOP/s of v_mfma_f32_*_f32, the chip's specification
PEAK_FP16_MFMA = 2.5e15
PEAK_HBM = 8.0e12       # bytes/s, the chip's specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--activation", default="ReLU")
    ap.add_argument("--fused-ab", action="store_true", help="fp32 only: the fused forward / inference kernel against the layer-by-layer kernels")
    ap.add_argument("--fused-backward-ab", action="store_true", help="fp32 only: the fused backward kernels against the layer-by-layer backward pass")
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

    def block(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    def fused_ab(backward):
        out = []
        switch, query = (C.set_fp32_fused_backward, "fp32_fused_backward") if backward else (C.set_fp32_fused_network, "fp32_fused_network")
        for in_width, width, hidden, outp in ((64, 64, 2, 16), (32, 32, 3, 32)):
            cfg = {"otype": "MLP", "activation": args.activation, "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}
            m = C.create_network_precision(in_width, outp, cfg, C.Precision.Fp32)
            x = (torch.rand((n, in_width), device="cuda") * 2 - 1).requires_grad_(True)
            p = m.initial_params(1337).requires_grad_(True)
            x_inf, p_inf = x.detach(), p.detach()
            saves = 2 if args.activation in ("SiLU", "Sine") else 1
            passes = {"inference": (lambda: m.fwd(x_inf, p_inf), 4 * (in_width + outp)),
                      "forward": (lambda: m.fwd(x, p), 4 * (in_width + outp + saves * hidden * width))}
            if backward:
                dy = torch.rand((n, outp), device="cuda") * 2 - 1
                ctx, y = m.fwd(x, p)

                def forward_backward():
                    c, out_ = m.fwd(x, p)
                    m.bwd(c, x, p, out_, dy)

                # backward reads dL/doutput and the stack at the derivative's values, writes dL/dinput; the gradients read the input, the
                # post-activations and each layer's dL/d(pre-activation), which (layer by layer, or for the gradients) is also written once
                bwd_bytes = 4 * (2 * in_width + 2 * outp + 4 * hidden * width)
                passes = {"forward_backward": (forward_backward, passes["forward"][1] + bwd_bytes), "backward": (lambda: m.bwd(ctx, x, p, y, dy), bwd_bytes)}
            for name, (fn, bytes_per_sample) in passes.items():
                samples = {True: [], False: []}
                try:
                    for fused in (True, False):
                        switch(fused)
                        assert getattr(m, query)(n) == int(fused)
                        for _ in range(args.warmup):
                            fn()
                    torch.cuda.synchronize()
                    for _ in range(args.repeats):
                        for fused in (True, False):
                            switch(fused)
                            samples[fused].append(block(fn))
                finally:
                    switch(True)
                r = {"network": f"{in_width}->{width}x{hidden}->{outp}", "activation": args.activation, "pass": name, "n": n, "bytes_per_sample": bytes_per_sample}
                for fused, key in ((True, "fused"), (False, "layer_by_layer")):
                    med = statistics.median(samples[fused])
                    r[key] = {"median_ms": round(med, 4), "min_ms": round(min(samples[fused]), 4), "max_ms": round(max(samples[fused]), 4),
                              "fraction_of_hbm_roof": round(bytes_per_sample * n / (med * 1e-3) / PEAK_HBM, 4)}
                r["speedup"] = round(r["layer_by_layer"]["median_ms"] / r["fused"]["median_ms"], 2)
                out.append(r)
                print(json.dumps(r), flush=True)
            del m, x, p
            C.free_temporary_memory()
        return out

    ab = args.fused_ab or args.fused_backward_ab
    results = fused_ab(args.fused_backward_ab) if ab else []
    for in_width, width, hidden in () if ab else ((64, 64, 2), (32, 256, 4)):
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

"""Times an eikonal training step on an fp32 network -- forward, backward with create_graph, double backward
(tcnn_module_backward_backward_input, csrc/mlp_general_fp32.hip mlp_f32_backward_backward) -- through tcnn.Network(dtype=torch.float32)
at N = 2^18 for 32 -> 256 x 4 -> 16 and 3 -> 64 x 2 -> 1, both with Softplus (beta 10, the library's), against a torch.nn.Linear fp32 MLP
of the same shape doing the same step in the same run: what a user does today, when the network behind a grid has to be plain torch.

The step: y = net(x); g = d(y.sum())/dx with create_graph; loss = ((|g| - 1)^2).mean(); loss.backward() -- parameter gradients of both.
HIP events around --steps steps after --warmup steps, repeated --repeats times: the median of the repeats with their minimum and maximum.

usage: python scripts/time_f32_second_order.py [--steps 20] [--warmup 5] [--repeats 5] [--n 262144] [--out results.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--out", default=None, help="also write the results to this JSON file")
    args = ap.parse_args()
    import torch
    import tinycudann as T

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

    def eikonal_step(net, x):
        def step():
            net.zero_grad(set_to_none=True)
            y = net(x)
            g, = torch.autograd.grad(y.sum(), [x], create_graph=True)
            ((g.norm(dim=1) - 1.0) ** 2).mean().backward()
        return step

    results = []
    for in_width, width, hidden, out in ((32, 256, 4, 16), (3, 64, 2, 1)):
        cfg = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}
        x = (torch.rand((n, in_width), device="cuda") * 2 - 1).requires_grad_(True)
        native = T.Network(in_width, out, cfg, dtype=torch.float32)
        layers, k = [], in_width
        for _ in range(hidden):
            layers += [torch.nn.Linear(k, width, bias=False), torch.nn.Softplus(beta=10.0)]
            k = width
        plain = torch.nn.Sequential(*layers, torch.nn.Linear(k, out, bias=False)).cuda()
        r = {"network": f"{in_width}->{width}x{hidden}->{out}", "activation": "Softplus", "n": n, "tcnn_fp32": timed(eikonal_step(native, x)),
             "torch_linear_fp32": timed(eikonal_step(plain, x))}
        r["torch_over_tcnn"] = round(r["torch_linear_fp32"]["median_ms"] / r["tcnn_fp32"]["median_ms"], 3)
        results.append(r)
        print(json.dumps(r), flush=True)
        del native, plain, x
        T.free_temporary_memory()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

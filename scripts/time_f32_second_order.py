"""Times an eikonal training step on an fp32 network -- forward, backward with create_graph, double backward
(tcnn_module_backward_backward_input, csrc/mlp_general_fp32.hip mlp_f32_backward_backward) -- through tcnn.Network(dtype=torch.float32)
at N = 2^18 for 32 -> 256 x 4 -> 16 and 3 -> 64 x 2 -> 1, both with Softplus (beta 10, the library's), against a torch.nn.Linear fp32 MLP
of the same shape doing the same step in the same run: what a user does today, when the network behind a grid has to be plain torch.

The step: y = net(x); g = d(y.sum())/dx with create_graph; loss = ((|g| - 1)^2).mean(); loss.backward() -- parameter gradients of both.
HIP events around --steps steps after --warmup steps, repeated --repeats times: the median of the repeats with their minimum and maximum.

--fused-ab: instead, the fused second-order kernels (csrc/mlp_f32_fused_second_order.hip) against the layer-by-layer launches in the same
run, toggled by tcnn_set_fp32_fused_second_order with the forward and backward switches on in both arms, through the module entry points on
resident data: 32 -> 64 x 2 -> 4 with Softplus and with ReLU and 32 -> 32 x 3 -> 32 with Softplus; the bwd_bwd_input call alone with all three
results on one saved context, and forward + backward + double backward.  The two settings alternate block by block (--repeats blocks of
--steps calls each, after --warmup calls of both); per setting the median block with the minimum and maximum.  Beside the call alone: the
bytes per sample its three kernels have to move and the fraction of the HBM roof the median implies.

usage: python scripts/time_f32_second_order.py [--steps 20] [--warmup 5] [--repeats 5] [--n 262144] [--fused-ab] [--out results.json]"""
import argparse
import json
import os
import statistics
import sys

PEAK_HBM = 8.0e12  # bytes/s, the chip's specification

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--fused-ab", action="store_true", help="the fused second-order kernels against the layer-by-layer launches")
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

    def block(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    def fused_ab():
        C = T._C
        out = []
        for in_width, width, hidden, n_out, activation in ((32, 64, 2, 4, "Softplus"), (32, 64, 2, 4, "ReLU"), (32, 32, 3, 32, "Softplus")):
            cfg = {"otype": "CutlassMLP", "activation": activation, "output_activation": "None", "n_neurons": width, "n_hidden_layers": hidden}
            m = C.create_network_precision(in_width, n_out, cfg, C.Precision.Fp32)
            outp = m.n_output_dims()  # padded
            x = (torch.rand((n, in_width), device="cuda") * 2 - 1).requires_grad_(True)
            p = m.initial_params(1337).requires_grad_(True)
            v = torch.rand((n, in_width), device="cuda") * 2 - 1
            dy = (torch.rand((n, outp), device="cuda") * 2 - 1).requires_grad_(True)
            ctx, _ = m.fwd(x, p)

            def all_three():
                c, y = m.fwd(x, p)
                m.bwd(c, x, p, y, dy)
                m.bwd_bwd_input(c, x, p, v, dy)

            # tangent chain: v, at in; U, T, dL/d(dy) out.  reverse chains: at, T, g in; D, C, dL/dinput out.  weight gradients: D, U, C, a, g, v, x in.
            # Without curvature (ReLU): no T, no C, no second operand pair; dL/dinput is zeros
            curved = activation not in ("None", "ReLU", "LeakyReLU")
            bytes_per_sample = 4 * ((4 if curved else 3) * in_width + 3 * outp + (10 if curved else 5) * hidden * width)
            for name, fn in (("bwd_bwd_input", lambda: m.bwd_bwd_input(ctx, x, p, v, dy)), ("forward_backward_double_backward", all_three)):
                samples = {True: [], False: []}
                try:
                    for fused in (True, False):
                        C.set_fp32_fused_second_order(fused)
                        assert m.fp32_fused_second_order(n) == int(fused) and m.fp32_fused_backward(n) == 1
                        for _ in range(args.warmup):
                            fn()
                    torch.cuda.synchronize()
                    for _ in range(args.repeats):
                        for fused in (True, False):
                            C.set_fp32_fused_second_order(fused)
                            samples[fused].append(block(fn))
                finally:
                    C.set_fp32_fused_second_order(True)
                r = {"network": f"{in_width}->{width}x{hidden}->{n_out}", "activation": activation, "pass": name, "n": n}
                if name == "bwd_bwd_input":
                    r["bytes_per_sample"] = bytes_per_sample
                for fused, key in ((True, "fused"), (False, "layer_by_layer")):
                    med = statistics.median(samples[fused])
                    r[key] = {"median_ms": round(med, 4), "min_ms": round(min(samples[fused]), 4), "max_ms": round(max(samples[fused]), 4)}
                    if name == "bwd_bwd_input" and fused:
                        r[key]["fraction_of_hbm_roof"] = round(bytes_per_sample * n / (med * 1e-3) / PEAK_HBM, 4)
                r["speedup"] = round(r["layer_by_layer"]["median_ms"] / r["fused"]["median_ms"], 2)
                out.append(r)
                print(json.dumps(r), flush=True)
            del m, x, p, ctx
            C.free_temporary_memory()
        return out

    results = fused_ab() if args.fused_ab else []
    for in_width, width, hidden, out in () if args.fused_ab else ((32, 256, 4, 16), (3, 64, 2, 1)):
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

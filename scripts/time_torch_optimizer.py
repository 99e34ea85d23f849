"""Times one training step of the headline shape through the PyTorch modules (batch 2^18, HashGrid 16 levels x 2, T = 2^19, FullyFusedMLP
64 x 2, 3-D -> 4, RelativeL2) with two loops, in the same run, on the same module configuration and the same resident batches:

  torch   -- RelativeL2 written in torch (the reference's gradient: the denominator is not differentiated) + torch.optim.Adam
  native  -- tinycudann.Loss("RelativeL2") + tinycudann.optim.Optimizer (Adam): the library's loss and optimizer kernels in fp32

Both loops run forward, loss, backward, optimizer step and zero_grad(set_to_none=True).  HIP events around --steps steps after --warmup
steps, repeated --repeats times: the median of the repeats is reported with their minimum and maximum (the spread).

usage: python scripts/time_torch_optimizer.py [--steps 50] [--warmup 20] [--repeats 7] [--n 262144] [--out profiles/torch_optimizer_timing.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))

ENCODING = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 2.0}
NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
ADAM = {"learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    import torch
    import tinycudann as tcnn

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    n = args.n
    batches = []
    for k in range(4):
        x = torch.rand((n, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(k))
        y = torch.empty((n, 4), device="cuda")
        tcnn._C.sinusoid_targets_(x, y)
        batches.append((x, y))

    def timed(step):
        for k in range(args.warmup):
            step(k)
        torch.cuda.synchronize()
        samples = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.steps):
                step(k)
            b.record()
            torch.cuda.synchronize()
            samples.append(a.elapsed_time(b) / args.steps)
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    def torch_loop():
        model = tcnn.NetworkWithInputEncoding(3, 4, ENCODING, NETWORK, seed=1337).cuda()
        opt = torch.optim.Adam(model.parameters(), lr=ADAM["learning_rate"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["epsilon"])

        def step(k):
            x, y = batches[k % len(batches)]
            p = model(x).float()
            loss = ((p - y) ** 2 / (p.detach() ** 2 + 0.01)).mean()
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return timed(step)

    def native_loop():
        model = tcnn.NetworkWithInputEncoding(3, 4, ENCODING, NETWORK, seed=1337).cuda()
        opt = tcnn.optim.Optimizer(model, {"otype": "Adam", **ADAM})
        loss_fn = tcnn.Loss("RelativeL2")

        def step(k):
            x, y = batches[k % len(batches)]
            loss = loss_fn(model(x).float(), y)  # (fp32 as in the torch loop: the fp32 loss kernel)
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return timed(step)

    result = {"shape": "HashGrid(L=16,F=2,T=2^19,base 16,per_level_scale 2.0) + FullyFusedMLP 64x2, 3-D -> 4, RelativeL2", "n": n, "steps": args.steps,
              "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
              "torch_optim_adam_torch_loss": torch_loop(), "tinycudann_optim_adam_tinycudann_loss": native_loop()}
    result["native_over_torch"] = round(result["tinycudann_optim_adam_tinycudann_loss"]["median_ms"] / result["torch_optim_adam_torch_loss"]["median_ms"], 3)
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

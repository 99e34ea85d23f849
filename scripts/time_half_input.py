"""Times what handing a `Network` module a resident 16-bit tensor costs with and without the 16-bit route (tcnn_module_*_half_input):
forward plus backward (parameter and input gradients) of Network(64 -> 64 x 2 -> 16) and Network(20 -> 128 x 4 -> 16) at N = 2^18.
  cast:  net(x.float()) -- what Module.forward did with every 16-bit input before the route existed: a torch cast to fp32 and the identity
         kernel in front of the network, the identity's backward kernel and autograd's cast of the fp32 gradient behind it;
  half:  net(x) -- one pad / transpose kernel each way, the gradient comes back in 16 bits.
The two are interleaved (cast, half, cast, half, ...); every measurement is 50 warm-up steps, then 1000 steps between one pair of HIP
events.  Both compute the same bits (tests/test_gpu_half_input.py).

usage: python scripts/time_half_input.py [--steps 1000] [--warmup 50] [--rounds 3] [--n 262144] [--out profiles/half_input_timing.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-cuda-nn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
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
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    shapes = {"64_to_64x2_to_16": (64, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}),
              "20_to_128x4_to_16": (20, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 128, "n_hidden_layers": 4})}
    result = {"n": n, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "binding": "compiled" if T._C.EXT is not None else "ctypes",
              "library": os.path.basename(T._C.library_path())}
    for name, (d, network) in shapes.items():
        net = T.Network(d, 16, network)
        assert net.native_tcnn_module.supports_half_input()
        g = torch.Generator(device="cuda").manual_seed(1)
        x = (torch.rand((n, d), device="cuda", generator=g) * 2 - 1).to(net.dtype).requires_grad_(True)
        dy = torch.randn((n, 16), device="cuda", generator=g).to(net.dtype)

        def step(widen):
            y = net(x.float() if widen else x)
            dparams, dx = torch.autograd.grad(y, [net.params, x], dy)
            assert dx.dtype == net.dtype
            return dparams, dx

        same = all(torch.equal(a, b) for a, b in zip(step(True), step(False)))
        times = {"cast": [], "half": []}
        for _ in range(args.rounds):
            times["cast"].append(round(timed(lambda: step(True)), 5))
            times["half"].append(round(timed(lambda: step(False)), 5))
        cast_ms, half_ms = statistics.median(times["cast"]), statistics.median(times["half"])
        result[name] = {"cast_ms": cast_ms, "half_ms": half_ms, "saved_ms": round(cast_ms - half_ms, 5), "cast_ms_rounds": times["cast"], "half_ms_rounds": times["half"],
                        "same_gradients": bool(same), "input_bytes_16bit": n * d * 2}
        del net
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

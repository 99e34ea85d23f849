"""Kernel trace of the encoding paths: a bare 16-bit grid, an fp32 grid, a Composite (16-bit and fp32) and both behind a network, each forward
with input gradients and backward once.  profiles/encoding_paths_trace_*.txt are its launches before and after the host paths were merged:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/trace_encoding_paths.py
    python scripts/trace_encoding_paths.py --list DIR > launches.txt      # one line per launch in start order: name grid block"""
import csv, glob, os, sys


def list_launches(directory):
    rows = []
    for f in glob.glob(directory + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        print(r["Kernel_Name"], "grid", r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], "block", r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"])


if len(sys.argv) == 3 and sys.argv[1] == "--list":
    list_launches(sys.argv[2])
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tiny-cuda-nn_amd")]
import numpy as np
import torch
import tinycudann as T
C = T._C
n = 512
GRID = {"otype": "HashGrid", "n_levels": 3, "n_features_per_level": 2, "log2_hashmap_size": 8, "base_resolution": 4, "per_level_scale": 2.0}
MIXED = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "Identity"}, dict(GRID, n_dims_to_encode=3, n_levels=2, n_features_per_level=4, log2_hashmap_size=10),
                                          {"n_dims_to_encode": 2, "otype": "TriangleWave", "n_frequencies": 2}]}
rng = np.random.default_rng(0)
for d, cfg, fp32 in ((3, GRID, False), (3, GRID, True), (8, MIXED, False), (8, MIXED, True)):
    m = C.create_encoding(d, cfg, *([C.Precision.Fp32] if fp32 else []))
    dt = torch.float32 if fp32 else torch.half
    x = torch.from_numpy(rng.random((n, d), dtype=np.float32)).cuda().requires_grad_(True)
    p = torch.from_numpy(rng.uniform(-0.5, 0.5, m.n_params()).astype(np.float32)).cuda().to(dt).requires_grad_(True)
    dy = torch.from_numpy(rng.standard_normal((n, m.n_output_dims())).astype(np.float32)).cuda().to(dt)
    ctx, y = m.fwd(x, p)
    dx, dp = m.bwd(ctx, x, p, y, dy)
    torch.cuda.synchronize()
    print(cfg["otype"], "fp32" if fp32 else "half", float(dx.abs().sum()), float(dp.float().abs().sum()))
# the same grid and Composite behind a network, through the trainer (the feature-major path)
for d, cfg in ((3, GRID), (8, MIXED)):
    tm = T.create_from_config(d, 3, {"loss": {"otype": "L2"}, "optimizer": {"otype": "Adam"}, "encoding": cfg,
                                     "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}}, seed=3)
    x = torch.from_numpy(rng.random((n, d), dtype=np.float32)).cuda()
    t = torch.from_numpy(rng.random((n, 3), dtype=np.float32)).cuda()
    dx = torch.zeros((n, d), device="cuda")
    tm.training_step(x, t, run_optimizer=False, dL_dinput=dx)
    torch.cuda.synchronize()
    print(cfg["otype"], "trainer", float(dx.abs().sum()))

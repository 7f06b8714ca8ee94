"""Microbenchmark of the fused Linear + label-smoothed CE (ops.linear_xent,
forward + backward with dW / db) against stock eager torch
F.cross_entropy(H @ W.T + b) with autograd on the same tensors and the same
GPU. One JSON line per shape NxVxE (N tokens, `--valid` of them not ignored):
time of each (device events, alternating windows, median / min / max), their
ratio, ns per GFLOP, and the share of the f32-MFMA time of the op's four
products of 2 N_valid V E FLOP at 155 TF. Pick V so that eager's [N, V] logits
fit."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tdfo_amd import ops  # noqa: E402

PEAK_F32_MFMA = 155e12      # FLOP/s

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="12800x30002x128,6400x30002x256,12800x30002x64",
                help="comma list of NxVxE")
ap.add_argument("--valid", type=float, default=0.2, help="share of tokens with a label")
ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_linear_xent needs a GPU"
dev = "cuda"


def window(fn, iters):
    """ms per call over one window of `iters` calls, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


for spec in args.shapes.split(","):
    N, V, E = (int(x) for x in spec.split("x"))
    g = torch.Generator(device=dev).manual_seed(0)
    H = torch.randn(N, E, device=dev, generator=g)
    W = torch.randn(V, E, device=dev, generator=g) * 0.2
    b = torch.randn(V, device=dev, generator=g) * 0.1
    y = torch.randint(1, V, (N,), device=dev, generator=g)
    y[torch.rand(N, device=dev, generator=g) >= args.valid] = 0
    nv = int((y != 0).sum())
    dH, lv = torch.empty(N, E, device=dev), torch.empty(N, device=dev)
    dW, db, loss = torch.empty(V, E, device=dev), torch.empty(V, device=dev), torch.empty(1, device=dev)

    def hip():
        ops.linear_xent(H, W, b, y, 0.1, 0, dH, lv, dW, db, loss=loss)

    Hr, Wr, br = (t.clone().requires_grad_(True) for t in (H, W, b))

    def eager():
        Hr.grad = Wr.grad = br.grad = None
        torch.nn.functional.cross_entropy(Hr @ Wr.t() + br, y, ignore_index=0,
                                          label_smoothing=0.1).backward()

    fns = {"hip": hip} if args.no_torch else {"hip": hip, "eager": eager}
    for fn in fns.values():                      # warm-up: code objects, library algorithms
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.repeats):                # alternate the two in one process
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
    rec = {"N": N, "N_valid": nv, "V": V, "E": E}
    for k, v in ms.items():
        rec[f"{k}_ms"] = round(statistics.median(v), 4)
        rec[f"{k}_ms_min"] = round(min(v), 4)
        rec[f"{k}_ms_max"] = round(max(v), 4)
    flops = 4 * 2.0 * nv * V * E
    rec["hip_ns_per_gflop"] = round(rec["hip_ms"] * 1e6 / (flops / 1e9), 3)
    rec["hip_fraction_of_f32_mfma_peak"] = round(flops / PEAK_F32_MFMA * 1e3 / rec["hip_ms"], 3)
    if not args.no_torch:
        rec["eager_over_hip"] = round(rec["eager_ms"] / rec["hip_ms"], 2)
        hip()
        eager()
        torch.cuda.synchronize()
        rec["max_abs_dW_diff"] = float((Wr.grad - dW).abs().max())
        rec["max_abs_dH_diff"] = float((Hr.grad - dH).abs().max())
    print(json.dumps(rec), flush=True)

"""Microbenchmark of the candidate-subset Linear + label-smoothed CE
(ops.linear_xent_rows: sampled softmax, forward + backward with dW / db)
against stock eager torch on the same GPU: gather of the candidate rows,
matmul, F.cross_entropy, autograd (its dW is the dense [V, E] gradient of the
gather). Every one of the N tokens carries a label; the candidates are the
labels plus S uniform negatives, built by ops.xent_candidates (M = N + S slots,
the repeats holes). One JSON line per NxSxE: time of each (device events,
alternating windows, median / min / max), the HIP call with the [V, E] + [V]
zero fill a training step adds, ns per GFLOP and the share of the f32-MFMA
time of the op's four products of 2 N Mv E FLOP at 155 TF."""
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
ap.add_argument("--shapes", default="12800x1024x64,12800x4096x64,12800x16384x64,"
                "12800x1024x128,12800x4096x128,12800x16384x128", help="comma list of NxSxE")
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_xent_rows needs a GPU"
dev = "cuda"
V = args.items + 2


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
    N, S, E = (int(x) for x in spec.split("x"))
    g = torch.Generator(device=dev).manual_seed(0)
    H = torch.randn(N, E, device=dev, generator=g)
    W = torch.randn(V, E, device=dev, generator=g) * 0.2
    b = torch.randn(V, device=dev, generator=g) * 0.1
    labels = torch.randint(1, V - 1, (N,), device=dev, generator=g)
    neg = torch.empty(S, dtype=torch.int64, device=dev)
    ops.sample_ids(42, torch.zeros(1, dtype=torch.int64, device=dev), 1, V - 1, neg)
    cand = torch.empty(N + S, dtype=torch.int64, device=dev)
    target = torch.empty(N, dtype=torch.int64, device=dev)
    ops.xent_candidates(labels, neg, 0, cand, target)
    slots = torch.nonzero(cand >= 0).view(-1)
    Mv = slots.numel()
    dH, lv = torch.empty(N, E, device=dev), torch.empty(N, device=dev)
    dW, db, loss = torch.zeros(V, E, device=dev), torch.zeros(V, device=dev), torch.empty(1, device=dev)

    def hip():
        ops.linear_xent_rows(H, W, b, cand, target, 0.1, dH, lv, dW, db, loss=loss)

    def hip_fill():
        dW.zero_()
        db.zero_()
        hip()

    # eager: the holes taken out beforehand (not timed), targets remapped
    rows = cand[slots]
    pos = torch.full((N + S,), -100, dtype=torch.int64, device=dev)
    pos[slots] = torch.arange(Mv, device=dev)
    y = pos[target]
    Hr, Wr, br = (t.clone().requires_grad_(True) for t in (H, W, b))

    def eager():
        Hr.grad = Wr.grad = br.grad = None
        torch.nn.functional.cross_entropy(Hr @ Wr[rows].t() + br[rows], y,
                                          label_smoothing=0.1).backward()

    fns = {"hip": hip, "hip_fill": hip_fill}
    if not args.no_torch:
        fns["eager"] = eager
    for fn in fns.values():                      # warm-up: code objects, library algorithms
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.repeats):                # alternate them in one process
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
    rec = {"N": N, "S": S, "M": N + S, "Mv": Mv, "V": V, "E": E}
    for k, v in ms.items():
        rec[f"{k}_ms"] = round(statistics.median(v), 4)
        rec[f"{k}_ms_min"] = round(min(v), 4)
        rec[f"{k}_ms_max"] = round(max(v), 4)
    flops = 4 * 2.0 * N * Mv * E
    rec["hip_ns_per_gflop"] = round(rec["hip_ms"] * 1e6 / (flops / 1e9), 3)
    rec["hip_fraction_of_f32_mfma_peak"] = round(flops / PEAK_F32_MFMA * 1e3 / rec["hip_ms"], 3)
    if not args.no_torch:
        rec["eager_over_hip"] = round(rec["eager_ms"] / rec["hip_ms"], 2)
        rec["eager_over_hip_fill"] = round(rec["eager_ms"] / rec["hip_fill_ms"], 2)
        hip_fill()
        eager()
        torch.cuda.synchronize()
        rec["max_abs_dW_diff"] = float((Wr.grad - dW).abs().max())
        rec["max_abs_dH_diff"] = float((Hr.grad - dH).abs().max())
    print(json.dumps(rec), flush=True)

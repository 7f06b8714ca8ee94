"""Microbenchmark of the fused full-catalogue top-K search (ops.topk_scores)
against stock eager ``torch.topk(q @ W.T + b, k)`` on the same GPU (chunked
over B where the [B, V] score matrix would not fit), at the Bert4Rec and
TwoTower catalogue shapes, at the embedding width --embed-dim. One JSON line
per shape: fused / eager time, the fused time's share of the f32-MFMA time
2 B V E / 155 TF and of one HBM pass over W at 6.3 TB/s, (with --splits) the
time under forced numbers of V ranges and (with --fallback) the time of the
chunked torch reference on the same device tensors, which is what
ops.topk_scores ran at E = 128 / 256 before the fused search covered them.
--rounds n times fused, fallback and eager n times each, alternating, and
reports the median with the range."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tdfo_amd import ops  # noqa: E402

PEAK_F32_MFMA = 155e12      # FLOP/s
PEAK_HBM = 6.3e12           # B/s
SHAPES = {"bert4rec": (1_000_002, 256, 100), "two_tower": (2_360_650, 2048, 100)}   # V, B, K

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="", help="bert4rec | two_tower (default: both)")
ap.add_argument("--splits", default="", help="comma list of forced split counts to A/B (0 = auto)")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--eager-score-bytes", type=float, default=4e9,
                help="largest eager score matrix: B is chunked to stay below it")
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--embed-dim", type=int, default=16, choices=ops.topk_fused_widths())
ap.add_argument("--fallback", action="store_true",
                help="also time ops.reference.topk_scores on the device tensors")
ap.add_argument("--rounds", type=int, default=1,
                help="alternating timing rounds per variant (median and range reported)")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_retrieval needs a GPU"
dev = "cuda"


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e6


def summary(rec, key, xs):
    """Median under `key`; with several rounds the range too."""
    rec[key] = round(statistics.median(xs), 1)
    if len(xs) > 1:
        rec[key + "_range"] = [round(min(xs), 1), round(max(xs), 1)]


E = args.embed_dim
for name, (V, B, K) in SHAPES.items():
    if args.shape and name != args.shape:
        continue
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B, E, device=dev, generator=g)
    W = torch.randn(V, E, device=dev, generator=g) * 0.1
    b = torch.randn(V, device=dev, generator=g) * 0.1
    ids = torch.empty(B, K, dtype=torch.int64, device=dev)
    sc = torch.empty(B, K, device=dev)

    def fused():
        ops.topk_scores(q, W, b, K, ids, sc)

    fids = torch.empty(B, K, dtype=torch.int64, device=dev)
    fsc = torch.empty(B, K, device=dev)

    def fallback():
        ops.reference.topk_scores(q, W, b, K, fids, fsc)

    cb = max(1, min(B, int(args.eager_score_bytes // (4 * V))))

    def eager():
        out = [torch.topk(q[i: i + cb] @ W.t() + b, K) for i in range(0, B, cb)]
        return out

    rec = {"shape": name, "V": V, "E": E, "B": B, "K": K}
    few = max(2, args.iters // 4)
    t_fused, t_fb, t_eager = [], [], []
    for _ in range(max(1, args.rounds)):
        t_fused.append(timed(fused, args.iters))
        if args.fallback:
            t_fb.append(timed(fallback, few))
        if not args.no_torch:
            t_eager.append(timed(eager, few))
    summary(rec, "fused_us", t_fused)
    us = statistics.median(t_fused)
    t_mfma = 2.0 * B * V * E / PEAK_F32_MFMA * 1e6
    t_hbm = V * E * 4 / PEAK_HBM * 1e6
    rec["f32_mfma_floor_us"] = round(t_mfma, 1)
    rec["hbm_pass_us"] = round(t_hbm, 1)
    rec["fraction_of_mfma_peak"] = round(t_mfma / us, 3)
    rec["fraction_of_hbm_pass"] = round(t_hbm / us, 3)
    for s in [int(x) for x in args.splits.split(",") if x]:
        old = ops.topk_splits(s)
        rec[f"fused_us_splits_{s}"] = round(timed(fused, args.iters), 1)
        ops.topk_splits(old)
    if args.fallback:
        summary(rec, "fallback_us", t_fb)
        rec["speedup_vs_fallback"] = round(rec["fallback_us"] / us, 2)
        fused()
        fallback()
        torch.cuda.synchronize()
        rec["fallback_same_ids"] = bool(torch.equal(fids, ids))
        rec["fallback_max_abs_score_diff"] = float((fsc - sc).abs().max())
    if not args.no_torch:
        rec["eager_chunk_B"] = cb
        summary(rec, "eager_us", t_eager)
        rec["speedup"] = round(rec["eager_us"] / us, 2)
        # same answer (ties aside: random floats)
        fused()
        ev = torch.cat([o.values for o in eager()])
        torch.cuda.synchronize()
        rec["max_abs_score_diff"] = float((ev - sc).abs().max())
    print(json.dumps(rec), flush=True)

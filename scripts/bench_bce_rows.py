"""Microbenchmark of the shared-negative Linear + BCE / gBCE
(ops.linear_bce_rows, forward + backward with dW / db) against stock eager
torch on the same GPU (gather of the negatives' and the labels' rows, matmul,
F.binary_cross_entropy_with_logits, autograd; its dW is the dense [V, E]
gradient of the gathers) and against ops.linear_xent_rows (sampled softmax) fed
the same labels and negatives. Every one of the N tokens carries a label,
uniform over the items or Zipf(--zipf a)-distributed; the S negatives are
uniform (ops.sample_ids), sorted and deduplicated by ops.bce_candidates. A
label that is also a negative is moved to row V - 1, which is never drawn, so
the eager form needs no mask. One JSON line per NxSxE: time of each (device
events, alternating windows, median / min / max), the HIP call with the
[V, E] + [V] zero fill a training step adds, the time of the positives' stage
(the call minus the same call with an order of -1s, whose waves all exit at
once) with the longest run of equal labels, the time of the negatives' wgrad
(that call minus the call without dW / db), ns per GFLOP and the share of the
f32-MFMA time of the op's four products of 2 N Sv E FLOP at 155 TF."""
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
ap.add_argument("--shapes", default="12800x256x64,12800x4096x64,12800x256x128,12800x4096x128",
                help="comma list of NxSxE")
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--zipf", type=float, default=0.0,
                help="labels Zipf-distributed with this exponent (0: uniform)")
ap.add_argument("--beta", type=float, default=1.0)
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_bce_rows needs a GPU"
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
    if args.zipf > 0:
        p = torch.arange(1, V - 1, device=dev, dtype=torch.float64).pow(-args.zipf)
        labels = torch.multinomial((p / p.sum()).float(), N, replacement=True, generator=g) + 1
    else:
        labels = torch.randint(1, V - 1, (N,), device=dev, generator=g)
    neg = torch.empty(S, dtype=torch.int64, device=dev)
    ops.sample_ids(42, torch.zeros(1, dtype=torch.int64, device=dev), 1, V - 1, neg)
    labels = torch.where(torch.isin(labels, neg), torch.full_like(labels, V - 1), labels)
    negs = torch.empty(S, dtype=torch.int64, device=dev)
    order = torch.empty(N, dtype=torch.int32, device=dev)
    ops.bce_candidates(labels, neg, 0, negs, order)
    no_order = torch.full_like(order, -1)
    rows = negs[negs >= 0]
    Sv = rows.numel()
    cand = torch.empty(N + S, dtype=torch.int64, device=dev)
    target = torch.empty(N, dtype=torch.int64, device=dev)
    ops.xent_candidates(labels, neg, 0, cand, target)
    dH, lv = torch.empty(N, E, device=dev), torch.empty(N, device=dev)
    dW, db, loss = torch.zeros(V, E, device=dev), torch.zeros(V, device=dev), torch.empty(1, device=dev)

    def hip():
        ops.linear_bce_rows(H, W, b, labels, order, negs, args.beta, 0, dH, lv, dW, db, loss=loss)

    def hip_no_pos():
        ops.linear_bce_rows(H, W, b, labels, no_order, negs, args.beta, 0, dH, lv, dW, db,
                            loss=loss)

    def hip_fwd():                              # no dW / db: compact, pass1, merge, loss
        ops.linear_bce_rows(H, W, b, labels, order, negs, args.beta, 0, dH, lv, loss=loss)

    def hip_fill():
        dW.zero_()
        db.zero_()
        hip()

    def xent_rows():
        ops.linear_xent_rows(H, W, b, cand, target, 0.1, dH, lv, dW, db, loss=loss)

    Hr, Wr, br = (t.clone().requires_grad_(True) for t in (H, W, b))
    tgt = torch.zeros(N, Sv + 1, device=dev)
    tgt[:, 0] = 1.0
    wpos = torch.ones(N, Sv + 1, device=dev)
    wpos[:, 0] = args.beta

    def eager():
        Hr.grad = Wr.grad = br.grad = None
        zy = (Hr * Wr[labels]).sum(1) + br[labels]
        z = torch.cat([zy[:, None], Hr @ Wr[rows].t() + br[rows]], 1)
        (torch.nn.functional.binary_cross_entropy_with_logits(z, tgt, weight=wpos, reduction="sum")
         / ((Sv + 1) * N)).backward()

    fns = {"hip": hip, "hip_no_pos": hip_no_pos, "hip_fwd": hip_fwd, "hip_fill": hip_fill,
           "xent_rows": xent_rows}
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
    rec = {"N": N, "S": S, "Sv": Sv, "V": V, "E": E, "zipf": args.zipf, "beta": args.beta,
           "longest_run": int(torch.bincount(labels).max())}
    for k, v in ms.items():
        rec[f"{k}_ms"] = round(statistics.median(v), 4)
        rec[f"{k}_ms_min"] = round(min(v), 4)
        rec[f"{k}_ms_max"] = round(max(v), 4)
    rec["pos_stage_ms"] = round(rec["hip_ms"] - rec["hip_no_pos_ms"], 4)
    rec["neg_wgrad_ms"] = round(rec["hip_no_pos_ms"] - rec["hip_fwd_ms"], 4)
    flops = 4 * 2.0 * N * Sv * E
    rec["hip_ns_per_gflop"] = round(rec["hip_ms"] * 1e6 / (flops / 1e9), 3)
    rec["hip_fraction_of_f32_mfma_peak"] = round(flops / PEAK_F32_MFMA * 1e3 / rec["hip_ms"], 3)
    rec["xent_rows_over_hip"] = round(rec["xent_rows_ms"] / rec["hip_ms"], 2)
    if not args.no_torch:
        rec["eager_over_hip"] = round(rec["eager_ms"] / rec["hip_ms"], 2)
        rec["eager_over_hip_fill"] = round(rec["eager_ms"] / rec["hip_fill_ms"], 2)
        hip_fill()
        eager()
        torch.cuda.synchronize()
        rec["max_abs_dW_diff"] = float((Wr.grad - dW).abs().max())
        rec["max_abs_dH_diff"] = float((Hr.grad - dH).abs().max())
    print(json.dumps(rec), flush=True)

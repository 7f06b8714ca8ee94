"""Microbenchmark of the attention core (ops.attention_fwd + attention_bwd:
csrc/kernels/attention.hip for T <= 64, attention_long.hip above) against
stock eager torch with autograd on the same tensors and the same GPU. One JSON
line per shape: forward + backward time of each (device events, alternating
repeats, median / min / max), their ratio, the largest difference of outputs
and gradients, and the HIP time's share of the f32-MFMA time of its algorithmic
FLOPs (4 B H T^2 d_k forward + 10 B H T^2 d_k backward) at 155 TF.
--causal times the causal kernels (keys j <= i) against eager torch with the
same combined mask; the FLOPs then count the T (T + 1) / 2 visible pairs.
--stream routes every shape with T > 64 through ops.attention_stream_fwd / bwd
(attention_stream.hip; T > 512 always takes them) and, at T <= 512, times the
attention_long.hip family next to it in the same alternation ("long_ms",
"stream_over_long")."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tdfo_amd import ops  # noqa: E402

PEAK_F32_MFMA = 155e12      # FLOP/s

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="256x200x64x2,64x512x64x1",
                help="comma list of BxTxExH")
ap.add_argument("--rate", type=float, default=0.0, help="dropout rate of the HIP op")
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--causal", action="store_true", help="causal attention (keys j <= i)")
ap.add_argument("--stream", action="store_true",
                help="time the streaming kernels at every T > 64 (T > 512 always does)")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_attention needs a GPU"
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
    B, T, E, H = (int(x) for x in spec.split("x"))
    dk = E // H
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B, T, 3 * E, device=dev, generator=g)
    ids = torch.randint(1, 1000, (B, T), device=dev, generator=g)
    ids[:, : T // 4] = 0                         # left padding, as training batches have
    dout = torch.randn(B, T, E, device=dev, generator=g)
    step = torch.tensor([3], dtype=torch.int64, device=dev)
    out, dqkv = torch.empty(B, T, E, device=dev), torch.empty_like(qkv)
    lse = torch.empty(B, H, T, device=dev) if T > ops.ATTN_SHORT_MAXT else None
    ckw = {"causal": True} if args.causal else {}
    future = torch.ones(T, T, dtype=torch.bool, device=dev).triu(1)

    stream = T > ops.ATTN_LONG_MAXT or (args.stream and T > ops.ATTN_SHORT_MAXT)
    delta = torch.empty(B, H, T, device=dev) if stream else None

    def long():
        ops.attention_fwd(qkv, ids, H, args.rate, 1, step, 0, out, lse=lse, **ckw)
        ops.attention_bwd(qkv, ids, dout, H, args.rate, 1, step, 0, dqkv, out=out, lse=lse,
                          **ckw)

    def streaming():
        ops.attention_stream_fwd(qkv, ids, H, args.rate, 1, step, 0, out, lse, **ckw)
        ops.attention_stream_bwd(qkv, ids, dout, H, args.rate, 1, step, 0, dqkv, out, lse, delta,
                                 **ckw)

    hip = streaming if stream else long

    x = qkv.clone().requires_grad_(True)
    mask = (ids != 0).view(B, 1, 1, T)
    res = {}

    def eager():
        x.grad = None
        q, k, v = x.view(B, T, 3, H, dk).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-2, -1) / math.sqrt(dk)).masked_fill(~mask, -1e9)
        if args.causal:
            s = s.masked_fill(future, float("-inf"))
        p = torch.dropout(torch.softmax(s, dim=-1), args.rate, True)
        o = (p @ v).transpose(1, 2).reshape(B, T, E)
        o.backward(dout)
        res["o"] = o

    fns = {"hip": hip}
    if stream and T <= ops.ATTN_LONG_MAXT:
        fns["long"] = long
    if not args.no_torch:
        fns["eager"] = eager
    for fn in fns.values():                      # warm-up: code objects, library algorithms
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.repeats):                # alternate the two in one process
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
    rec = {"B": B, "T": T, "E": E, "H": H, "d_k": dk, "rate": args.rate, "causal": args.causal,
           "kernels": "stream" if stream else "long" if T > ops.ATTN_SHORT_MAXT else "short"}
    for k, v in ms.items():
        rec[f"{k}_ms"] = round(statistics.median(v), 4)
        rec[f"{k}_ms_min"] = round(min(v), 4)
        rec[f"{k}_ms_max"] = round(max(v), 4)
    flops = 14.0 * B * H * (T * (T + 1) / 2 if args.causal else T * T) * dk
    rec["hip_fraction_of_f32_mfma_peak"] = round(flops / PEAK_F32_MFMA * 1e3 / rec["hip_ms"], 3)
    if "long" in fns:
        rec["stream_over_long"] = round(rec["hip_ms"] / rec["long_ms"], 3)
    if not args.no_torch:
        rec["eager_over_hip"] = round(rec["eager_ms"] / rec["hip_ms"], 2)
        if args.rate == 0.0:                     # (eager's dropout draws another mask)
            hip()
            eager()
            torch.cuda.synchronize()
            rec["max_abs_out_diff"] = float((res["o"].detach() - out).abs().max())
            rec["max_abs_grad_diff"] = float((x.grad - dqkv).abs().max())
    print(json.dumps(rec), flush=True)

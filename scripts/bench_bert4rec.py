#!/usr/bin/env python
"""Bert4Rec training throughput on one GPU (reference config: per-device batch
16, T=20, E=16, 2 heads, 2 layers) with a Goodreads-scale vocabulary.
--max-len / --embed-dim / --heads / --layers pick another shape, e.g. the
published BERT4Rec one: --max-len 200 --embed-dim 64 (T > 64 runs the tiled
attention and wide LayerNorm kernels; the fused block covers T <= 64).
--causal trains the next-item (causal attention) model on shifted labels.
--negatives S trains with the sampled-softmax loss over S shared negatives
(0: the full softmax); --loss bce --negatives S with BCE against them, gBCE
with --gbce-t t."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tdfo_amd.models.bert4rec import Bert4RecTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-len", type=int, default=20)
    ap.add_argument("--embed-dim", type=int, default=16)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--causal", action="store_true",
                    help="causal attention, per-position input block, labels = the next item")
    ap.add_argument("--negatives", type=int, default=0,
                    help="sampled softmax over this many shared negatives (0: full softmax)")
    ap.add_argument("--loss", choices=("full", "sampled", "bce"), default=None,
                    help="training loss (default: sampled when --negatives is given, else full)")
    ap.add_argument("--gbce-t", type=float, default=0.0,
                    help="--loss bce: gBCE calibration t in [0, 1] (0: plain BCE)")
    ap.add_argument("--torch-encoder", action="store_true",
                    help="torch reference attention/LayerNorm instead of the HIP kernels")
    a = ap.parse_args()
    if a.torch_encoder:
        import tdfo_amd.models.bert4rec as m
        m.USE_FUSED = False
    dev = "cuda"
    T = a.max_len
    ckw = {"causal": True} if a.causal else {}
    loss = a.loss or ("sampled" if a.negatives else "full")
    if loss != "full":
        ckw.update(loss=loss, num_negatives=a.negatives)
    if loss == "bce":
        ckw.update(gbce_t=a.gbce_t)
    tr = Bert4RecTrainer(a.items, T, a.embed_dim, a.heads, a.layers, a.batch, device=dev, **ckw)
    g = torch.Generator(device=dev).manual_seed(0)
    pool = []
    for _ in range(8):
        if a.causal:                 # windows of T + 1 items: inputs | the next item
            w = torch.randint(1, a.items + 1, (a.batch, T + 1), device=dev, generator=g)
            pool.append((w[:, :-1].contiguous(), w[:, 1:].contiguous()))
            continue
        s = torch.randint(1, a.items + 1, (a.batch, T), device=dev, generator=g)
        m = torch.rand(a.batch, T, device=dev, generator=g) < 0.2
        m[:, -1] = True
        lab = torch.where(m, s, torch.zeros_like(s))
        s = torch.where(m, torch.full_like(s, a.items + 1), s)
        pool.append((s, lab))
    for i in range(a.warmup):
        tr.load_batch(*pool[i % 8])
        tr.step()
    if not a.no_graph:
        tr.capture_graph()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(a.steps):
        tr.load_batch(*pool[i % 8])
        tr.step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t
    print(json.dumps({"model": "bert4rec", "batch": a.batch, "vocab": a.items + 2,
                      "max_len": T, "embed_dim": a.embed_dim, "heads": a.heads,
                      "layers": a.layers, "causal": a.causal,
                      "loss_kind": loss, "negatives": a.negatives, "gbce_t": a.gbce_t,
                      "graph": not a.no_graph, "fused_encoder": not a.torch_encoder, "ms_per_step": round(el / a.steps * 1e3, 4),
                      "sequences_per_sec": round(a.batch * a.steps / el, 1),
                      "loss": round(tr.pop_loss(), 4)}))


if __name__ == "__main__":
    main()

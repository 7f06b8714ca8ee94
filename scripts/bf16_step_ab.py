#!/usr/bin/env python
"""Full training step with fp32 against bf16 embedding tables, through
DLRMTrainer at the headline shapes (Criteo-1TB cardinalities, B = 8192,
D = 128, one GPU): DLRM and DCN-v2, each table type in a fresh trainer,
alternated --repeats times in one process (a trainer is freed before the
next is built: the fp32 tables alone are 90 GiB). Protocol of bench.py's
``measure``: eager warm-up, capture, two replays, a 30 ms burn, then --steps
steps between device synchronisations, a fresh on-device batch per step.
One JSON line per run with ms/step and the HBM the tables and their
optimizer state hold.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tdfo_amd import ops  # noqa: E402
from tdfo_amd.models.dlrm import (CRITEO_1TB_ROWS, MLPERF_MULTIHOT, DLRMConfig,  # noqa: E402
                                  DLRMTrainer)
from tdfo_amd.train.loop import StepLoop, make_source  # noqa: E402


def run(model: str, table_dtype: str, B: int, steps: int, warmup: int) -> dict:
    kw = dict(table_rows=list(CRITEO_1TB_ROWS), table_dtype=table_dtype)
    if model == "dcnv2":
        kw.update(interaction="dcn", pooling=list(MLPERF_MULTIHOT), top=[1024, 1024, 512, 256, 1])
    cfg = DLRMConfig(**kw)
    tr = DLRMTrainer(cfg, B, "cuda:0")
    loop = StepLoop(tr, make_source(cfg.table_rows, B, torch.device("cuda:0"),
                                    cfg.pooling_factors(), 1, 0, kind="fresh"))
    loop.run(warmup - 3)
    tr.capture_graph(warmup=1)
    loop.run(2)
    torch.cuda.synchronize()
    tr.pop_loss()
    ops.burn_us(30e3)
    torch.cuda.synchronize()
    t = time.perf_counter()
    loop.run(steps)
    torch.cuda.synchronize()
    el = time.perf_counter() - t
    st = tr.emb.tw_store
    table_b = st.weight.numel() * st.weight.element_size()
    state_b = sum(s.numel() * s.element_size() for s in (st.state1, st.state2) if s is not None)
    rec = {"model": model, "table_dtype": table_dtype, "batch": B, "steps": steps,
           "ms_per_step": round(el * 1e3 / steps, 4),
           "loss": round(tr.pop_loss() / (steps * B), 4),
           "table_GiB": round(table_b / 2 ** 30, 2), "state_GiB": round(state_b / 2 ** 30, 2),
           "planned_GiB": tr.plan.summary()["mem_GiB"]}
    del loop, tr
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="dlrm,dcnv2")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    for model in args.models.split(","):
        for rep in range(args.repeats):
            for dt in ("fp32", "bf16"):
                rec = run(model, dt, args.batch, args.steps, args.warmup)
                rec["repeat"] = rep
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

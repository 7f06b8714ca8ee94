"""Bert4Rec training driver (reference torchrec/train.py:147-273).

``model_parallel = true`` with more than one rank -> sharded item table
(all-to-all embedding engine, DMP equivalent); otherwise the table is
replicated (DDP equivalent, sparse row-gradient all-gather). Deliberate
differences from the reference, all documented in SURVEY §7.5 terms:
  * Q6: each rank processes ``per_device_train_batch_size`` rows (global =
    x world), the steps-per-epoch count is exact;
  * Q5: no per-step ``loss.item()``; losses are summed on device;
  * Q8: the checkpoint keeps the reference name ``bert4recepoch_{N}_model.pth``
    but only rank 0 writes it (table gathered first);
  * the partial last batch is padded with PAD rows (all labels ignored), so
    every step has the same static shape (hipGraph replay) with identical
    loss/gradients to the unpadded batch;
  * metrics are exact means over users (the reference averages per-batch means).
Log lines follow torchrec/train.py:111,144 (validation before epoch 1 prints
as "Epoch 0": quirk Q16).
"""
from __future__ import annotations

import json
import time
from pathlib import Path
from typing import Dict, List, Optional

import torch

from ..config import Config
from ..data.bert4rec_etl import read_columns
from ..data.columnar import DeviceColumns
from ..models.bert4rec import Bert4RecTrainer
from ..parallel.dist import init_distributed
from ..utils import guarded
from ..utils.checkpoint import bert4rec_ckpt_name, save_state_dict


def _pad_rows(x: torch.Tensor, n: int) -> torch.Tensor:
    if x.shape[0] == n:
        return x
    pad = torch.zeros(n - x.shape[0], *x.shape[1:], dtype=x.dtype, device=x.device)
    return torch.cat([x, pad])


def run(cfg: Config, out_dir: str = ".", device: Optional[str] = None) -> List[Dict]:
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    info = init_distributed(device)
    guarded.rank_preflight(info)          # W > 1: collective self-test, c10d on mismatch
    rank, world, dev, group = info.rank, info.world_size, info.device, info.group
    # objective = next_item: the causal model on the next-item ETL output
    causal = cfg.objective == "next_item"
    root = cfg.data_dir / ("parquet_sasrec" if causal else "parquet_bert4rec")
    train_cols = read_columns(str(root / cfg.train_data))
    eval_cols = read_columns(str(root / cfg.eval_data))
    n_tr, n_ev = len(train_cols["user_id"]), len(eval_cols["user_id"])
    if rank == 0:
        print(f"===== train size: {n_tr:,}, eval size: {n_ev:,} =====")
        print(f"===== num devices: {world} =====\n")
    sm_name = "size_map_sasrec.json" if causal else "size_map_bert4rec.json"
    sm = cfg.size_map or json.loads((cfg.data_dir / sm_name).read_text())
    n_items = int(sm["n_items"])
    if rank == 0:
        print(f"==== vocab size: {n_items + 2:,} ====")
    mode = "dmp" if (cfg.model_parallel and world > 1) else ("ddp" if world > 1 else "local")
    B, EB = cfg.per_device_train_batch_size, cfg.per_device_eval_batch_size
    tr = Bert4RecTrainer(n_items, cfg.max_len, cfg.embed_dim, cfg.n_heads, cfg.n_layers, B,
                         cfg.learning_rate, cfg.weight_decay, dev, mode, group, rank, world,
                         seed=cfg.seed, causal=causal,
                         loss={"sampled_softmax": "sampled"}.get(cfg.train_loss, cfg.train_loss),
                         num_negatives=cfg.num_negatives, gbce_t=cfg.gbce_t)
    data_dev = dev if cfg.data_on_device else torch.device("cpu")
    train = DeviceColumns({"seqs": train_cols["train_interactions"].astype("int64"),
                           "labels": train_cols["labels"].astype("int64")}, data_dev)
    evald = DeviceColumns({"seqs": eval_cols["eval_seqs"].astype("int64"),
                           "cand": eval_cols["candidate_items"].astype("int64")}, data_dev)
    use_graph = cfg.hip_graph and dev.type == "cuda" and world == 1

    def validate(epoch_idx: int) -> Dict[str, float]:
        for b in evald.batches(EB, rank=rank, world_size=world):
            if b["seqs"].shape[0] == 0 and mode != "dmp":
                continue
            tr.eval_batch(b["seqs"].to(dev), b["cand"].to(dev))
            if cfg.eval_full_ranking:
                # the positive (candidate 0) ranked against the whole catalogue
                tr.eval_batch_full(b["seqs"].to(dev), b["cand"][:, 0].to(dev))
        m = tr.pop_metrics()
        if cfg.eval_full_ranking:
            m.update({"full/" + k: v for k, v in tr.pop_metrics_full().items()})
        if rank == 0:
            print(f"\nEpoch {epoch_idx + 1}, metrics {m}\n", flush=True)
        return m

    history = []
    validate(-1)
    for epoch in range(cfg.n_epochs):
        t0 = time.perf_counter()
        steps = 0
        for b in train.batches(B, shuffle=True, seed=cfg.seed, epoch=epoch, rank=rank,
                               world_size=world):
            tr.load_batch(_pad_rows(b["seqs"].to(dev), B), _pad_rows(b["labels"].to(dev), B))
            tr.step()
            steps += 1
            if use_graph and tr.graph is None and steps >= 2:
                tr.capture_graph()
            if cfg.max_steps and steps >= cfg.max_steps:
                break
        if dev.type == "cuda":
            torch.cuda.synchronize()
        el = time.perf_counter() - t0
        loss = tr.pop_loss()
        if rank == 0:
            print(f"\nEpoch {epoch + 1}, average loss {loss}\n", flush=True)
            print(f"[throughput] {steps * B * world / max(el, 1e-9):,.0f} sequences/s", flush=True)
        m = validate(epoch)
        history.append({"epoch": epoch + 1, "loss": loss, **m})
        if cfg.metrics_file and rank == 0:
            with open(cfg.metrics_file, "a") as f:
                f.write(json.dumps(history[-1]) + "\n")
        if (epoch + 1) % 10 == 0:
            sd = tr.state_dict()            # collective in dmp mode
            if rank == 0:
                path = str(Path(out_dir) / bert4rec_ckpt_name(epoch + 1))
                save_state_dict(sd, path)
                print(f"Epoch {epoch + 1} model has been saved to {path}")
    return history

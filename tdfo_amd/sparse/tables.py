"""Embedding table configs and the table-batched embedding store.

``TableBatchedEmbedding`` keeps every table of one embedding width in a single
fused buffer ``[sum(rows), D]`` (one allocation, sized for 288 GB HBM; fp32,
or bf16 with stochastically rounded updates) with per-table row offsets, so one HIP launch serves all tables (the role of
fbgemm's TBE in torchrec/models.py:150-164 of the reference). Its backward is
fused with the optimizer (rowwise-Adagrad / Adam / Adagrad / SGD) and never
materialises a dense embedding gradient (contrast reference quirk Q1, where
JAX all-reduces full-table gradients: jax-flax/train_dp.py:63).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from .. import ops

# Debug bounds checks on every lookup (TDFO_CHECK_IDS=1 or config
# ``debug_checks = true``): out-of-range ids raise instead of reading
# another table's rows (or faulting the GPU).
DEBUG_CHECKS = os.environ.get("TDFO_CHECK_IDS", "0") == "1"


def set_debug_checks(on: bool) -> None:
    global DEBUG_CHECKS
    DEBUG_CHECKS = bool(on)


EMB_OPTIMIZERS = {
    "sgd": ops.EMB_SGD,
    "rowwise_adagrad": ops.EMB_ROWWISE_ADAGRAD,
    "exact_rowwise_adagrad": ops.EMB_ROWWISE_ADAGRAD,
    "adam": ops.EMB_ADAM,
    "adagrad": ops.EMB_ADAGRAD,
    "dense_grad": ops.EMB_DENSE_GRAD,
}


@dataclass
class TableConfig:
    name: str
    num_embeddings: int
    embedding_dim: int
    feature_names: List[str] = field(default_factory=list)
    pooling: str = "sum"            # "sum" | "mean" | "none" (sequence)
    init_range: Optional[float] = None  # uniform(-r, r); default sqrt(1/num_embeddings)

    def __post_init__(self):
        if not self.feature_names:
            self.feature_names = [self.name]

    @property
    def bytes_fp32(self) -> int:
        return self.num_embeddings * self.embedding_dim * 4

    def bytes_at(self, elem_bytes: int) -> int:
        """Row storage at ``elem_bytes`` per element (4: fp32, 2: bf16)."""
        return self.num_embeddings * self.embedding_dim * int(elem_bytes)


# table storage types: name -> (torch dtype, bytes per element)
TABLE_DTYPES = {"fp32": (torch.float32, 4), "bf16": (torch.bfloat16, 2)}
BF16_TABLE_DIMS = (64, 128, 256)
BF16_TABLE_OPTIMIZERS = ("sgd", "rowwise_adagrad", "exact_rowwise_adagrad")


def table_dtype_of(name: str):
    """(torch dtype, element bytes) of a ``table_dtype`` setting."""
    if name not in TABLE_DTYPES:
        raise ValueError(f"table_dtype must be one of {sorted(TABLE_DTYPES)}, got {name!r}")
    return TABLE_DTYPES[name]


@dataclass
class EmbOptimConfig:
    name: str = "rowwise_adagrad"
    lr: float = 0.01
    eps: float = 1e-8
    beta1: float = 0.9
    beta2: float = 0.999
    weight_decay: float = 0.0
    initial_accumulator: float = 0.0
    # bf16 tables: round the updated rows stochastically (counter-based,
    # deterministic) instead of to nearest; ignored for fp32 tables
    stochastic_rounding: bool = True

    @property
    def code(self) -> int:
        return EMB_OPTIMIZERS[self.name]

    def state_floats_per_row(self, dim: int) -> int:
        c = self.code
        if c == ops.EMB_ROWWISE_ADAGRAD:
            return 1
        if c == ops.EMB_ADAGRAD:
            return dim
        if c == ops.EMB_ADAM:
            return 2 * dim
        return 0


class TableBatchedEmbedding:
    """All tables of one width in one fused buffer, with a fused optimizer.

    ``row_counts`` lists the rows this store holds per (local) table — for a
    row-wise shard that is the shard's slice, for a column-wise shard the
    table's full rows at the shard's width.

    ``dtype=torch.bfloat16`` stores the rows in bf16 (optimizer state stays
    fp32): SGD and row-wise Adagrad at D in {64, 128, 256}. The update runs in
    fp32 on the widened rows; the row store rounds stochastically
    (``optim.stochastic_rounding``, default) with 16 random bits per element
    that are a pure function of (``sr_seed``, ``sr_step``, global row,
    column). ``sr_step`` is an int64 device scalar advanced once per update
    inside the update's own launches (graph-replay safe); an apply replayed
    without a new prepare reuses its value. Both are part of ``state_dict``.
    """

    def __init__(self, row_counts: Sequence[int], dim: int, device, optim: EmbOptimConfig,
                 init_ranges: Optional[Sequence[float]] = None, seed: int = 0,
                 dtype=torch.float32, scratch_rows: int = 0):
        """``scratch_rows`` extra rows past the real ones (row ``total_rows``
        onwards): targets for the padding entries of a fixed-capacity
        exchange, updated with junk and never read by a lookup."""
        self.dim = int(dim)
        self.bf16 = dtype == torch.bfloat16
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"embedding tables are stored in float32 or bfloat16, not {dtype}")
        if self.bf16 and (self.dim not in BF16_TABLE_DIMS or
                          optim.name not in BF16_TABLE_OPTIMIZERS):
            raise ValueError(
                f"bf16 embedding tables support optimizers {BF16_TABLE_OPTIMIZERS} at "
                f"embedding_dim in {BF16_TABLE_DIMS}; got {optim.name!r} at D = {self.dim} "
                "(use table_dtype fp32)")
        self.row_counts = [int(r) for r in row_counts]
        self.num_tables = len(self.row_counts)
        self.device = torch.device(device)
        self.optim = optim
        offs = [0]
        for r in self.row_counts:
            offs.append(offs[-1] + r)
        self.total_rows = offs[-1]
        self.row_offset_host = offs[:-1]
        self.row_offset = torch.tensor(offs[:-1], dtype=torch.int64, device=self.device)
        self.scratch_rows = int(scratch_rows)
        nrows = max(1, self.total_rows + self.scratch_rows)
        self.weight = torch.zeros(nrows, self.dim, dtype=dtype, device=self.device)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        for t, r in enumerate(self.row_counts):
            if r == 0:
                continue
            rng = init_ranges[t] if init_ranges is not None else math.sqrt(1.0 / max(1, r))
            if self.bf16:
                # drawn in fp32 and rounded to nearest, a slab at a time
                slab = max(1, (1 << 28) // self.dim)
                for s0 in range(0, r, slab):
                    n = min(slab, r - s0)
                    tmp = torch.empty(n, self.dim, dtype=torch.float32, device=self.device)
                    tmp.uniform_(-rng, rng, generator=gen)
                    self.weight[offs[t] + s0: offs[t] + s0 + n].copy_(tmp)
            else:
                self.weight[offs[t]: offs[t] + r].uniform_(-rng, rng, generator=gen)
        # stochastic-rounding stream of a bf16 store: its seed and update counter
        # (the seed as a host tensor: state_dict hands out the tensor itself, so a
        # loader that copies into the store's tensors restores it too)
        self._sr_seed = torch.tensor((int(seed) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF,
                                     dtype=torch.int64)
        self.sr_step = torch.zeros((), dtype=torch.int64, device=self.device) if self.bf16 else None
        c = optim.code
        self.state1 = self.state2 = None
        if c == ops.EMB_ROWWISE_ADAGRAD:
            self.state1 = torch.full((nrows,), optim.initial_accumulator,
                                     dtype=torch.float32, device=self.device)
        elif c == ops.EMB_ADAGRAD:
            self.state1 = torch.full_like(self.weight, optim.initial_accumulator,
                                          dtype=torch.float32)
        elif c == ops.EMB_ADAM:
            self.state1 = torch.zeros_like(self.weight, dtype=torch.float32)
            self.state2 = torch.zeros_like(self.weight, dtype=torch.float32)
        self.key_bits = ops.key_bits_for(self.total_rows + self.scratch_rows)

    # ------------------------------------------------------------------
    def check_ids(self, indices, offsets, row_offset, T, B):
        """Debug bounds check: every id of virtual table v must be
        in [0, rows of the table whose rows start at row_offset[v]). Host sync;
        skipped during hipGraph capture. Raises IndexError naming the table."""
        if indices.numel() == 0 or (indices.is_cuda and torch.cuda.is_current_stream_capturing()):
            return
        starts = torch.tensor(self.row_offset_host, dtype=torch.int64, device=indices.device)
        counts = torch.tensor(self.row_counts, dtype=torch.int64, device=indices.device)
        ro = row_offset.to(indices.device).view(-1)[:T]
        tab = torch.searchsorted(starts, ro, right=True) - 1          # virtual -> physical
        bag = torch.searchsorted(offsets[: T * B + 1], torch.arange(
            indices.numel(), device=indices.device), right=True) - 1
        v = torch.clamp(bag // B, 0, T - 1)
        lim = counts[tab[v]]
        bad = (indices < 0) | (indices >= lim)
        if bool(bad.any()):
            p = int(bad.nonzero()[0, 0])
            raise IndexError(f"embedding id {int(indices[p])} out of range for table "
                             f"{int(tab[v[p]])} ({int(lim[p])} rows) at position {p}")

    def forward(self, indices, offsets, row_offset, T, B, out, out_off, out_stride, mean=False,
                psw=None, onehot=False, bumps=()):
        """Pooled lookup over ``T`` (virtual) tables of ``B`` bags each
        (``bumps``: step counters the launch advances by one)."""
        if DEBUG_CHECKS:
            self.check_ids(indices, offsets, row_offset, T, B)
        ops.embedding_bag_fwd(self.weight, row_offset, indices, offsets, out_off, T, B, out,
                              out_stride, mean=mean, psw=psw, onehot=onehot, bumps=bumps)

    @property
    def sr_seed(self) -> int:
        return int(self._sr_seed)

    def _sr_args(self):
        if not self.bf16:
            return {}
        return dict(sr_seed=self.sr_seed, sr_counter=self.sr_step,
                    stochastic_rounding=self.optim.stochastic_rounding)

    def backward_update(self, indices, offsets, row_offset, T, B, grad, grad_off, grad_stride,
                        hyper, mean=False, psw=None, dense_grad=None, segsort=0):
        o = self.optim
        ops.embedding_bwd(self.weight, row_offset, indices, offsets, grad_off, T, B, grad,
                          grad_stride, o.code, hyper, state1=self.state1, state2=self.state2,
                          eps=o.eps, beta1=o.beta1, beta2=o.beta2, weight_decay=o.weight_decay,
                          key_bits=self.key_bits, mean=mean, psw=psw, dense_grad=dense_grad,
                          segsort=segsort, **self._sr_args())

    def backward_prepare(self, indices, offsets, row_offset, T, B, grad_off, grad_stride,
                         mean=False, psw=None, segsort=0, bag_len=None):
        """Ids-only half of the backward (keys + sort) into a persistent
        workspace; GPU only (CPU: no-op, backward_apply does everything)."""
        self._prepared = None
        if not self.weight.is_cuda or indices.numel() == 0:
            return
        need = ops.embedding_bwd_workspace(indices.numel(), self.dim)
        if getattr(self, "_bwd_ws", None) is None or self._bwd_ws.numel() < need:
            self._bwd_ws = torch.empty(need, dtype=torch.uint8, device=self.weight.device)
        seg = ops.effective_segsort(segsort)       # fixed here for the apply half too
        ops.embedding_bwd_prepare(self.weight, row_offset, indices, offsets, grad_off, T, B,
                                  grad_stride, self._bwd_ws, key_bits=self.key_bits, mean=mean,
                                  psw=psw, segsort=seg, bag_len=bag_len, sr_counter=self.sr_step)
        self._prepared = (indices.data_ptr(), indices.numel(), T, B)
        self._prepared_segsort = seg

    def backward_apply(self, indices, offsets, row_offset, T, B, grad, grad_off, grad_stride,
                       hyper, mean=False, psw=None, dense_grad=None, segsort=0):
        """Gradient half after backward_prepare (falls back to the fused
        backward_update when nothing was prepared for these ids)."""
        key = (indices.data_ptr(), indices.numel(), T, B)
        if getattr(self, "_prepared", None) != key:
            return self.backward_update(indices, offsets, row_offset, T, B, grad, grad_off,
                                        grad_stride, hyper, mean=mean, psw=psw,
                                        dense_grad=dense_grad, segsort=segsort)
        o = self.optim
        ops.embedding_bwd_apply(self.weight, row_offset, indices, offsets, grad_off, T, B, grad,
                                grad_stride, o.code, hyper, self._bwd_ws, state1=self.state1,
                                state2=self.state2, eps=o.eps, beta1=o.beta1, beta2=o.beta2,
                                weight_decay=o.weight_decay, key_bits=self.key_bits, mean=mean,
                                psw=psw, dense_grad=dense_grad,
                                segsort=self._prepared_segsort, **self._sr_args())
        self._prepared = None

    def table_weight(self, t: int) -> torch.Tensor:
        s = self.row_offset_host[t]
        return self.weight[s: s + self.row_counts[t]]

    def state_dict(self):
        d = {"weight": self.weight}
        if self.state1 is not None:
            d["state1"] = self.state1
        if self.state2 is not None:
            d["state2"] = self.state2
        if self.bf16:
            d["sr_seed"] = self._sr_seed
            d["sr_step"] = self.sr_step
        return d

    def load_state_dict(self, d):
        # (an fp32 checkpoint into a bf16 store rounds to nearest, a bf16 one
        # into an fp32 store widens)
        self.weight.copy_(d["weight"])
        if self.bf16 and "sr_step" in d:
            self._sr_seed.fill_(int(d["sr_seed"]))
            self.sr_step.copy_(d["sr_step"])
        if self.state1 is not None and "state1" in d:
            self.state1.copy_(d["state1"])
        if self.state2 is not None and "state2" in d:
            self.state2.copy_(d["state2"])

"""Bert4Rec ETL (reference torchrec/preprocessing.py) on numpy/pyarrow.

  * users with 20..200 interactions (:12-13,28-43); book ids sorted per user;
  * ids remapped to 1..n (0 = PAD, n_items+1 = MASK) (:46-72);
  * per user: train = all but the last two items, eval = second-to-last,
    test = last (dropped, quirk Q13) (:83-109);
  * static BERT masking with ``mask_prob`` + the last train item always
    masked; labels = original item where masked else PAD (:112-150, Q11);
  * sliding windows of ``max_len`` every ``sliding_step``, PAD-padded
    (:194-226) — vectorised (one gather) instead of the reference's
    per-user Python loop;
  * eval: last ``max_len`` of [PAD.., train items, MASK] (:229-239) and
    101 candidates = [eval item] + 100 popularity-weighted negatives that
    exclude the user's positives (:260-315). We always return exactly 100
    negatives (the reference's set difference can come up short);
  * FILE_NUM=2 parquet parts with list<int32> columns, train parts shuffled
    with seed 42; ``size_map_bert4rec.json {n_users, n_items}`` (:318-375).

``objective="next_item"`` (causal / SASRec-style training) writes
``parquet_sasrec/`` and ``size_map_sasrec.json`` with the same column names:
training windows of ``max_len + 1`` raw train items every ``sliding_step``,
``train_interactions = w[:, :-1]``, ``labels = w[:, 1:]`` (the next item, PAD
past the end; no MASK token, no RNG); eval sequences are the last ``max_len``
train items left-padded, with no MASK slot. The vocabulary keeps its
``n_items + 2`` rows so table shapes match the masked model's.
"""
from __future__ import annotations

import json
import math
import time
from pathlib import Path
from typing import Dict, Tuple

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pyarrow.parquet as pq

MIN_INTERACTIONS = 20
MAX_INTERACTIONS = 200
PAD_ID = 0
EVAL_NEG_NUM = 100
FILE_NUM = 2


def read_sorted(data_dir) -> Tuple[np.ndarray, np.ndarray]:
    tbl = pacsv.read_csv(Path(data_dir) / "goodreads_interactions.csv",
                         convert_options=pacsv.ConvertOptions(
                             column_types={"user_id": pa.int32(), "book_id": pa.int32()},
                             include_columns=["user_id", "book_id"]))
    user = tbl["user_id"].to_numpy()
    book = tbl["book_id"].to_numpy()
    cnt = np.bincount(user)
    keep = (cnt[user] >= MIN_INTERACTIONS) & (cnt[user] <= MAX_INTERACTIONS)
    user, book = user[keep], book[keep]
    order = np.lexsort((book, user))
    return user[order], book[order]


def map_ids(user, book) -> Tuple[np.ndarray, np.ndarray, int, int]:
    uu, ui = np.unique(user, return_inverse=True)
    bu, bi = np.unique(book, return_inverse=True)
    u = (ui + 1).astype(np.int32)
    b = (bi + 1).astype(np.int32)
    n_users, n_items = len(uu), len(bu)
    assert u.min() == 1 and u.max() == n_users and b.min() == 1 and b.max() == n_items
    return u, b, n_users, n_items


def item_popularity(book) -> Tuple[np.ndarray, np.ndarray]:
    cnt = np.bincount(book)
    items = np.nonzero(cnt)[0]
    c = cnt[items]
    order = np.argsort(-c, kind="stable")
    items, c = items[order], c[order]
    return items.astype(np.int64), c / c.sum()


def split(u, b):
    """Rows are sorted by (user, book). Returns per-user train ranges, eval items."""
    n = np.bincount(u)[1:]
    starts = np.zeros(len(n) + 1, dtype=np.int64)
    np.cumsum(n, out=starts[1:])
    train_len = n - 2
    eval_item = b[starts[1:] - 2]
    return starts[:-1], train_len, eval_item


def mask_train(b, starts, train_len, mask_prob, mask_id, rng):
    """Concatenated train items (per user) -> (masked items, labels)."""
    idx = np.concatenate([np.arange(s, s + L) for s, L in zip(starts, train_len)])
    items = b[idx]
    last = np.cumsum(train_len) - 1
    is_last = np.zeros(len(items), dtype=bool)
    is_last[last] = True
    cond = (rng.random(size=len(items), dtype=np.float32) <= mask_prob) | is_last
    masked = np.where(cond, mask_id, items).astype(np.int32)
    labels = np.where(cond, items, PAD_ID).astype(np.int32)
    return masked, labels


def sliding_windows(seq, lens, seq_len, step):
    """Windows of seq_len every `step` over each user's (padded) sequence.
    seq: concatenated per-user sequences with lengths `lens`."""
    starts = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    nwin = (lens + step - 1) // step
    user_of = np.repeat(np.arange(len(lens)), nwin)
    first = np.repeat(np.cumsum(nwin) - nwin, nwin)
    woff = (np.arange(nwin.sum()) - first) * step              # offset inside the user
    pos = woff[:, None] + np.arange(seq_len)[None, :]
    valid = pos < lens[user_of][:, None]
    gidx = starts[user_of][:, None] + np.minimum(pos, lens[user_of][:, None] - 1)
    out = np.where(valid, seq[gidx], PAD_ID).astype(np.int32)
    return user_of, out


def next_item_windows(b, starts, train_len, seq_len, step):
    """Next-item training windows: (user index, inputs [n, seq_len], labels
    [n, seq_len]) with labels[:, t] = the item after inputs[:, t] (PAD at and
    after a user's last train item)."""
    idx = np.concatenate([np.arange(s, s + L) for s, L in zip(starts, train_len)])
    user_of, w = sliding_windows(b[idx], train_len, seq_len + 1, step)
    return user_of, np.ascontiguousarray(w[:, :-1]), np.ascontiguousarray(w[:, 1:])


def eval_seqs_next_item(b, starts, train_len, seq_len):
    """Last seq_len train items per user, left-padded (the last position's
    hidden state is the next-item query: no MASK slot)."""
    n = len(train_len)
    out = np.full((n, seq_len), PAD_ID, dtype=np.int32)
    take = np.minimum(train_len, seq_len)
    for i in range(n):
        k = take[i]
        if k:
            s = starts[i] + train_len[i] - k
            out[i, seq_len - k:] = b[s: s + k]
    return out


def eval_seqs(b, starts, train_len, seq_len, mask_id):
    n = len(train_len)
    out = np.full((n, seq_len), PAD_ID, dtype=np.int32)
    out[:, -1] = mask_id
    take = np.minimum(train_len, seq_len - 1)
    for i in range(n):
        k = take[i]
        if k:
            s = starts[i] + train_len[i] - k
            out[i, seq_len - 1 - k: seq_len - 1] = b[s: s + k]
    return out


def sample_negatives(b, starts, train_len, eval_item, items, probs, rng):
    """100 popularity-weighted negatives per user, excluding train + eval items."""
    n = len(train_len)
    cdf = np.cumsum(probs)
    cdf /= cdf[-1]
    out = np.zeros((n, EVAL_NEG_NUM), dtype=np.int32)
    for i in range(n):
        pos = set(b[starts[i]: starts[i] + train_len[i]].tolist())
        pos.add(int(eval_item[i]))
        chosen, seen = [], set()
        while len(chosen) < EVAL_NEG_NUM:
            k = 2 * (EVAL_NEG_NUM + len(pos))
            draw = items[np.searchsorted(cdf, rng.random(k), side="right").clip(0, len(items) - 1)]
            for x in draw.tolist():
                if x not in pos and x not in seen:
                    seen.add(x)
                    chosen.append(x)
                    if len(chosen) == EVAL_NEG_NUM:
                        break
            if len(seen) + len(pos) >= len(items) and len(chosen) < EVAL_NEG_NUM:
                raise ValueError("not enough items to sample 100 negatives")
        out[i] = chosen
    return out


def _write_parts(write_dir: Path, cols: Dict[str, np.ndarray], prefix: str, verbose=True):
    write_dir.mkdir(parents=True, exist_ok=True)
    n = len(next(iter(cols.values())))
    unit = math.ceil(n / FILE_NUM)
    for i, off in enumerate(range(0, n, unit), start=1):
        t0 = time.perf_counter()
        part = {k: v[off: off + unit] for k, v in cols.items()}
        if prefix == "train":
            perm = np.random.default_rng(42).permutation(len(part["user_id"]))
            part = {k: v[perm] for k, v in part.items()}
        arrays = {}
        for k, v in part.items():
            if v.ndim == 2:
                arrays[k] = pa.FixedSizeListArray.from_arrays(pa.array(v.reshape(-1)), v.shape[1])
                arrays[k] = arrays[k].cast(pa.list_(pa.int32()))
            else:
                arrays[k] = pa.array(v)
        pq.write_table(pa.table(arrays), write_dir / f"{prefix}_part_{i}.parquet")
        if verbose:
            print(f"{prefix} part_{i} finished in {(time.perf_counter() - t0):.2f}s")


OBJECTIVES = ("masked", "next_item")


def _run_etl_next_item(data_dir: Path, max_len: int, sliding_step: int, seed: int, verbose: bool):
    user, book = read_sorted(data_dir)
    if verbose:
        print(f"data size: {len(user):,}")
    u, b, n_users, n_items = map_ids(user, book)
    items, probs = item_popularity(b)
    (data_dir / "size_map_sasrec.json").write_text(
        json.dumps({"n_users": n_users, "n_items": n_items}, indent=4))
    starts, train_len, eval_item = split(u, b)
    uidx, seqs, labs = next_item_windows(b, starts, train_len, max_len, sliding_step)
    train = {"user_id": (uidx + 1).astype(np.int32), "train_interactions": seqs, "labels": labs}
    if verbose:
        print(f"train seq data size: {len(seqs):,}")
    out = data_dir / "parquet_sasrec"
    _write_parts(out, train, "train", verbose)
    ev = eval_seqs_next_item(b, starts, train_len, max_len)
    negs = sample_negatives(b, starts, train_len, eval_item, items, probs,
                            np.random.default_rng(seed))
    cand = np.concatenate([eval_item[:, None].astype(np.int32), negs], 1)
    evald = {"user_id": np.arange(1, n_users + 1, dtype=np.int32), "eval_seqs": ev,
             "candidate_items": cand}
    if verbose:
        print(f"eval seq data size: {len(ev):,}")
    _write_parts(out, evald, "eval", verbose)
    return {"n_users": n_users, "n_items": n_items, "n_train_seqs": len(seqs)}


def run_etl(data_dir, max_len: int = 20, sliding_step: int = 10, mask_prob: float = 0.2,
            seed: int = 42, verbose: bool = True, objective: str = "masked"):
    data_dir = Path(data_dir)
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES}, got {objective!r}")
    if objective == "next_item":
        return _run_etl_next_item(data_dir, max_len, sliding_step, seed, verbose)
    rng = np.random.default_rng(seed)
    user, book = read_sorted(data_dir)
    if verbose:
        print(f"data size: {len(user):,}")
    u, b, n_users, n_items = map_ids(user, book)
    mask_id = n_items + 1
    items, probs = item_popularity(b)
    (data_dir / "size_map_bert4rec.json").write_text(
        json.dumps({"n_users": n_users, "n_items": n_items}, indent=4))
    starts, train_len, eval_item = split(u, b)
    masked, labels = mask_train(b, starts, train_len, mask_prob, mask_id, rng)
    if verbose:
        print(f"total masked ratio: {(masked == mask_id).mean():.4f}")
    uidx, seqs = sliding_windows(masked, train_len, max_len, sliding_step)
    _, labs = sliding_windows(labels, train_len, max_len, sliding_step)
    train = {"user_id": (uidx + 1).astype(np.int32), "train_interactions": seqs, "labels": labs}
    if verbose:
        print(f"train seq data size: {len(seqs):,}")
    out = data_dir / "parquet_bert4rec"
    _write_parts(out, train, "train", verbose)
    ev = eval_seqs(b, starts, train_len, max_len, mask_id)
    negs = sample_negatives(b, starts, train_len, eval_item, items, probs, rng)
    cand = np.concatenate([eval_item[:, None].astype(np.int32), negs], 1)
    evald = {"user_id": np.arange(1, n_users + 1, dtype=np.int32), "eval_seqs": ev,
             "candidate_items": cand}
    if verbose:
        print(f"eval seq data size: {len(ev):,}")
    _write_parts(out, evald, "eval", verbose)
    return {"n_users": n_users, "n_items": n_items, "n_train_seqs": len(seqs)}


def read_columns(pattern: str) -> Dict[str, np.ndarray]:
    """List columns -> [rows, len] int32 arrays."""
    p = Path(pattern)
    files = sorted(p.parent.glob(p.name), key=lambda x: (len(x.name), x.name))
    if not files:
        raise FileNotFoundError(pattern)
    tbl = pa.concat_tables([pq.read_table(f) for f in files])
    out = {}
    for c in tbl.column_names:
        col = tbl[c].combine_chunks()
        if pa.types.is_list(col.type) or pa.types.is_fixed_size_list(col.type):
            flat = col.flatten().to_numpy()
            out[c] = flat.reshape(len(col), -1).astype(np.int32)
        else:
            out[c] = col.to_numpy()
    return out

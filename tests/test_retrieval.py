"""Full-catalogue top-K retrieval and full-ranking eval on CPU: the reference
of the fused search (ops.topk_scores) against a brute-force sort, and the
trainer methods built on it."""
import dataclasses
import json

import pytest
import torch

from tdfo_amd.models.bert4rec import METRIC_NAMES, Bert4RecTrainer, recall_ndcg_sums
from tdfo_amd.models.two_tower import (FEATURES, SIZE_KEYS, TwoTowerConfig, TwoTowerTrainer,
                                       catalogue_columns)
from tdfo_amd.ops import reference as ref
from tests.retrieval_cases import brute_force, exact_case, inner_range, run_topk

SM = {"user": 300, "item": 400, "language": 7, "is_ebook": 2, "format": 9, "publisher": 50,
      "pub_decade": 14}


@pytest.mark.parametrize("E,B,V,K,X,full", [
    (16, 5, 300, 10, 0, True), (16, 9, 300, 10, 20, False), (32, 7, 300, 100, 50, False),
    (64, 6, 130, 128, 20, False), (16, 4, 7, 10, 1, False), (16, 3, 1, 1, 1, False),
    (16, 3, 1, 3, 0, True), (32, 8, 300, 1, 1, False)])
def test_reference_matches_brute_force(monkeypatch, E, B, V, K, X, full):
    """Integer-valued data with heavy ties, exclude, [v_lo, v_hi) and target;
    64-item chunks so the running best crosses many chunk boundaries."""
    monkeypatch.setattr(ref, "TOPK_CHUNK", 64)
    exact_case.cache_clear()
    c = exact_case(E, B, V, K, X, full, seed=1)
    exact_case.cache_clear()
    ids, scores, rank = brute_force(c["q"], c["W"], c["bias"], K, c["v_lo"], c["v_hi"],
                                    c["exclude"], c["target"])
    assert torch.equal(c["ids"], ids)
    assert torch.equal(c["scores"], scores)
    assert torch.equal(c["rank"], rank)
    if V >= 100 and K >= 10:
        assert (c["scores"][:, 1:] == c["scores"][:, :-1]).any(), "the case should hold ties"


def test_reference_without_bias_and_target():
    g = torch.Generator().manual_seed(0)
    q = torch.randint(-2, 3, (4, 16), generator=g).float()
    W = torch.randint(-2, 3, (90, 16), generator=g).float()
    ids, scores, rank = run_topk(q, W, None, 7, 0, 90)
    bi, bs, _ = brute_force(q, W, None, 7, 0, 90)
    assert rank is None and torch.equal(ids, bi) and torch.equal(scores, bs)


def test_fewer_than_k_eligible_pads():
    g = torch.Generator().manual_seed(1)
    q = torch.randn(3, 16, generator=g)
    W = torch.randn(12, 16, generator=g)
    excl = torch.tensor([[1, 2, -1], [3, 3, 3], [-1, -1, -1]])
    ids, scores, _ = run_topk(q, W, torch.zeros(12), 16, *inner_range(12), exclude=excl)
    n = [8, 9, 10]                      # 10 ids in [1, 11) minus the distinct excluded ones
    for b in range(3):
        assert (ids[b, : n[b]] >= 1).all() and (ids[b, : n[b]] < 11).all()
        assert (ids[b, n[b]:] == -1).all()
        assert torch.isinf(scores[b, n[b]:]).all() and (scores[b, n[b]:] < 0).all()
        assert torch.isfinite(scores[b, : n[b]]).all()
    ids, scores, _ = run_topk(q, W, None, 4, 5, 5)           # empty range
    assert (ids == -1).all() and (scores == float("-inf")).all()


def test_target_rank_rules():
    """Ties count against the target, the target itself never does, whether it
    is excluded or outside [v_lo, v_hi) or not."""
    q = torch.ones(1, 16)
    W = torch.zeros(6, 16)
    W[:, 0] = torch.tensor([5.0, 3, 3, 3, 1, 9])            # scores 5 3 3 3 1 9
    for target, excl, lo, hi, want in [
            (2, None, 0, 6, 4),            # 9, 5 and the two other 3s
            (2, [[2, 2]], 0, 6, 4),        # the target in the exclude list: the same
            (2, [[1, 5]], 0, 6, 2),        # excluded items do not count
            (0, None, 1, 5, 0),            # target outside the range: as if eligible
            (4, None, 1, 5, 3),
            (5, None, 0, 5, 0)]:
        e = torch.tensor(excl) if excl is not None else None
        _, _, rank = run_topk(q, W, None, 1, lo, hi, e, torch.tensor([target]))
        assert int(rank) == want, (target, excl, lo, hi)


def _tiny_bert(seed=0, device="cpu"):
    return Bert4RecTrainer(n_items=30, max_len=6, embed_dim=16, n_heads=2, n_layers=1,
                           batch_size=4, device=device, seed=seed)


def _hidden(tr, seqs):
    tr.model.eval()
    tr.item.eval()
    with torch.no_grad():
        return tr.model.encode(tr._embed(seqs), seqs)[:, -1, :]


def test_bert4rec_recommend():
    tr = _tiny_bert()
    g = torch.Generator().manual_seed(0)
    seqs = torch.randint(1, 31, (4, 6), generator=g)
    seqs[0, :2] = 0                                          # left padding
    seqs[:, -1] = 31                                         # MASK at the predicted position
    ids, scores = tr.recommend(seqs, 10)
    assert ids.shape == (4, 10) and scores.shape == (4, 10)
    logits = _hidden(tr, seqs) @ tr.model.out.weight.detach().t() + tr.model.out.bias.detach()
    for b in range(4):
        got = ids[b].tolist()
        assert 0 not in got and 31 not in got and not set(got) & set(seqs[b].tolist())
        assert len(set(got)) == 10
        lg = logits[b].clone()
        lg[0] = lg[31] = float("-inf")
        lg[seqs[b]] = float("-inf")
        want = torch.sort(lg, descending=True, stable=True)
        assert got == want.indices[:10].tolist()
        torch.testing.assert_close(scores[b], want.values[:10], rtol=1e-5, atol=1e-6)
    ids2, _ = tr.recommend(seqs, 10, exclude_seen=False)
    for b in range(4):
        lg = logits[b].clone()
        lg[0] = lg[31] = float("-inf")
        assert ids2[b].tolist() == torch.sort(lg, descending=True, stable=True).indices[:10].tolist()
    ids3, sc3 = tr.recommend(seqs, 40)                       # more than the 30 items
    assert (ids3[:, 30:] == -1).all() and (sc3[:, 30:] == float("-inf")).all()


def test_bert4rec_eval_batch_full_matches_recall_ndcg_sums():
    """candidates = [target | every other eligible item]: the sampled-metric
    formulas on the explicit scores give the full-ranking metrics."""
    tr = _tiny_bert(seed=2)
    g = torch.Generator().manual_seed(3)
    total = torch.zeros(len(METRIC_NAMES), dtype=torch.float64)
    n = 0
    for B in (4, 3):
        seqs = torch.randint(1, 31, (B, 6), generator=g)
        seqs[:, -1] = 31
        targets = torch.randint(1, 31, (B,), generator=g)
        before = tr.metric_sums.clone()
        rank = tr.eval_batch_full(seqs, targets)
        assert torch.equal(tr.metric_sums, before)           # the sampled sums are untouched
        cand = torch.stack([torch.tensor([int(t)] + [v for v in range(1, 31) if v != int(t)])
                            for t in targets])
        logits = _hidden(tr, seqs) @ tr.model.out.weight.detach().t() + tr.model.out.bias.detach()
        sc = logits.gather(1, cand)
        assert torch.equal(rank, (sc[:, 1:] >= sc[:, :1]).sum(1))
        total += recall_ndcg_sums(sc).double()
        n += B
    m = tr.pop_metrics_full()
    assert list(m) == METRIC_NAMES
    for i, k in enumerate(METRIC_NAMES):
        assert m[k] == pytest.approx(float(total[i]) / n, rel=1e-12, abs=0)
    assert all(v == 0.0 for v in tr.pop_metrics_full().values())      # popped


def _tt_batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    d = {f: torch.randint(0, SM[k], (B,), generator=g) for f, k in zip(FEATURES, SIZE_KEYS)}
    d["avg_rating"] = torch.rand(B, generator=g)
    d["num_pages"] = torch.rand(B, generator=g)
    d["label"] = (d["user_id"] % 2 == 0).float()
    return d


def test_two_tower_vectors_reproduce_eval_logits():
    tr = TwoTowerTrainer(TwoTowerConfig(SM, learning_rate=5e-3), 64, "cpu")
    for i in range(3):
        tr.load_batch(_tt_batch(64, i))
        tr.step()
    b = _tt_batch(50, 9)
    tr.load_batch(b, eval_mode=True)
    lg = tr.evaluate_batch().clone()
    u = tr.user_vectors(b["user_id"])
    v = tr.item_vectors(b)
    assert u.shape == (50, 16) and v.shape == (50, 16)
    got = (u * v).sum(1)
    assert float((got - lg).abs().max()) <= 1e-5 * float(lg.abs().max())
    torch.testing.assert_close(tr.user_vectors(b["user_id"], chunk=7), u, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(tr.item_vectors(b, chunk=7), v, rtol=1e-6, atol=1e-7)


def test_two_tower_catalogue_and_recommend():
    tr = TwoTowerTrainer(TwoTowerConfig(SM), 64, "cpu")
    b = _tt_batch(500, 4)
    cat = catalogue_columns(b)
    item = b["item_id"]
    uniq = torch.unique(item)
    assert torch.equal(cat["item_id"], uniq) and "user_id" not in cat and "label" not in cat
    for r in (0, 5, len(uniq) - 1):
        first = int((item == uniq[r]).nonzero()[0])
        for f in ("publisher", "avg_rating", "num_pages"):
            assert cat[f][r] == b[f][first]
    iv = tr.item_vectors(cat)
    users = torch.arange(0, 20)
    excl = torch.full((20, 3), -1)
    ids0, _ = tr.recommend(users, iv, 5)
    excl[:, 0] = ids0[:, 0]
    ids, scores = tr.recommend(users, iv, 5, exclude=excl)
    full = tr.user_vectors(users) @ iv.t()
    for u in range(20):
        lg = full[u].clone()
        lg[ids0[u, 0]] = float("-inf")
        want = torch.sort(lg, descending=True, stable=True)
        assert ids[u].tolist() == want.indices[:5].tolist()
        torch.testing.assert_close(scores[u], want.values[:5], rtol=1e-5, atol=1e-6)


def test_eval_full_ranking_key_leaves_default_records_alone(tmp_path):
    """A recipe epoch with eval_full_ranking=false writes the records of a run
    without the key; true adds full/ metrics and changes nothing else."""
    from tdfo_amd.config import Config
    from tdfo_amd.data.bert4rec_etl import run_etl
    from tdfo_amd.data.goodreads import make_synthetic_raw
    from tdfo_amd.train.bert4rec import run

    raw = tmp_path / "goodreads"
    raw.mkdir()
    make_synthetic_raw(raw, 80, 300, seed=5, mean_inter=30)
    base = Config(data_dir=raw, model="bert4rec", n_epochs=1, max_steps=3,
                  per_device_train_batch_size=32, per_device_eval_batch_size=32,
                  data_on_device=False)
    assert base.eval_full_ranking is False
    run_etl(base.data_dir, base.max_len, base.sliding_step, base.mask_prob, base.seed)
    out = {}
    for name, kw in [("absent", {}), ("off", {"eval_full_ranking": False}),
                     ("on", {"eval_full_ranking": True})]:
        mf = tmp_path / f"{name}.jsonl"
        cfg = dataclasses.replace(base, metrics_file=str(mf), **kw)
        hist = run(cfg, out_dir=str(tmp_path), device="cpu")
        out[name] = (mf.read_bytes(), hist)
    assert out["absent"][0] == out["off"][0] and out["absent"][1] == out["off"][1]
    rec_off = json.loads(out["off"][0].decode().splitlines()[-1])
    rec_on = json.loads(out["on"][0].decode().splitlines()[-1])
    assert not any(k.startswith("full/") for k in rec_off)
    assert {"full/" + k for k in METRIC_NAMES} <= set(rec_on)
    assert {k: v for k, v in rec_on.items() if not k.startswith("full/")} == rec_off
    for k in (10, 20, 50):
        assert 0.0 <= rec_on[f"full/NDCG@{k}"] <= rec_on[f"full/Recall@{k}"] <= 1.0

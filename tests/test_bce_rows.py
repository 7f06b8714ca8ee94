"""BCE / gBCE training on the CPU: the reference op against the fp64 oracle and
against torch's BCE-with-logits, the candidate builder, the config keys and the
Bert4RecTrainer(loss="bce") step."""
import pytest
import torch
import torch.nn.functional as F

from tdfo_amd import config as cfgmod
from tdfo_amd import ops
from tdfo_amd.models.bert4rec import Bert4RecTrainer
from tests import bce_rows_oracle as bo
from tests.test_sasrec import _next_item_batch

# fp32 torch ops against fp64 under rel_err: sums of at most 513 + E rounded
# terms of one sign pattern; a plain fp32 evaluation of the formulas measures
# below 1e-6 at these shapes, the bound leaves ten times that
REF_BOUND = 1e-5


@pytest.mark.parametrize("N,S", bo.SHAPES[:-1])
@pytest.mark.parametrize("beta", bo.BETAS)
def test_reference_matches_fp64_oracle(N, S, beta):
    E, FILL = 16, 1.0
    H, W, b, labels, order, negs = bo.make_case(N, S, E)
    want = bo.oracle_case(N, S, E, bo.V, 1.0, beta)
    dH, lv = torch.ones(N, E), torch.ones(N)
    dW, db = torch.full((bo.V, E), FILL), torch.full((bo.V,), FILL)
    loss, acc = torch.zeros(1), torch.full((1,), 2.0, dtype=torch.float64)
    ops.linear_bce_rows(H, W, b, labels, order, negs, beta, bo.IGNORE, dH, lv, dW, db, loss=loss,
                        loss_acc=acc)
    named = bo.named_rows(labels, negs, bo.V)
    assert bool((dW[~named] == FILL).all()) and bool((db[~named] == FILL).all())
    got = [dH, lv, dW[named], db[named], loss[0]]
    ref = [want[0], want[1], want[2][named], want[3][named], want[4]]
    for k, a, r in zip(bo.NAMES, got, ref):
        e = bo.rel_err(a, r)
        print(f"{k}: {e:.2e}")
        assert e < REF_BOUND, k
    assert abs(float(acc) - 2.0 - float(loss)) < 1e-6


def test_plain_bce_is_torch_bce_with_logits():
    """beta = 1, no holes, hits or ignored tokens: BCE-with-logits over
    [positive | negatives] with targets [1, 0, ...], summed, / ((S + 1) N)."""
    N, S, E, V = 33, 20, 16, 200
    g = torch.Generator().manual_seed(5)
    H, W, b = torch.randn(N, E, generator=g), torch.randn(V, E, generator=g) * 0.3, \
        torch.randn(V, generator=g) * 0.1
    perm = torch.randperm(V, generator=g)
    negs = torch.sort(perm[:S]).values
    labels = perm[S:][torch.randint(0, V - S, (N,), generator=g)]
    dH, lv = torch.empty(N, E), torch.empty(N)
    dW, db, loss = torch.zeros(V, E), torch.zeros(V), torch.zeros(1)
    ops.linear_bce_rows(H, W, b, labels, bo.label_order(labels, V, -100), negs, 1.0, -100, dH, lv,
                        dW, db, loss=loss)
    Hr, Wr, br = (t.clone().requires_grad_(True) for t in (H, W, b))
    rows = torch.cat([labels.view(-1, 1), negs.expand(N, S)], 1)            # [N, 1 + S]
    z = (Hr[:, None, :] * Wr[rows]).sum(-1) + br[rows]
    tgt = torch.zeros(N, S + 1)
    tgt[:, 0] = 1.0
    ref = F.binary_cross_entropy_with_logits(z, tgt, reduction="sum") / ((S + 1) * N)
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) < 1e-6
    torch.testing.assert_close(dH, Hr.grad, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(dW, Wr.grad, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(db, br.grad, rtol=1e-5, atol=1e-7)


def test_candidate_builder():
    labels, neg = bo.candidate_case()
    V = 3002
    neg = neg.clone()
    neg[11], neg[12] = -4, 2 ** 31 + 5                        # out of range: holes
    negs = torch.zeros(neg.numel(), dtype=torch.int64)
    order = torch.zeros(labels.numel(), dtype=torch.int32)
    ops.bce_candidates(labels, neg, 0, negs, order)
    bo.check_candidates(labels, neg, negs, order, V)
    assert int(labels[5]) in negs.tolist()                    # a negative equal to a label stays
    # every label ignored: any permutation, the negatives as before
    before = negs.clone()
    ops.bce_candidates(torch.zeros_like(labels), neg, 0, negs, order)
    bo.check_candidates(torch.zeros_like(labels), neg, negs, order, V)
    assert torch.equal(negs, before)


def test_config_keys():
    f = cfgmod.Config.__dataclass_fields__
    assert f["gbce_t"].default == 0.0 and f["train_loss"].default == "full"
    cfg = cfgmod.from_dict({"model": "bert4rec", "train_loss": "bce", "num_negatives": 64})
    assert cfg.train_loss == "bce" and cfg.num_negatives == 64 and cfg.gbce_t == 0.0
    cfg = cfgmod.from_dict({"model": "bert4rec", "train_loss": "bce", "num_negatives": 64,
                            "gbce_t": 0.75})
    assert cfg.gbce_t == 0.75
    with pytest.raises(ValueError, match="gbce_t"):
        cfgmod.from_dict({"model": "bert4rec", "train_loss": "bce", "num_negatives": 64,
                          "gbce_t": 1.5})
    with pytest.raises(ValueError, match="num_negatives"):
        cfgmod.from_dict({"model": "bert4rec", "train_loss": "bce"})
    with pytest.raises(ValueError, match="bert4rec"):
        cfgmod.from_dict({"model": "dlrm", "train_loss": "bce", "num_negatives": 8})
    with pytest.raises(ValueError, match="bert4rec"):
        cfgmod.from_dict({"model": "dlrm", "gbce_t": 0.5})
    with pytest.raises(ValueError, match="full\\|sampled_softmax"):
        cfgmod.from_dict({"model": "bert4rec", "train_loss": "sampled"})
    with pytest.raises(ValueError, match="num_negatives"):
        Bert4RecTrainer(30, 8, 16, 2, 1, 2, loss="bce", num_negatives=31)
    with pytest.raises(ValueError, match="gbce_t"):
        Bert4RecTrainer(30, 8, 16, 2, 1, 2, loss="bce", num_negatives=8, gbce_t=-0.1)


N_ITEMS, T, E, B, S = 300, 20, 16, 16, 64


def _trainer(**kw):
    return Bert4RecTrainer(N_ITEMS, T, E, 2, 2, B, lr=3e-3, device="cpu", dropout=0.0, seed=3,
                           causal=True, loss="bce", num_negatives=S, **kw)


def test_gbce_beta():
    assert _trainer().beta == 1.0
    alpha = S / (N_ITEMS - 1)
    assert abs(_trainer(gbce_t=0.75).beta - (1 - 0.75 * (1 - alpha))) < 1e-12
    assert abs(_trainer(gbce_t=1.0).beta - alpha) < 1e-12


def test_bce_step_equals_plain_autograd_and_is_reproducible():
    """Two trainers with one seed take bit-identical steps, the negatives
    differ between consecutive steps, and a step equals autograd through the
    loss written with torch ops on the same negatives followed by the same
    flat optimizer."""
    a, b, c = _trainer(gbce_t=0.75), _trainer(gbce_t=0.75), _trainer(gbce_t=0.75)
    g = torch.Generator().manual_seed(1)
    s, l = _next_item_batch(g, B, T, N_ITEMS)
    for t in (a, b):
        t.load_batch(s, l)
        t.step()
    assert torch.equal(a.opt.flat, b.opt.flat) and torch.equal(a.item.weight, b.item.weight)
    assert torch.equal(a.neg, b.neg) and torch.equal(a.negs, b.negs)
    assert int(a.neg.min()) >= 1 and int(a.neg.max()) <= N_ITEMS
    bo.check_candidates(l.reshape(-1), a.neg, a.negs, a.order, a.V)
    # c: the same step by hand
    ops.bump(c._counters)
    c.opt.zero_grads()
    c.model.train()
    c.item.train()
    h = c.model.encode(c._embed(s), s).reshape(-1, E)
    y = l.reshape(-1)
    on = y != 0
    rows = a.negs[a.negs >= 0]
    Wc, bc = c.model.out.weight, c.model.out.bias
    z = h[on] @ Wc[rows].t() + bc[rows]
    zy = (h[on] * Wc[y[on]]).sum(1) + bc[y[on]]
    keep = rows.view(1, -1) != y[on].view(-1, 1)
    per = (c.beta * F.softplus(-zy) + (F.softplus(z) * keep).sum(1)) / (keep.sum(1) + 1)
    loss = per.mean()
    loss.backward()
    c.opt.step()
    assert abs(a.pop_loss() - float(loss.detach())) < 1e-5
    torch.testing.assert_close(a.opt.flat, c.opt.flat, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a.item.weight, c.item.weight, rtol=1e-5, atol=1e-5)
    neg0 = a.neg.clone()
    a.load_batch(*_next_item_batch(g, B, T, N_ITEMS))
    a.step()
    assert not torch.equal(a.neg, neg0)


def test_bce_trainer_learns():
    tr = _trainer()
    s, l = _next_item_batch(torch.Generator().manual_seed(0), B, T, N_ITEMS)
    losses = []
    for i in range(30):
        tr.load_batch(s, l)
        tr.step()
        if i % 10 == 9:
            losses.append(tr.pop_loss())
    assert losses[-1] < losses[0], losses


# ------------------------------------------------ chosen numbers of valid tokens
@pytest.mark.parametrize("E", (16, 256))
def test_nv_builder_and_yardstick(E):
    """``make_case(nv=, hot=)`` yields exactly nv valid tokens and a hot run
    of the asked length, and the fp32 reference has a finite, non-zero row_err
    on every such case."""
    N, S = bo.NV_SHAPE
    todo = [(N, nv, None) for nv in bo.NV] + [(N, bo.HOT_NV, h) for h in bo.HOT]
    todo += [(bo.NV_TWICE_N, nv, None) for nv in bo.NV_TWICE]
    for n, nv, hot in todo:
        labels = bo.make_case(n, S, E, bo.V, 1.0, nv, hot)[3]
        on = bo.valid_tokens(labels, bo.V)
        assert int(on.sum()) == nv
        run = int(torch.bincount(labels[on]).max())
        assert run == (hot if hot is not None else max(1, nv // 3)) or nv < 3
        if n == N:
            for k, v in bo.ref_err(n, S, E, bo.V, 1.0, 0.3, nv, hot).items():
                assert 0 < v < 1e-2, (nv, hot, k, v)


@pytest.mark.parametrize("N,S,E,nv,beta", [(9, 5, 16, 4, 1.0), (40, 33, 64, 17, 0.3),
                                           (20, 129, 128, 20, 0.3)])
def test_bce_oracle_matches_autograd_fp64(N, S, E, nv, beta):
    V = 300
    H, W, b, labels, _, negs = bo.make_case(N, S, E, V, 1.0, nv)
    want = bo.oracle(H, W, b, labels, negs, beta)
    rows = bo.valid_negs(negs, V)
    on = bo.valid_tokens(labels, V)
    assert int(on.sum()) == nv
    Hd, Wd, bd = (t.double().requires_grad_(True) for t in (H, W, b))
    y = labels[on]
    z = Hd[on] @ Wd[rows].t() + bd[rows]
    zy = (Hd[on] * Wd[y]).sum(1) + bd[y]
    keep = (rows.view(1, -1) != y.view(-1, 1)).double()
    per = (beta * F.softplus(-zy) + (F.softplus(z) * keep).sum(1)) / (keep.sum(1) + 1)
    m = per.sum() / nv
    m.backward()
    lossv = torch.zeros(N, dtype=torch.float64)
    lossv[on] = per.detach()
    for k, a, r in zip(bo.NAMES, want, (Hd.grad, lossv, Wd.grad, bd.grad, m.detach())):
        assert bo.rel_err(a, r) < 1e-12, k

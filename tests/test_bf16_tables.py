"""bf16 embedding tables with stochastically rounded updates, on the CPU
reference (the same public path the HIP kernels take on a GPU:
test_gpu_bf16_tables.py). The bounds are derived in tests/bf16_table_cases.py."""
import functools

import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.data.synthetic import SyntheticCriteo
from tdfo_amd.models.dlrm import DLRMConfig, DLRMTrainer
from tdfo_amd.ops import reference as ref
from tdfo_amd.sparse.planner import plan_sharding
from tdfo_amd.sparse.sharded import ShardedEmbeddingBags
from tdfo_amd.sparse.tables import EmbOptimConfig, TableBatchedEmbedding, TableConfig
from tdfo_amd.utils import sharded_ckpt
from tests import bf16_table_cases as bc
from tests import sparse_oracle as so


def _clone(states):
    return [None if s is None else s.clone() for s in states]


# ------------------------------------------------------ 1. rounding primitive
@pytest.mark.parametrize("row0", [0, (1 << 32) + 12345])
def test_stochastic_round_contract(row0):
    """ops.bf16_stochastic_round on CPU tensors (the integer mirror): bf16
    values and NaN / inf keep, every result is a bf16 neighbour, and it is the
    one away from zero exactly when r >= 65536 - low16."""
    x = bc.round_inputs()
    cnt = torch.tensor(7, dtype=torch.int64)
    y = ops.bf16_stochastic_round(x, bc.SR_SEED, cnt, row0=row0)
    assert y.dtype == torch.bfloat16 and int(cnt) == 7
    bc.check_rounding(x, y, bc.SR_SEED, 7, row0)
    # another counter: another stream (same neighbours, other choices)
    y2 = ops.bf16_stochastic_round(x, bc.SR_SEED, torch.tensor(8, dtype=torch.int64), row0=row0)
    bc.check_rounding(x, y2, bc.SR_SEED, 8, row0)
    assert not torch.equal(y.view(torch.int16), y2.view(torch.int16))


def test_round_to_nearest_loses_small_update():
    assert float(torch.tensor(1.0 + 2.0 ** -10).to(torch.bfloat16)) == 1.0


# -------------------------------------------- 2. update vs the float64 oracle
@pytest.mark.parametrize("sr", [False, True], ids=["rn", "sr"])
@pytest.mark.parametrize("path", range(len(so.BWD_PATHS)), ids=[p[0] for p in so.BWD_PATHS])
@pytest.mark.parametrize("opt", bc.BF16_OPTS)
@pytest.mark.parametrize("D", bc.BF16_DIMS)
def test_update_vs_oracle(D, opt, path, sr):
    c = bc.rounded(so.bwd_case(D, path))
    st = so.bwd_states(c, opt)
    kw = bc.sr_kw("cpu", sr)
    got = so.run_bwd(c, opt, "cpu", _clone(st), **kw)
    bc.check_bwd(got, c, st, bc.bwd_exact(c, opt, st), sr)
    assert int(kw["sr_counter"]) == 1


@pytest.mark.parametrize("opt", bc.BF16_OPTS)
def test_skipped_step_changes_nothing(opt):
    c = bc.rounded(so.bwd_case(128, 1))
    st = so.bwd_states(c, opt)
    lr, step = so.HYPER
    hyper = torch.tensor([lr, step, 0.5, 1.0])
    got = so.run_bwd(c, opt, "cpu", _clone(st), hyper=hyper, **bc.sr_kw("cpu", True))
    bc.check_bwd(got, c, st, None, True)
    hyper = torch.tensor([lr, step, 0.5, 0.0])
    got = so.run_bwd(c, opt, "cpu", _clone(st), hyper=hyper, **bc.sr_kw("cpu", True))
    bc.check_bwd(got, c, st, bc.bwd_exact(c, opt, st, hyper), True)


def test_unsupported_combinations_raise():
    c = bc.rounded(so.bwd_case(64, 0))
    st = so.bwd_states(c, ops.EMB_ADAM)
    with pytest.raises(ValueError, match="EMB_SGD and EMB_ROWWISE_ADAGRAD"):
        so.run_bwd(c, ops.EMB_ADAM, "cpu", _clone(st))
    for name, dim in (("adam", 128), ("adagrad", 64), ("rowwise_adagrad", 32),
                      ("sgd", 512)):
        with pytest.raises(ValueError, match="bf16 embedding tables support"):
            TableBatchedEmbedding([10], dim, "cpu", EmbOptimConfig(name), dtype=torch.bfloat16)
    st = TableBatchedEmbedding([10], 64, "cpu", EmbOptimConfig("rowwise_adagrad"),
                               dtype=torch.bfloat16)
    assert st.weight.dtype == torch.bfloat16 and st.state1.dtype == torch.float32
    assert TableConfig("t", 10, 64).bytes_at(2) * 2 == TableConfig("t", 10, 64).bytes_fp32


# ------------------------------------------- 3. SR makes progress, RN does not
def test_sr_makes_progress_rn_does_not():
    bc.check_progress(bc.run_progress("cpu", True))
    st = bc.run_progress("cpu", False)
    assert bool((st.weight.float() == 1.0).all())
    assert int(st.sr_step) == 64


# ------------------------------------------------------------ 4. determinism
def _det_store(seed):
    st = TableBatchedEmbedding([300, 40], 64, "cpu", EmbOptimConfig("rowwise_adagrad", lr=0.05),
                               seed=seed, dtype=torch.bfloat16)
    st.weight.copy_(torch.randn(340, 64, generator=torch.Generator().manual_seed(1)))
    return st


def _det_update(st, k):
    g = torch.Generator().manual_seed(100 + k)
    B, T, D = 64, 2, 64
    idx = torch.cat([torch.randint(0, 300, (B,), generator=g), torch.randint(0, 40, (B,), generator=g)])
    offs = torch.arange(T * B + 1, dtype=torch.int64)
    grad = torch.randn(B, T * D, generator=g) * 0.1
    st.backward_update(idx, offs, st.row_offset, T, B, grad, torch.tensor([0, D]), T * D,
                       torch.tensor([0.05, float(k + 1)]))


def _bits(st):
    return st.weight.view(torch.int16).clone()


def test_determinism_and_resume():
    a, b, other = _det_store(5), _det_store(5), _det_store(6)
    saved = None
    for k in range(5):
        for st in (a, b, other):
            _det_update(st, k)
        if k == 1:
            saved = {n: v.clone() for n, v in a.state_dict().items()}
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(a.state1, b.state1)
    assert not torch.equal(_bits(a), _bits(other))
    assert set(saved) == {"weight", "state1", "sr_seed", "sr_step"} and int(saved["sr_step"]) == 2
    r = _det_store(99)                    # another seed: the checkpoint's stream takes over
    r.load_state_dict(saved)
    for k in range(2, 5):
        _det_update(r, k)
    assert torch.equal(_bits(r), _bits(a)) and torch.equal(r.state1, a.state1)
    assert int(r.sr_step) == 5 and r.sr_seed == a.sr_seed


def test_checkpoint_dtype_conversion():
    f = TableBatchedEmbedding([50], 64, "cpu", EmbOptimConfig("sgd"), seed=1)
    h = TableBatchedEmbedding([50], 64, "cpu", EmbOptimConfig("sgd"), seed=2, dtype=torch.bfloat16)
    h.load_state_dict(f.state_dict())               # fp32 -> bf16: nearest
    assert torch.equal(h.weight, f.weight.to(torch.bfloat16))
    f2 = TableBatchedEmbedding([50], 64, "cpu", EmbOptimConfig("sgd"), seed=3)
    f2.load_state_dict(h.state_dict())              # bf16 -> fp32: widens
    assert torch.equal(f2.weight, h.weight.float())


# ---------------------------------------------------------------- 5. forward
@pytest.mark.parametrize("mode", so.FWD_MODES, ids=lambda m: f"{m[0]}-psw{int(m[1])}-mean{int(m[2])}")
def test_forward_equals_fp32_table_of_same_values(mode):
    dt, use_psw, mean = mode
    c = bc.rounded(so.fwd_multihot_case(64))
    wide = dict(c, W=c["W"].float())
    odt = torch.bfloat16 if dt == "bf16" else torch.float32
    assert torch.equal(so.run_fwd(c, "cpu", odt, use_psw, mean),
                       so.run_fwd(wide, "cpu", odt, use_psw, mean))


# ---------------------------------------------------------------- 6. planner
def test_planner_element_size():
    tabs = [TableConfig("big", 1_000_000, 128)]
    opt = EmbOptimConfig("rowwise_adagrad")
    kw = dict(hbm_bytes=400_000_000, reserve_frac=0.0)
    with pytest.raises(MemoryError):                 # 516 B / row: 516 MB
        plan_sharding(tabs, 1, opt, **kw)
    p = plan_sharding(tabs, 1, opt, table_dtype="bf16", **kw)
    assert p.mem_bytes == [1_000_000 * 260] and p.kind_of(0) == "table_wise"
    with pytest.raises(ValueError, match="table_dtype"):
        plan_sharding(tabs, 1, opt, table_dtype="fp16", **kw)
    # fp32 plans: the default and the explicit setting agree, figure for figure
    tabs = [TableConfig(f"t{i}", r, 64) for i, r in enumerate([5_000_000, 300, 70_000, 2_000_000])]
    for W, strat in ((1, "auto"), (4, "auto"), (4, "column_wise"), (4, "row_wise"),
                     (2, "data_parallel")):
        a = plan_sharding(tabs, W, opt, strategy=strat, batch_per_rank=1024)
        b = plan_sharding(tabs, W, opt, strategy=strat, batch_per_rank=1024, table_dtype="fp32")
        assert a == b
        h = plan_sharding(tabs, W, opt, strategy=strat, batch_per_rank=1024, table_dtype="bf16")
        assert all(x < y for x, y in zip(h.mem_bytes, a.mem_bytes) if y)
    assert plan_sharding(tabs, 1, opt).mem_bytes == [sum(t.num_embeddings for t in tabs) * 4 * 65]


def test_bf16_row_wise_plan_is_refused():
    tabs = [TableConfig("a", 1000, 64), TableConfig("b", 64, 64)]
    opt = EmbOptimConfig("rowwise_adagrad")
    plan = plan_sharding(tabs, 2, opt, strategy="row_wise", batch_per_rank=32)
    with pytest.raises(NotImplementedError, match="table-wise and column-wise.*a row_wise"):
        ShardedEmbeddingBags(tabs, plan, 0, 32, [1, 1], "cpu", opt, table_dtype="bf16")
    plan = plan_sharding(tabs, 1, opt, batch_per_rank=32)
    eng = ShardedEmbeddingBags(tabs, plan, 0, 32, [1, 1], "cpu", opt, table_dtype="bf16")
    assert eng.tw_store.weight.dtype == torch.bfloat16


# -------------------------------------------------------------- 7. DLRM-tiny
def _tiny(table_dtype, seed, interaction="dot"):
    return DLRMConfig(embedding_dim=64, table_rows=[1000, 50, 300, 20000, 7], bottom=[64, 64],
                      top=[64, 32, 1], dense_lr=1e-2, emb_lr=0.05, table_dtype=table_dtype,
                      seed=seed, interaction=interaction, dcn_rank=64)


@functools.lru_cache(maxsize=None)
def _tiny_loss(table_dtype, seed, steps=120, tail=30):
    cfg = _tiny(table_dtype, seed)
    tr = DLRMTrainer(cfg, 128, "cpu")
    data = SyntheticCriteo(cfg.table_rows, 128, device="cpu", seed=1)
    for i in range(steps):
        if i == steps - tail:
            tr.pop_loss()
        tr.load_batch(*data.next())
        tr.step()
    return tr.pop_loss() / (tail * 128)


def test_dlrm_tiny_bf16_loss_parity():
    """Mean loss of the last 30 of 120 steps, bf16 tables against fp32 tables,
    seeds 0..4 (model initialisation; the data stream is the same). Allowed
    gap of the five-seed means: the max - min spread of the five fp32 runs.
    Measured on the CPU reference: fp32 runs 0.5597 .. 0.5830 (mean 0.5722,
    spread 0.0233); bf16 runs 0.5614 .. 0.5762 (mean 0.5702, gap 0.0019)."""
    f = [_tiny_loss("fp32", s) for s in range(5)]
    h = [_tiny_loss("bf16", s) for s in range(5)]
    spread = max(f) - min(f)
    gap = abs(sum(h) / 5 - sum(f) / 5)
    print(f"fp32 {f} spread {spread:.5f}; bf16 {h} gap {gap:.5f}")
    assert all(x == x for x in h)
    assert gap <= spread, (gap, spread)


@pytest.mark.parametrize("interaction", ["dot", "dcn"])
def test_dlrm_tiny_bf16_trains_and_checkpoints(tmp_path, interaction):
    cfg = _tiny("bf16", 0, interaction)
    tr = DLRMTrainer(cfg, 128, "cpu")
    data = SyntheticCriteo(cfg.table_rows, 128, device="cpu", seed=1)
    w0 = tr.emb.tw_store.weight.clone()
    for _ in range(4):
        tr.load_batch(*data.next())
        tr.step()
    st = tr.emb.tw_store
    assert st.weight.dtype == torch.bfloat16 and st.state1.dtype == torch.float32
    assert int(st.sr_step) == 4 and not torch.equal(st.weight, w0)
    # sharded checkpoint: dtype, bits and the counter come back
    sharded_ckpt.save(tr, str(tmp_path / "ck"), 4, 0, 1, {"model": "dlrm"})
    tr2 = DLRMTrainer(_tiny("bf16", 7, interaction), 128, "cpu")
    assert sharded_ckpt.load(tr2, str(tmp_path / "ck"), 0, 1, expect_meta={"model": "dlrm"}) == 4
    st2 = tr2.emb.tw_store
    assert st2.weight.dtype == torch.bfloat16 and int(st2.sr_step) == 4
    assert torch.equal(st2.weight.view(torch.int16), st.weight.view(torch.int16))
    assert torch.equal(st2.state1, st.state1)
    # ... and widen into an fp32 model
    tr3 = DLRMTrainer(_tiny("fp32", 7, interaction), 128, "cpu")
    sharded_ckpt.load(tr3, str(tmp_path / "ck"), 0, 1)
    assert torch.equal(tr3.emb.tw_store.weight, st.weight.float())
    # flat state (the in-memory / legacy checkpoint path)
    flat = {k: v.clone() for k, v in tr.flat_state().items()}
    assert flat["emb.tw.weight"].dtype == torch.bfloat16 and int(flat["emb.tw.sr_step"]) == 4
    tr4 = DLRMTrainer(_tiny("bf16", 9, interaction), 128, "cpu")
    tr4.load_flat_state(flat)
    assert tr4.emb.tw_store.sr_seed == st.sr_seed and int(tr4.emb.tw_store.sr_step) == 4


def test_config_key():
    from tdfo_amd import config as cfgmod

    base = cfgmod.Config.__dataclass_fields__
    assert base["table_dtype"].default == "fp32"
    cfg = cfgmod.from_dict({"model": "dlrm", "table_dtype": "bf16"})
    assert cfg.table_dtype == "bf16"
    with pytest.raises(ValueError, match="fp32\\|bf16"):
        cfgmod.from_dict({"model": "dlrm", "table_dtype": "fp16"})
    with pytest.raises(ValueError, match="dlrm and dcnv2"):
        cfgmod.from_dict({"model": "two_tower", "table_dtype": "bf16"})
    cfg = cfgmod.apply_overrides(cfgmod.from_dict({"model": "dcnv2"}), ["table_dtype=bf16"])
    from tdfo_amd.train.dlrm import dlrm_config

    assert dlrm_config(cfg, "auto").table_dtype == "bf16"

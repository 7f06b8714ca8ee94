"""bf16 embedding tables on the HIP kernels (run on MI355X): the lookup from
2-byte rows, the stochastically rounded update on every sort / combine path,
the rounding primitive against its Python mirror, graph replay and the DLRM /
DCN-v2 trainers. Cases and bounds: tests/bf16_table_cases.py (the cached
shapes of tests/sparse_oracle.py with the table rounded to bf16)."""
import functools

import pytest
import torch

from tdfo_amd import ops
from tests import bf16_table_cases as bc
from tests import sparse_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _clone(states):
    return [None if s is None else s.clone() for s in states]


# ---------------------------------------------------------------- 1. forward
@functools.lru_cache(maxsize=None)
def _fwd_oracle(D, use_psw, mean):
    c = bc.rounded(so.fwd_multihot_case(D))
    return so.embedding_bag_fwd(c["W"].float(), c["ro"], c["idx"], c["offs"], c["out_off"], c["T"],
                                c["B"], c["out_stride"], psw=c["psw"] if use_psw else None,
                                mean=mean)


@pytest.mark.parametrize("mode", so.FWD_MODES, ids=lambda m: f"{m[0]}-psw{int(m[1])}-mean{int(m[2])}")
@pytest.mark.parametrize("D", bc.BF16_DIMS)
def test_fwd_multihot(D, mode):
    """emb_fwd_kernel from bf16 rows against the float64 oracle of the rounded
    table (the bound covers fp32 accumulation and a bf16 output), and bit for
    bit what the fp32 kernel gives from the same values."""
    dt, use_psw, mean = mode
    c = bc.rounded(so.fwd_multihot_case(D))
    out = so.run_fwd(c, DEV, DT[dt], use_psw, mean)
    so.check_fwd(out, _fwd_oracle(D, use_psw, mean))
    assert torch.equal(out, so.run_fwd(dict(c, W=c["W"].float()), DEV, DT[dt], use_psw, mean))


@pytest.mark.parametrize("large", [False, True], ids=["small", "grid-cap"])
@pytest.mark.parametrize("D", bc.BF16_DIMS)
def test_fwd_onehot(D, large):
    c = bc.rounded(so.fwd_onehot_case(D, large))
    dt = torch.bfloat16 if D <= 64 else torch.float32
    a = so.run_fwd(c, DEV, dt, True, False, onehot=True)
    b = so.run_fwd(c, DEV, dt, True, False, onehot=False)
    assert torch.equal(a, b)
    so.check_fwd(a, so.fwd_onehot_oracle(dict(c, W=c["W"].float()), True, DEV))


@pytest.mark.parametrize("D", bc.BF16_DIMS)
def test_fwd_integer_rows_exact(D):
    """Integer rows in [-4, 4] and bag lengths from FWD_LENS: every sum is
    exact in fp32, so the fp32 output equals the float64 oracle bit for bit."""
    c = dict(so.fwd_multihot_case(D))
    g = torch.Generator().manual_seed(D)
    c["W"] = torch.randint(-4, 5, c["W"].shape, generator=g).to(torch.bfloat16)
    out = so.run_fwd(c, DEV, torch.float32, False, False)
    exact, _, _, written = so.embedding_bag_fwd(c["W"].float(), c["ro"], c["idx"], c["offs"],
                                                c["out_off"], c["T"], c["B"], c["out_stride"])
    got = out.cpu().double().view(exact.shape)
    assert torch.equal(got[written], exact[written])
    assert bool((got[~written] == so.SENTINEL).all())


# ------------------------------------------------------ 2. rounding primitive
def test_stochastic_round_equals_mirror():
    x = bc.round_inputs(128)
    row0 = (1 << 32) + 12345
    for counter in (0, 7):
        cnt = torch.tensor(counter, dtype=torch.int64, device=DEV)
        y = ops.bf16_stochastic_round(x.to(DEV), bc.SR_SEED, cnt, row0=row0).cpu()
        want = ops.bf16_stochastic_round(x, bc.SR_SEED, torch.tensor(counter), row0=row0)
        nan = torch.isnan(x)
        assert torch.equal(y.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
        assert bool(torch.isnan(y.float()[nan]).all())
        bc.check_rounding(x, y, bc.SR_SEED, counter, row0)
        assert int(cnt) == counter                     # read only


# ------------------------------------------------ 3. update against the oracle
SHAPES = ("general-f32-sum", "general-bf16-psw-mean", "onehot256-f32", "onehot250-bf16",
          "fixed-len", "long", "onehot256-key40", "onehot250-key40", "multirun")


def _run_shape(D, opt, shape, sr, counter=0, **over):
    """-> (case, states, result) of one update on the GPU."""
    kw = bc.sr_kw(DEV, sr, counter)
    if shape == "fixed-len":
        c = bc.rounded(so.bwd_fixed_len_case(D))
        st = so.bwd_states(c, opt)
        return c, st, bc.run_split(c, opt, DEV, _clone(st), bag_len=c["bag_len"].to(DEV), **kw)
    if shape == "long":
        c = bc.rounded(so.bwd_long_case(D))
    elif shape == "multirun":
        c = bc.rounded(so.bwd_multirun_case(D))
        kw["segsort"] = 2
    elif shape.endswith("key40"):
        c = bc.rounded(so.bwd_onehot_case(D, int(shape[6:9])))
        kw.update(segsort=1, key_bits=40)
    else:
        p = SHAPES.index(shape)
        c = bc.rounded(so.bwd_case(D, p))
        kw["segsort"] = 1 if so.BWD_PATHS[p][2] else 0
    kw.update(over)
    st = so.bwd_states(c, opt)
    return c, st, so.run_bwd(c, opt, DEV, _clone(st), **kw)


@pytest.mark.parametrize("sr", [False, True], ids=["rn", "sr"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("opt", bc.BF16_OPTS)
@pytest.mark.parametrize("D", bc.BF16_DIMS)
def test_update_vs_oracle(D, opt, shape, sr):
    """Every sort and combine path of the update on bf16 rows: ragged bags on
    the radix sort (fp32 sums; bf16 gradients with psw and mean), the per-table
    sort with the in-kernel (B = 256) and the separate (B = 250) combine,
    prepare / apply with ``bag_len``, the long-run combine, 64-bit keys and the
    run merge. Nearest-even and stochastic stores within their bounds, no
    element exempt; untouched rows keep their bits."""
    c, st, got = _run_shape(D, opt, shape, sr)
    bc.check_bwd(got, c, st, bc.bwd_exact(c, opt, st), sr)


@pytest.mark.parametrize("opt", bc.BF16_OPTS)
def test_skipped_step_writes_nothing(opt):
    lr, step = so.HYPER
    for shape in ("general-bf16-psw-mean", "onehot256-f32"):
        hyper = torch.tensor([lr, step, 0.5, 1.0])
        c, st, got = _run_shape(128, opt, shape, True, hyper=hyper)
        bc.check_bwd(got, c, st, None, True)


def test_unsupported_combinations_raise():
    c = bc.rounded(so.bwd_case(64, 0))
    for opt in (ops.EMB_ADAM, ops.EMB_ADAGRAD, ops.EMB_DENSE_GRAD):
        st = so.bwd_states(c, opt)
        with pytest.raises(RuntimeError, match="EMB_SGD and EMB_ROWWISE_ADAGRAD"):
            so.run_bwd(c, opt, DEV, _clone(st))
    for D in (16, 32, 512):
        c = bc.rounded(so.bwd_case(D, 2))
        with pytest.raises(RuntimeError, match=r"D in \{64, 128, 256\}"):
            so.run_bwd(c, ops.EMB_SGD, DEV, [None, None, None])
        with pytest.raises(RuntimeError, match=r"D in \{64, 128, 256\}"):
            so.run_fwd(bc.rounded(so.fwd_multihot_case(D)), DEV, torch.float32, False, False)
    W = torch.zeros(8, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.embedding_dense_update(W, torch.zeros(8, 64, device=DEV), 8, ops.EMB_SGD,
                                   torch.tensor([0.1, 1.0], device=DEV))
    c = bc.rounded(so.bwd_case(64, 0))
    with pytest.raises(RuntimeError, match="sr_counter"):
        so.run_bwd(c, ops.EMB_SGD, DEV, [None, None, None], stochastic_rounding=True)


# --------------------------------------------------- 4. path independence
@pytest.mark.parametrize("opt", bc.BF16_OPTS)
def test_paths_write_the_same_bits(opt):
    """D = 128, stochastic rounding, one seed and counter: the random bits are
    a function of (seed, counter, row, column) only."""
    D = 128
    # fused vs prepare / apply (radix sort, psw, mean, bf16 gradient)
    c, st, fused = _run_shape(D, opt, "general-bf16-psw-mean", True, counter=4)
    split = bc.run_split(c, opt, DEV, _clone(st), **bc.sr_kw(DEV, True, 4))
    assert so.same_bits(fused, split)
    # per-table LDS sort vs device-wide radix sort; 32- vs 64-bit keys
    for shape in ("onehot250-bf16", "onehot256-f32"):
        c, st, seg = _run_shape(D, opt, shape, True, counter=4)
        old = ops.embedding_segsort(0)
        try:
            _, _, radix = _run_shape(D, opt, shape, True, counter=4)
        finally:
            ops.embedding_segsort(old)
        assert so.same_bits(seg, radix)
        _, _, wide = _run_shape(D, opt, shape, True, counter=4, key_bits=40)
        assert so.same_bits(seg, wide)
    c, st, narrow = _run_shape(D, opt, "general-f32-sum", True, counter=4)
    _, _, wide = _run_shape(D, opt, "general-f32-sum", True, counter=4, key_bits=40)
    assert so.same_bits(narrow, wide)
    # another counter: other bits
    _, _, other = _run_shape(D, opt, "general-f32-sum", True, counter=5)
    assert not torch.equal(other["W"], narrow["W"])


def test_inkernel_combine_on_and_off():
    """TDFO_EMB_INKERNEL_COMBINE is read when the library loads: one fresh
    child process each way, the same bits."""
    assert bc.ikc_child(1) == bc.ikc_child(0)


@pytest.mark.parametrize("opt", bc.BF16_OPTS)
def test_nearest_even_vs_cpu_reference(opt):
    """The kernels and the CPU reference both round an fp32 value within tol
    of the float64 result to nearest, so they are at most one bf16 spacing
    + tol apart: |RN(a) - RN(b)| <= |a - b| + ulp/2 + ulp/2."""
    for shape in ("general-bf16-psw-mean", "onehot250-bf16"):
        c, st, got = _run_shape(128, opt, shape, False)
        bc.check_bwd(got, c, st, bc.bwd_exact(c, opt, st), False)
        cpu = so.run_bwd(c, opt, "cpu", _clone(st), **bc.sr_kw("cpu", False))
        a, b = got["W"].cpu().double(), cpu["W"].double()
        tol = 1e-4 * max(1.0, float(b.abs().max()))
        assert bool(((a - b).abs() <= bc.bf16_ulp(b.abs() + tol) + tol).all())
        if got["s1"] is not None:
            assert float((got["s1"].cpu() - cpu["s1"]).abs().max()) < 1e-3


# ------------------------------------------------------------ 5. progress
def test_sr_makes_progress_rn_does_not():
    bc.check_progress(bc.run_progress(DEV, True))
    st = bc.run_progress(DEV, False)
    assert bool((st.weight.float() == 1.0).all())
    # the kernels and the CPU reference draw the same bits
    a, b = bc.run_progress(DEV, True, updates=3), bc.run_progress("cpu", True, updates=3)
    assert torch.equal(a.weight.cpu().view(torch.int16), b.weight.view(torch.int16))


# ---------------------------------------------------------- 6. graph replay
def _graph_store():
    from tdfo_amd.sparse.tables import EmbOptimConfig, TableBatchedEmbedding

    return TableBatchedEmbedding([300, 40, 5000], 128, DEV,
                                 EmbOptimConfig("rowwise_adagrad", lr=0.05), seed=4,
                                 dtype=torch.bfloat16)


def test_graph_replay_advances_the_counter():
    T, B, D = 3, 256, 128
    g = torch.Generator().manual_seed(9)
    idx = torch.cat([torch.randint(0, r, (B,), generator=g) for r in (300, 40, 5000)]).to(DEV)
    offs = torch.arange(T * B + 1, dtype=torch.int64, device=DEV)
    off = torch.tensor([0, D, 2 * D], dtype=torch.int64, device=DEV)
    hyper = torch.tensor([0.05, 1.0], device=DEV)
    a, b = _graph_store(), _graph_store()
    outs = {id(s): torch.zeros(B, T * D, dtype=torch.bfloat16, device=DEV) for s in (a, b)}

    def step(st):
        out = outs[id(st)]
        st.forward(idx, offs, st.row_offset, T, B, out, off, T * D, onehot=True)
        st.backward_prepare(idx, offs, st.row_offset, T, B, off, T * D, segsort=1)
        st.backward_apply(idx, offs, st.row_offset, T, B, out, off, T * D, hyper, segsort=1)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(a)                                        # warm-up: the workspace exists
    torch.cuda.current_stream().wait_stream(s)
    step(b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(a)
    for _ in range(3):
        graph.replay()
        step(b)
    torch.cuda.synchronize()
    assert int(a.sr_step) == 4 and int(b.sr_step) == 4
    assert torch.equal(a.weight.view(torch.int16), b.weight.view(torch.int16))
    assert torch.equal(a.state1, b.state1)
    assert torch.equal(outs[id(a)], outs[id(b)])


# ------------------------------------------------------------ 7. trainers
@pytest.mark.parametrize("interaction", ["dot", "dcn"])
def test_trainer_bf16_tables(interaction):
    from tdfo_amd.data.synthetic import SyntheticCriteo
    from tdfo_amd.models.dlrm import DLRMConfig, DLRMTrainer

    rows = [1000, 20, 5000, 300]
    cfg = DLRMConfig(embedding_dim=128, table_rows=rows, table_dtype="bf16",
                     interaction=interaction)
    tr = DLRMTrainer(cfg, 256, DEV)
    st = tr.emb.tw_store
    assert st.weight.dtype == torch.bfloat16 and st.state1.dtype == torch.float32
    w0 = st.weight.clone()
    data = SyntheticCriteo(rows, 256, device=DEV, seed=0)
    seen = torch.zeros(st.weight.shape[0], dtype=torch.bool, device=DEV)
    ro = torch.tensor(st.row_offset_host, device=DEV)
    for i in range(10):
        if i == 5:                                     # five eager steps, five replayed
            tr.capture_graph(warmup=0)
            assert tr.graph is not None
        batch = data.next()
        ids = batch[1].view(len(rows), 256)
        seen[(ids + ro[:, None]).view(-1)] = True
        tr.load_batch(*batch)
        tr.step()
    torch.cuda.synchronize()
    loss = tr.pop_loss() / (10 * 256)
    assert loss == loss and 0 < loss < 10, loss
    sd = tr.state_dict()["emb"]["tw"]
    w1 = sd["weight"]
    assert w1.dtype == torch.bfloat16 and int(sd["sr_step"]) == 10
    assert not torch.equal(w1[seen], w0[seen])
    assert torch.equal(w1[~seen].view(torch.int16), w0[~seen].view(torch.int16))
    assert bool(torch.isfinite(w1.float()).all())

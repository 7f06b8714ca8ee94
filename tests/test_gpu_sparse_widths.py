"""The sparse HIP kernels at every dispatched row width and key size (run on
MI355X): embedding bag forward (embedding.hip), fused embedding backward +
optimizer, the row-wise "rows" exchange (rowwise.hip) and the pairwise
interaction (interaction.hip), each against a float64 oracle
(tests/sparse_oracle.py) or the project's CPU reference, at the smallest
shapes that reach the width-specific paths. The bounds are derived in
sparse_oracle.py; test_sparse_oracle.py holds the CPU references to the same
ones."""
import functools

import pytest
import torch

from tdfo_amd import ops
from tdfo_amd.ops import reference as ref
from tests import sparse_oracle as so
from tests.test_gpu_rowwise import _recv_from, make_meta, rand_ids

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


# ------------------------------------------------------- A. embedding forward
@functools.lru_cache(maxsize=None)
def _fwd_oracle(D, use_psw, mean):
    c = so.fwd_multihot_case(D)
    return so.embedding_bag_fwd(c["W"], c["ro"], c["idx"], c["offs"], c["out_off"], c["T"],
                                c["B"], c["out_stride"], psw=c["psw"] if use_psw else None,
                                mean=mean)


@pytest.mark.parametrize("mode", so.FWD_MODES, ids=lambda m: f"{m[0]}-psw{int(m[1])}-mean{int(m[2])}")
@pytest.mark.parametrize("D", so.WIDTHS)
def test_embedding_fwd_multihot(D, mode):
    """emb_fwd_kernel at every width (D = 512: two column passes per lane):
    bags of 0..130 ids (three staging chunks, the next chunk's prefetch, lane
    groups of one wave with different trip counts), per-sample weights, mean,
    permuted output slots; the 8 pad columns of every row keep their fill."""
    dt, use_psw, mean = mode
    out = so.run_fwd(so.fwd_multihot_case(D), DEV, DT[dt], use_psw, mean)
    so.check_fwd(out, _fwd_oracle(D, use_psw, mean))


@pytest.mark.parametrize("large", [False, True], ids=["small", "grid-cap"])
@pytest.mark.parametrize("use_psw", [False, True])
@pytest.mark.parametrize("D", so.WIDTHS)
def test_embedding_fwd_onehot(D, use_psw, large):
    """emb_fwd_onehot_kernel == emb_fwd_kernel bit for bit, and both equal
    W[row] * psw in float64 within the forward bound. ``grid-cap``: 37 bags more
    than 8192 blocks x 4 waves x bags-per-wave(D), the first count at which a
    lane group holds a second bag in flight (``has1``) and at which the
    general kernel's waves take more than one work item."""
    c = so.fwd_onehot_case(D, large)
    dt = torch.bfloat16 if D <= 64 else torch.float32
    a = so.run_fwd(c, DEV, dt, use_psw, False, onehot=True)
    b = so.run_fwd(c, DEV, dt, use_psw, False, onehot=False)
    assert torch.equal(a, b)
    oracle = so.fwd_onehot_oracle(c, use_psw, DEV)
    so.check_fwd(a, oracle)
    so.check_fwd(b, oracle)


# ------------------------------------------- B. embedding backward + optimizer
def _clone(states):
    return [None if s is None else s.clone() for s in states]


def _check(c, opt, got, states, hyper=None):
    return so.check_bwd(got, so.bwd_before(c, states), c["urows"],
                        so.bwd_exact(c, opt, states, hyper), c["D"])


@pytest.mark.parametrize("path", range(len(so.BWD_PATHS)), ids=[p[0] for p in so.BWD_PATHS])
@pytest.mark.parametrize("opt", so.ALL_OPTS)
@pytest.mark.parametrize("D", so.WIDTHS)
def test_embedding_bwd_all_widths(D, opt, path):
    """Every BwdCfg<D> (elements per lane 1..8, chunk sizes 16 / 32 / 16 / 8)
    under every optimizer: the radix-sort path on ragged bags (fp32 sums, and
    bf16 gradients with per-sample weights and mean), the one-hot per-table
    sort with the in-kernel combine (B = 256) and with the separate combine
    (B = 250, also bit-equal to the radix-sort path). Rows no id touches keep
    their bits, states included."""
    c = so.bwd_case(D, path)
    onehot = so.BWD_PATHS[path][2]
    st = so.bwd_states(c, opt)
    got = so.run_bwd(c, opt, DEV, _clone(st), segsort=1 if onehot else 0)
    _check(c, opt, got, st)
    if path == 3:
        assert so.same_bits(got, so.run_bwd(c, opt, DEV, _clone(st), segsort=0))


@pytest.mark.parametrize("opt", [ops.EMB_ROWWISE_ADAGRAD, ops.EMB_ADAM, ops.EMB_DENSE_GRAD])
@pytest.mark.parametrize("D", [16, 256, 512])
def test_embedding_bwd_long_runs_widths(D, opt):
    """~5460 ids on each row of a 3-row table: more than COMBINE_LONG chunks at
    the narrowest and the two widest rows, so emb_combine_long_kernel finishes
    them. Equal to the oracle and bitwise reproducible."""
    c = so.bwd_long_case(D)
    st = so.bwd_states(c, opt)
    a = so.run_bwd(c, opt, DEV, _clone(st))
    b = so.run_bwd(c, opt, DEV, _clone(st))
    assert so.same_bits(a, b)
    _check(c, opt, a, st)


KEY64_SHAPES = ("general-f32-sum", "general-bf16-psw-mean", "onehot256", "onehot2304", "multirun")


@pytest.mark.parametrize("shape", KEY64_SHAPES)
@pytest.mark.parametrize("opt", [ops.EMB_SGD, ops.EMB_ADAM])
@pytest.mark.parametrize("D", [16, 128, 512])
def test_embedding_bwd_key_bits_40(D, opt, shape):
    """key_bits = 40 runs the uint64_t instantiations (keys kernel, per-table
    sort, run merge, two-half readlane, update and combine): bit-equal to the
    default 32-bit keys and equal to the oracle. Not covered: a key above
    2^32 needs a table of more than 2^32 rows, so these are the 64-bit code
    paths with a zero high word, not the high word itself."""
    seg = 0
    if shape.startswith("general"):
        c = so.bwd_case(D, KEY64_SHAPES.index(shape))
    elif shape == "multirun":
        c, seg = so.bwd_multirun_case(D), 2
    else:
        c, seg = so.bwd_onehot_case(D, int(shape[6:])), 1
    st = so.bwd_states(c, opt)
    wide = so.run_bwd(c, opt, DEV, _clone(st), segsort=seg, key_bits=40)
    narrow = so.run_bwd(c, opt, DEV, _clone(st), segsort=seg)
    assert so.same_bits(wide, narrow)
    _check(c, opt, wide, st)


@pytest.mark.parametrize("fixed", [False, True], ids=["ragged", "bag_len"])
@pytest.mark.parametrize("opt", [ops.EMB_ROWWISE_ADAGRAD, ops.EMB_ADAM])
@pytest.mark.parametrize("D", [16, 512])
def test_embedding_bwd_prepare_apply_widths(D, opt, fixed):
    """prepare + apply == the fused call bit for bit on the radix-sort path
    with per-sample weights and mean, at the narrowest and widest rows; with
    fixed-length bags also when the keys pass divides by ``bag_len``."""
    c = so.bwd_fixed_len_case(D) if fixed else so.bwd_case(D, 1)
    st = so.bwd_states(c, opt)
    fused = so.run_bwd(c, opt, DEV, _clone(st))
    _check(c, opt, fused, st)
    i = so.bwd_inputs(c, DEV)
    hyper = c["hyper"].to(DEV)
    for bag_len in ([None, c["bag_len"].to(DEV)] if fixed else [None]):
        t = so.bwd_tensors(c, _clone(st), DEV)
        ws = torch.empty(ops.embedding_bwd_workspace(c["idx"].numel(), D), dtype=torch.uint8,
                         device=DEV)
        ops.embedding_bwd_prepare(t["W"], i["ro"], i["idx"], i["offs"], i["goff"], c["T"], c["B"],
                                  c["stride"], ws, mean=c["mean"], psw=i["psw"], bag_len=bag_len)
        ops.embedding_bwd_apply(t["W"], i["ro"], i["idx"], i["offs"], i["goff"], c["T"], c["B"],
                                i["grad"], c["stride"], opt, hyper, ws, state1=t["s1"],
                                state2=t["s2"], eps=so.EPS, beta1=so.BETA1, beta2=so.BETA2,
                                weight_decay=so.WEIGHT_DECAY, mean=c["mean"], psw=i["psw"])
        assert so.same_bits(fused, t)


def test_embedding_bwd_loss_scale_hyper():
    """hyper = [lr, step, unscale, skip] at D = 256: unscale 0.5 is the step of
    halved gradients; skip > 0 leaves W and both Adam moments bit for bit."""
    c = so.bwd_case(256, 1)
    opt = ops.EMB_ADAM
    st = so.bwd_states(c, opt)
    lr, step = so.HYPER
    for skip in (0.0, 1.0):
        hyper = torch.tensor([lr, step, 0.5, skip])
        _check(c, opt, so.run_bwd(c, opt, DEV, _clone(st), hyper=hyper), st, hyper)


# ------------------------------------------------ C. row-wise "rows" exchange
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("D", [16, 32, 64, 128, 256])
def test_rw_rows_exchange(D, W):
    """One process plays every rank of the one-hot rows exchange: bucketize,
    owner-side row gather, the all-to-all as a host permutation, requester
    scatter into the pooled region + slot map, gradient gather, and the owner
    backward on per-slot gradients -- every stage against its reference.
    Rows and maps are exact; slots past a segment's count and the region's pad
    columns keep their fill."""
    rows, L, B, seed = [1000, 37, 5000], [1, 1, 1], 96, 17
    nrw = len(rows)
    meta, n, total = make_meta(rows, L, B, W)
    cap, ld = n, nrw * D + 8
    meta_d = meta.to(DEV)
    sent = so.SENTINEL
    # 1. bucketize, per requester
    ids, send = [], []
    for r in range(W):
        ids.append(rand_ids(rows, L, B, torch.Generator().manual_seed(seed + r), "cpu"))
        s = torch.full((W * (cap + 1),), -7, dtype=torch.int64, device=DEV)
        ws = torch.empty(ops.rw_bucketize_workspace(n, W), dtype=torch.uint8, device=DEV)
        ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.rw_bucketize(ids[r].to(DEV), meta_d, nrw, W, B, cap, n, s, ws, ovf)
        exp = torch.full((W * (cap + 1),), -7, dtype=torch.int64)
        ref.rw_bucketize(ids[r], meta, nrw, W, B, cap, n, exp, torch.zeros(1, dtype=torch.int32))
        got, exp = s.cpu().view(W, cap + 1), exp.view(W, cap + 1)
        assert int(ovf) == 0 and torch.equal(got[:, cap], exp[:, cap])
        for o in range(W):
            k = int(exp[o, cap])
            assert torch.equal(got[o, :k], exp[o, :k]), (r, o)
        send.append(s)
    # 2. every owner gathers the rows of what it received
    g = torch.Generator().manual_seed(seed + 100 + D)
    Wt, recv, rows_out = [], [], []
    for o in range(W):
        rv = _recv_from(rows, L, B, W, owner=o, seed=seed, dev=DEV)[0]
        for r in range(W):      # what requester r bucketized for owner o, as received
            k = int(rv.view(W, cap + 1)[r, cap])
            assert torch.equal(rv.view(W, cap + 1)[r, :k], send[r].view(W, cap + 1)[o, :k])
        Wt.append(torch.randn(total + 1, D, generator=g).to(DEV))
        out = torch.full((W * (cap + 1) * D,), sent, dtype=torch.bfloat16, device=DEV)
        ops.rw_rows_gather(Wt[o], rv, W, cap, out)
        exp = torch.full((W * (cap + 1) * D,), sent, dtype=torch.bfloat16)
        ref.rw_rows_gather(Wt[o].cpu(), rv.cpu(), W, cap, exp)
        assert torch.equal(out.cpu(), exp), o
        recv.append(rv)
        rows_out.append(out.view(W, cap + 1, D))
    lrow = ref.rw_unpack_meta(meta, nrw)[3]
    gsend = []
    for r in range(W):
        # 3. the all-to-all: requester r receives segment r of every owner
        rows_in = torch.stack([rows_out[o][r] for o in range(W)]).contiguous().view(-1)
        # 4. scatter into the pooled region + the slot map
        region = torch.full((B * ld,), sent, dtype=torch.bfloat16, device=DEV)
        smap = torch.full((W * (cap + 1),), -7, dtype=torch.int32, device=DEV)
        ops.rw_rows_scatter(send[r], W, cap, B, D, rows_in, region, ld, smap, nrw)
        eregion = torch.full((B * ld,), sent, dtype=torch.bfloat16)
        emap = torch.full((W * (cap + 1),), -7, dtype=torch.int32)
        ref.rw_rows_scatter(send[r].cpu(), W, cap, B, D, rows_in.cpu(), eregion, ld, emap, nrw)
        assert torch.equal(region.cpu(), eregion) and torch.equal(smap.cpu(), emap), r
        reg = region.cpu().view(B, ld)
        assert bool((reg[:, nrw * D:] == sent).all())
        # the whole lookup end to end: bag (j, b) holds bf16 W_owner[local row of its id]
        for j in range(nrw):
            gid = ids[r][j * B:(j + 1) * B]
            want = torch.stack([Wt[int(i) % W][int(lrow[j]) + int(i) // W] for i in gid])
            assert torch.equal(reg[:, j * D:(j + 1) * D], want.to(torch.bfloat16).cpu()), (r, j)
        # 5. the backward's gradient rows, slot by slot
        dregion = torch.randn(B * ld, generator=g).to(torch.bfloat16).to(DEV)
        gs = torch.full((W * (cap + 1) * D,), sent, dtype=torch.bfloat16, device=DEV)
        ops.rw_grads_gather(smap, W, cap, D, dregion, gs)
        egs = torch.full((W * (cap + 1) * D,), sent, dtype=torch.bfloat16)
        ref.rw_grads_gather(emap, W, cap, D, dregion.cpu(), egs)
        assert torch.equal(gs.cpu(), egs), r
        gsend.append(gs.view(W, cap + 1, D))
    # owner 0's backward on the per-slot gradients it receives
    grecv = torch.stack([gsend[r][0] for r in range(W)]).contiguous().view(-1)
    hyper = torch.tensor([0.05, 1.0], device=DEV)
    kb = ops.key_bits_for(total + 1)
    for opt in (ops.EMB_ROWWISE_ADAGRAD, ops.EMB_SGD):
        s1 = torch.rand(total + 1, generator=g).to(DEV) if opt == ops.EMB_ROWWISE_ADAGRAD else None
        Wg = Wt[0].clone()
        sg1 = s1.clone() if s1 is not None else None
        ws = torch.empty(ops.embedding_bwd_workspace(W * cap, D), dtype=torch.uint8, device=DEV)
        ops.embedding_bwd_prepare_rw(Wg, recv[0], meta_d, nrw, W, B, cap, False, kb, D, total, ws,
                                     rows=True)
        ops.embedding_bwd_apply_rw(Wg, recv[0], meta_d, nrw, W, B, cap, False, kb, grecv, D, opt,
                                   hyper, ws, state1=sg1, rows=True)
        We = Wt[0].clone().cpu()
        se1 = s1.clone().cpu() if s1 is not None else None
        ref.rw_embedding_bwd(We, recv[0].cpu(), meta, nrw, W, B, cap, False, grecv.cpu(), D, opt,
                             se1, None, hyper.cpu(), 1e-8, 0.9, 0.999, 0.0, rows=True)
        # every real row matches; the scratch row (last) is junk by design
        diff = (Wg[:total].cpu() - We[:total]).abs() > 1e-5 + 1e-4 * We[:total].abs()
        assert not bool(diff.any()), int(diff.sum())
        assert not torch.equal(We[:total], Wt[0][:total].cpu())
        if se1 is not None:
            assert torch.allclose(sg1[:total].cpu(), se1[:total], atol=1e-5, rtol=1e-4)


# ------------------------------------------------------------ D. interaction
@pytest.mark.parametrize("B", so.INTER_B)
@pytest.mark.parametrize("F", so.INTER_F)
@pytest.mark.parametrize("D", so.INTER_D)
def test_interaction_widths(D, F, B):
    """inter_fwd_kernel / inter_bwd_kernel at every width (D = 256: eight
    column tiles in two batches, the dX image written over X columns, more
    than 64 KiB of LDS) and at both ends of the feature count, bf16 single
    rounding per element. ``dense`` is a column slice of a wider buffer with
    negatives, +0.0 and -0.0 (the ReLU mask is !(x > 0)); the gradient slots
    are permuted and further apart than the forward's; pads, gaps and the
    columns beside d_dense keep their fill (the output pad is zeroed)."""
    c = so.inter_case(D, F, B)
    so.check_inter_fwd(so.run_inter_fwd(c, DEV), c)
    for relu_mask in (True, False):
        dd, de = so.run_inter_bwd(c, DEV, relu_mask)
        so.check_inter_bwd(dd, de, c, relu_mask)


@pytest.mark.parametrize("D", so.INTER_D)
def test_interaction_ones_col(D):
    """``ones_col`` inside the pad: that column is exactly 1.0, the rest of the
    pad exactly 0."""
    c = so.inter_case(D, 17, 37)
    oc = c["ones_col"]
    assert D + c["P"] <= oc < c["ldo"]
    out = so.run_inter_fwd(c, DEV, oc)
    so.check_inter_fwd(out, c, oc)
    assert bool((out[:, oc] == 1.0).all())

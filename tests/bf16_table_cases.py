"""Shared inputs, bounds and runners of the bf16-table tests
(test_bf16_tables.py on the CPU reference, test_gpu_bf16_tables.py on the HIP
kernels). The cases are the cached ones of tests/sparse_oracle.py with the
table rounded to bf16; the float64 oracle runs on that rounded table.

Bounds of one update of a bf16 row (none measured on the code under test).
The update is computed in fp32 on the widened row, so the value y that gets
rounded is within the project's tol = 1e-4 max(1, max|exact|) of the float64
result, and only the store rounds. With ulp the bf16 spacing at |exact| + tol
(>= the spacing at y):
  nearest even   |got - exact| <= ulp / 2 + tol
  stochastic     |got - exact| <  ulp + tol   (one of y's two bf16 neighbours)
The row-wise Adagrad state stays fp32: the project's 1e-3 scaling.
"""
import hashlib
import os
import subprocess
import sys

import torch

from tdfo_amd.ops import reference as ref
from tests import sparse_oracle as so

BF16_DIMS = (64, 128, 256)
BF16_OPTS = (ref.EMB_SGD, ref.EMB_ROWWISE_ADAGRAD)
SR_SEED = 0x5EED1234
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rounded(c):
    """The case with its table rounded to nearest bf16 (a bf16 tensor)."""
    d = dict(c)
    d["W"] = c["W"].to(torch.bfloat16)
    return d


def bf16_ulp(v):
    """bf16 spacing at |v| (float64 tensor): 2^(floor(log2 |v|) - 7), the
    subnormal spacing 2^-133 below the smallest normal."""
    _, e = torch.frexp(v.abs().double())             # |v| = m 2^e, m in [0.5, 1)
    return torch.pow(2.0, (e - 8).clamp_min(-133).double())


def bwd_exact(c, opt, states, hyper=None):
    """float64 oracle of one update of the rounded table's touched rows."""
    s1, s2, dg = states
    return so.embedding_opt(c["W"].double(), c["urows"], c["g"], opt,
                            c["hyper"] if hyper is None else hyper, s1, s2, dg,
                            weight_decay=so.WEIGHT_DECAY)


def check_bwd(got, c, states, exact, sr):
    """Touched rows of W within the rounding bound of ``exact`` (every element),
    the row-wise state within 1e-3, every other row bitwise unchanged; exact
    None (a skipped step): nothing changes. Returns the worst err / bound."""
    W0, s1 = c["W"], states[0]
    Wg = got["W"].detach().cpu()
    assert Wg.dtype == torch.bfloat16
    rows = c["urows"]
    if exact is None:
        assert torch.equal(Wg.view(torch.int16), W0.view(torch.int16)), "W changed on a skipped step"
        if s1 is not None:
            assert torch.equal(got["s1"].cpu(), s1), "state changed on a skipped step"
        return 0.0
    untouched = torch.ones(W0.shape[0], dtype=torch.bool)
    untouched[rows] = False
    assert torch.equal(Wg[untouched].view(torch.int16), W0[untouched].view(torch.int16)), \
        "an untouched row changed"
    ex = exact["W"]
    tol = 1e-4 * max(1.0, float(ex.abs().max()))
    ulp = bf16_ulp(ex.abs() + tol)
    err = (Wg[rows].double() - ex).abs()
    bound = ulp + tol if sr else ulp / 2 + tol
    bad = ~(err < bound) if sr else ~(err <= bound)
    assert not bool(bad.any()), (int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))
    if exact["s1"] is not None:
        g1 = got["s1"].detach().cpu()
        assert g1.dtype == torch.float32
        assert torch.equal(g1[untouched], s1[untouched]), "state of an untouched row changed"
        e1 = float((g1[rows].double() - exact["s1"]).abs().max())
        assert e1 < 1e-3 * max(1.0, float(exact["s1"].abs().max())), e1
    return float((err / bound).max())


def sr_kw(dev, sr, counter=0, seed=SR_SEED):
    """The rounding arguments of ops.embedding_bwd (a fresh counter tensor)."""
    return dict(sr_seed=seed, stochastic_rounding=sr,
                sr_counter=torch.tensor(counter, dtype=torch.int64, device=dev))


def run_split(c, opt, dev, states, bag_len=None, segsort=0, key_bits=None, **kw):
    """prepare + apply of a case (GPU) -> the updated tensors."""
    from tdfo_amd import ops

    t = so.bwd_tensors(c, states, dev)
    i = so.bwd_inputs(c, dev)
    ws = torch.empty(ops.embedding_bwd_workspace(c["idx"].numel(), c["D"]), dtype=torch.uint8,
                     device=dev)
    seg = ops.effective_segsort(segsort)
    ops.embedding_bwd_prepare(t["W"], i["ro"], i["idx"], i["offs"], i["goff"], c["T"], c["B"],
                              c["stride"], ws, mean=c["mean"], psw=i["psw"], bag_len=bag_len,
                              segsort=seg, key_bits=key_bits, sr_counter=kw.get("sr_counter"))
    ops.embedding_bwd_apply(t["W"], i["ro"], i["idx"], i["offs"], i["goff"], c["T"], c["B"],
                            i["grad"], c["stride"], opt, c["hyper"].to(dev), ws, state1=t["s1"],
                            state2=t["s2"], eps=so.EPS, beta1=so.BETA1, beta2=so.BETA2,
                            weight_decay=so.WEIGHT_DECAY, mean=c["mean"], psw=i["psw"],
                            segsort=seg, key_bits=key_bits, **kw)
    return t


# ------------------------------------------------------ rounding primitive
def round_inputs(D=128):
    """[n, D] fp32: 2^16 random values over many binades plus the edge cases
    (+-0, subnormals, +-inf, NaN, the largest finite bf16, bf16 values)."""
    g = torch.Generator().manual_seed(20240)
    x = torch.randn(1 << 16, generator=g) * torch.pow(
        2.0, torch.randint(-30, 30, (1 << 16,), generator=g).float())
    bf = torch.randn(256, generator=g).to(torch.bfloat16).float()        # representable
    edge = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, float("inf"), float("-inf"),
                         float("nan"), 3.3895313892515355e38, -3.3895313892515355e38, 1.0,
                         1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 1.0 + 2.0 ** -8])
    x = torch.cat([x, bf, edge])
    pad = (-x.numel()) % D
    x = torch.cat([x, torch.zeros(pad)])
    return x.view(-1, D).contiguous()


def check_rounding(x, y, seed, counter, row0):
    """``y`` (bf16) is the contract's stochastic rounding of ``x``: the random
    bits recomputed here from ``_hash3``."""
    n, D = x.shape
    bits = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    low = bits & 0xFFFF
    yb = y.cpu().view(torch.int16).to(torch.int64) & 0xFFFF
    nan = torch.isnan(x)
    inf = torch.isinf(x)
    fin = ~(nan | inf)
    assert bool(torch.isnan(y.float()[nan]).all()) and not bool(torch.isnan(y.float()[~nan]).any())
    assert torch.equal(y.float()[inf], x[inf])
    rep = fin & (low == 0)
    assert torch.equal(yb[rep], (bits >> 16)[rep]), "a bf16 value moved"
    down = bits >> 16                                 # neighbour towards zero
    up = down + 1                                     # neighbour away from zero (may be inf)
    assert bool(((yb == down) | (yb == up))[fin].all()), "not a bf16 neighbour"
    key = (seed ^ ((counter * 0x632BE5AB) & 0xFFFFFFFF)) & 0xFFFFFFFF
    row = torch.arange(n, dtype=torch.int64) + row0
    rowh = ((row & 0xFFFFFFFF) ^ (((row >> 32) & 0xFFFFFFFF) * 0x9E3779B1)) & 0xFFFFFFFF
    r = ref._hash3(torch.full((1, 1), key, dtype=torch.int64), rowh[:, None],
                   torch.arange(D, dtype=torch.int64)[None, :]) & 0xFFFF
    want_up = r >= 65536 - low                        # (low == 0: never)
    assert torch.equal((yb == up)[fin], want_up[fin]), "rounding direction"


# ------------------------------------------------- progress and statistics
def progress_store(dev, sr, seed=3):
    from tdfo_amd.sparse.tables import EmbOptimConfig, TableBatchedEmbedding

    st = TableBatchedEmbedding([512], 128, dev, EmbOptimConfig("sgd", lr=1.0,
                                                               stochastic_rounding=sr),
                               seed=seed, dtype=torch.bfloat16)
    st.weight.fill_(1.0)
    return st


def run_progress(dev, sr, seed=3, updates=64):
    """512 rows x 128 of 1.0, one id per bag (a permutation of the rows), SGD
    with lr = 1 and gradient -2^-10 everywhere: every update adds 2^-10 = 1/8
    of the bf16 spacing at 1, every intermediate exact in fp32."""
    st = progress_store(dev, sr, seed)
    B, D = 512, 128
    idx = torch.randperm(B, generator=torch.Generator().manual_seed(11)).to(dev)
    offs = torch.arange(B + 1, dtype=torch.int64, device=dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    grad = torch.full((B, D), -(2.0 ** -10), dtype=torch.float32, device=dev)
    hyper = torch.tensor([1.0, 1.0], device=dev)
    for _ in range(updates):
        st.backward_update(idx, offs, st.row_offset, 1, B, grad, zero, D, hyper, segsort=1)
    return st


def check_progress(st, updates=64):
    w = st.weight.detach().cpu()
    assert w.dtype == torch.bfloat16
    k = (w.double() - 1.0) * 128.0
    assert torch.equal(k, k.round()) and float(k.min()) >= 0 and float(k.max()) <= updates
    assert int(st.sr_step) == updates
    n = k.numel()
    assert n == 65536
    mean, var = float(k.mean()), float(k.var())
    assert abs(mean - 8.0) <= 6 * (7 / 65536) ** 0.5, mean
    assert abs(var - 7.0) <= 6 * 7 * (2 / 65536) ** 0.5, var
    rdev = float((k.mean(1) - 8.0).abs().max())
    cdev = float((k.mean(0) - 8.0).abs().max())
    assert rdev <= 6 * (7 / 128) ** 0.5, rdev
    assert cdev <= 6 * (7 / 512) ** 0.5, cdev
    return mean, var, rdev, cdev


# ------------------------------- child process: in-kernel combine on / off
def ikc_digest():
    """sha256 of the tables after an SR update of the one-hot B = 256 case at
    D = 128 under both optimizers (run with TDFO_EMB_INKERNEL_COMBINE set: the
    library reads it when it loads)."""
    h = hashlib.sha256()
    c = rounded(so.bwd_onehot_case(128, 256))
    for opt in BF16_OPTS:
        st = so.bwd_states(c, opt)
        got = so.run_bwd(c, opt, "cuda", [None if s is None else s.clone() for s in st],
                         segsort=1, **sr_kw("cuda", True, counter=4))
        h.update(got["W"].cpu().view(torch.int16).numpy().tobytes())
        if got["s1"] is not None:
            h.update(got["s1"].cpu().numpy().tobytes())
    return h.hexdigest()


def ikc_child(value):
    env = dict(os.environ, TDFO_EMB_INKERNEL_COMBINE=str(value))
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "tests.bf16_table_cases"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()[-1]


if __name__ == "__main__":
    print(ikc_digest())

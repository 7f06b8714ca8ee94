"""CPU self-check of tests/dense_oracle.py. Every case of the GPU GEMM tests
runs through ``ops.gemm`` on CPU tensors -- the fp32 torch reference -- and
must pass ``check_gemm`` in both data modes with no element exempted: the
float64 oracle agrees with the project's reference, and the bounds need no
kernel's help. The teeth tests then show that ``check_gemm`` fails on a
correct result with one defect planted in it."""
import pytest
import torch

from tdfo_amd import ops
from tests import dense_oracle as do

MODES = ("exact", "float")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", do.ALL_CASES, ids=do.case_id)
def test_reference_meets_oracle(case, mode):
    got = do.run_gemm(case, "cpu", mode=mode)
    assert do.check_gemm(got, do.gemm_oracle(case, mode), mode, slab0=True) <= 1.0


@pytest.mark.parametrize("pair,mode", [(n, m) for n in do.PAIRS for m in do.PAIR_MODES[n]])
def test_reference_pairs_meet_oracle(pair, mode):
    cases = do.PAIRS[pair]
    for c, got in zip(cases, do.run_pair(cases, "cpu", mode=mode)):
        assert do.check_gemm(got, do.gemm_oracle(c, mode), mode, slab0=True) <= 1.0


@pytest.mark.parametrize("mode", MODES)
def test_reference_wrappers_meet_oracle(mode):
    assert do.check_wrappers("cpu", mode) <= 1.0


def test_case_lists_skip_nothing():
    """Every layout gets only the shapes its contract allows, and the lists
    hold what the kernels' paths need."""
    for c in do.ALL_CASES + do.PAIRS["long"]:
        assert not (c.a_col and c.M % 8) and not (c.b_col and c.N % 8)
        assert c.S <= c.ktiles and c.ld32 >= c.N and c.ld32 % 4 == 0
    assert any(c.empty_slabs() for c in do.SPLIT_CASES)
    assert {c.K for c in do.K_CASES} == set(do.K_SWEEP)
    assert any(c.N % 8 and c.mask for c in do.EPI_CASES)
    # a row-layout A on the 128-row two-stage body (policy 1) needs 256 tiles
    assert any(not c.a_col and -(-c.M // 128) * -(-c.N // 128) >= 256 for c in do.SHAPE_CASES)
    for n, (w, d) in do.PAIRS.items():
        assert w.a_col and w.b_col and d.b_col and (w.csum == (n == "csum"))
    d = do.case_data(do.PITCH_CASES[1], "exact")                 # odd pitch, 2-B aligned base
    for slot in (d["out"]["c"], d["in"]["mask"][0]):
        assert slot.off % 2 == 1 and slot.stride[0] % 8 == 3
    a = do.case_data(do.K_CASES[0], "exact")["in"]["a"][0]
    assert a.off % 8 == 0 and a.stride[0] % 8 == 0 and a.stride[0] > a.size[1]


def test_split_with_epilogue_is_refused():
    M, N, K = 8, 8, 128
    a = torch.ones(M, K, dtype=torch.bfloat16)
    b = torch.ones(N, K, dtype=torch.bfloat16)
    o = torch.zeros(2 * M * N)
    for kw in (dict(bias=torch.ones(N)), dict(relu=True),
               dict(mask=torch.ones(M, N, dtype=torch.bfloat16))):
        with pytest.raises(RuntimeError, match="splits > 1 takes no bias, relu or mask"):
            ops.gemm(a, False, b, False, out32=o, splits=2, **kw)
    assert bool((o == 0).all())
    ops.gemm(a, False, b, False, out32=o, splits=2)
    assert bool((o.view(2, M, N).sum(0) == K).all())


# ------------------------------------------------------------------- teeth
def _values(c, mode, drop=None, twice=False, bias_shift=0, mask_first=False, relu_last=False,
            ge=False, c2_from_c=False):
    """What a kernel with the given defect would compute, float64; slab 0
    holds everything."""
    d = do.case_data(c, mode)
    A, B = d["A"], d["B"]
    x = A @ B
    if drop is not None:
        m, n, k = drop
        x[m, n] -= A[m, k] * B[k, n]
    if twice:
        x = x + A[:, 64:128] @ B[64:128]
    bias = d["bias"].roll(bias_shift) if c.bias else torch.zeros(c.N, dtype=torch.float64)
    live = torch.ones(c.M, c.N, dtype=torch.bool)
    if c.mask:
        live = (d["mask"] >= 0) if ge else (d["mask"] > 0)
    zero = torch.zeros_like(x)
    relu = (lambda t: t.clamp_min(0)) if c.relu else (lambda t: t)
    if mask_first:                    # mask, then bias, then ReLU
        v = relu(torch.where(live, x, zero) + bias)
    elif relu_last:                   # bias, mask, then ReLU
        v = relu(torch.where(live, x + bias, zero))
    else:
        v = torch.where(live, relu(x + bias), zero)
    mul = d["mul"] if c.mul else 1.0
    add = d["add"] if c.add else 0.0
    c32 = torch.zeros(c.S, c.M, c.N, dtype=torch.float64)
    c32[0] = v
    csum = torch.zeros(c.S, c.M, dtype=torch.float64)
    csum[0] = A.sum(1)
    return {"c": v, "c32": c32, "csum": csum,
            "c2": (do.rne_bf16(v) if c2_from_c else v) * mul + add}


def _bits(got):
    return {k: p.view(torch.int16 if p.dtype == torch.bfloat16 else torch.int32).clone()
            for k, p in got.items()}


def _must_fail(c, mode, good, bad):
    """``bad`` differs from ``good`` in at least one output bit, ``good``
    passes and ``bad`` does not."""
    o = do.gemm_oracle(c, mode)
    assert do.check_gemm(good, o, mode, slab0=True) <= 1.0
    gb, bb = _bits(good), _bits(bad)
    assert any(not torch.equal(gb[k], bb[k]) for k in gb), "the corruption changed nothing"
    with pytest.raises(AssertionError):
        do.check_gemm(bad, o, mode, slab0=True)


def _heavy_term(c, mode):
    """(m, n, k) of the largest |a b| among elements no epilogue stage hides."""
    d, o = do.case_data(c, mode), do.gemm_oracle(c, mode)
    keep = o["live"] & (o["v"] > 0)
    terms = d["A"][:, None, :].abs() * d["B"].t()[None, :, :].abs()       # [M, N, K]
    terms = terms * keep[:, :, None]
    i = int(terms.argmax())
    return i // (c.N * c.K), i // c.K % c.N, i % c.K


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("defect", ["k_term_dropped", "k_tile_twice", "bias_shifted", "mask_first",
                                    "mask_ge", "c2_from_rounded_c"])
def test_teeth_wrong_arithmetic(defect, mode):
    c = do.TEETH_EPI
    kw = {"k_term_dropped": dict(drop=_heavy_term(c, mode)), "k_tile_twice": dict(twice=True),
          "bias_shifted": dict(bias_shift=1), "mask_first": dict(mask_first=True),
          "mask_ge": dict(ge=True), "c2_from_rounded_c": dict(c2_from_c=True)}[defect]
    _must_fail(c, mode, do.compose(c, mode, _values(c, mode)),
               do.compose(c, mode, _values(c, mode, **kw)))


@pytest.mark.parametrize("mode", MODES)
def test_relu_after_mask_is_the_same_function(mode):
    """ReLU before or after a 0/1 mask gives the same values (they differ only
    in the sign of a zero, which ``==`` ignores on purpose), so no check can
    or should tell the two orders apart; what does differ, and is caught
    above, is the mask moving in front of the bias."""
    c = do.TEETH_EPI
    a, b = _values(c, mode), _values(c, mode, relu_last=True)
    assert all(bool((a[k] == b[k]).all()) for k in a)
    assert not bool((a["c"] == _values(c, mode, mask_first=True)["c"]).all())


@pytest.mark.parametrize("mode", MODES)
def test_teeth_bf16_truncation(mode):
    c = do.TEETH_EPI
    good = do.compose(c, mode, _values(c, mode))
    bad = {k: p.clone() for k, p in good.items()}
    v = _values(c, mode)["c"].float()
    trunc = (v.view(torch.int32) & -65536).view(torch.float32)            # drop the low 16 bits
    do.case_data(c, mode)["out"]["c"].view(bad["c"]).copy_(trunc)
    _must_fail(c, mode, good, bad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["c", "c2", "c32"])
def test_teeth_write_into_the_ring(name, mode):
    c = do.TEETH_EPI
    good = do.compose(c, mode, _values(c, mode))
    slot = do.case_data(c, mode)["out"][name]
    for at in (slot.off - 1, slot.off + c.N if name != "c32" else slot.off + c.N + 1):
        bad = {k: p.clone() for k, p in good.items()}
        assert float(bad[name][at]) == do.SENTINEL
        bad[name][at] = 0.0
        _must_fail(c, mode, good, bad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("defect", ["k_term_dropped", "slab_unwritten", "slab_csum_unwritten",
                                    "csum_next_column"])
def test_teeth_split(defect, mode):
    c = do.TEETH_SPLIT
    good = do.compose(c, mode, _values(c, mode))
    if defect == "k_term_dropped":
        d = do.case_data(c, mode)
        terms = d["A"][:, None, :].abs() * d["B"].t()[None, :, :].abs()
        i = int(terms.argmax())
        bad = do.compose(c, mode, _values(c, mode, drop=(i // (c.N * c.K), i // c.K % c.N,
                                                         i % c.K)))
    else:
        bad = {k: p.clone() for k, p in good.items()}
        sl = do.case_data(c, mode)["out"]["c32"].view(bad["c32"]).view(c.S, c.M, c.ld32)
        if defect == "slab_unwritten":
            sl[1, :, :c.N] = float("nan")             # as the harness initialised it
        elif defect == "slab_csum_unwritten":
            sl[1, :, c.N] = float("nan")
        else:
            sl[:, :, c.N + 1] = sl[:, :, c.N]
            sl[:, :, c.N] = 0.0
    _must_fail(c, mode, good, bad)


def test_teeth_empty_slab_not_zeroed():
    c = do.SPLIT_CASES[4]                             # 5 K tiles in 4 splits
    assert c.S == 4 and c.empty_slabs() == [3]
    o = do.gemm_oracle(c, "exact")
    v = _values(c, "exact")
    good = do.compose(c, "exact", v)
    assert do.check_gemm(good, o, "exact") == 0.0
    v["c32"][3, 5, 5], v["c32"][0, 5, 5] = 1.0, v["c32"][0, 5, 5] - 1.0   # the sum still holds
    with pytest.raises(AssertionError, match="empty slab"):
        do.check_gemm(do.compose(c, "exact", v), o, "exact")

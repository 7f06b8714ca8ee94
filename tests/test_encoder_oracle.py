"""The float64 oracles of tests/encoder_oracle.py checked on the CPU: the
hand-written backwards against torch.autograd, the dropout masks against the
reference's bit for bit, the fp32 reference's own error on every case of the
GPU test (the yardstick of its bound), the ReLU-margin condition, the LDS
formula, and that the metric rejects planted errors."""
import math

import pytest
import torch

from tdfo_amd.ops import reference as ref
from tests import encoder_oracle as eo

F64 = torch.float64


def _rel(a, r):
    return float((a - r).abs().max() / (r.abs().max() + 1e-300))


# ------------------------------------------------ backwards vs autograd (fp64)
def _plain_ln(v, gamma, beta):
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    return (v - mu) / torch.sqrt(var + eo.EPS) * gamma + beta


def _plain_mha(qkv, valid, H, m, causal):
    B, T, E3 = qkv.shape
    E = E3 // 3
    q, k, v = qkv.view(B, T, 3, H, E // H).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1) / math.sqrt(E // H)).masked_fill(~valid.view(B, 1, 1, T), -1e9)
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), -math.inf)
    return ((torch.softmax(s, -1) * m) @ v).transpose(1, 2).reshape(B, T, E)


@pytest.mark.parametrize("rate", [None, 0.0, 0.5])
@pytest.mark.parametrize("M,n,family", [(5, 65, "randn"), (3, 2, "mean100"), (5, 129, "const"),
                                        (1, 1, "randn")])
def test_layernorm_and_prologue_bwd_match_autograd(M, n, family, rate):
    c = eo.ln_case(M, n, family, rate)
    x, pos, gamma, beta = (t.to(F64).requires_grad_(True) for t in (c.x, c.pos, c.gamma, c.beta))
    y = _plain_ln(x + pos, gamma, beta) * c.m
    gr = torch.autograd.grad(y, [x, gamma, beta, pos], c.g.to(F64))
    assert _rel(c.exact["y"], y.detach()) < 1e-12
    names = ["dx", "dgamma", "dbeta"] + (["dpos"] if rate is not None else [])
    for k, r in zip(names, gr):
        assert _rel(c.exact[k], r) < 1e-10, k


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", [(2, 33, 16, 4, 0.0, "full"), (2, 64, 16, 4, 0.25, "left"),
                                  (2, 2, 16, 2, 0.0, "lone"), (3, 63, 64, 4, 0.0, "lone")])
def test_mha_bwd_matches_autograd(case, causal):
    c = eo.attn_case(*case, causal)
    qkv = c.qkv.to(F64).requires_grad_(True)
    out = _plain_mha(qkv, c.valid, c.H, c.m, causal)
    (g,) = torch.autograd.grad(out, qkv, c.dout.to(F64))
    assert _rel(c.exact["out"], out.detach()) < 1e-12
    assert _rel(c.exact["dqkv"], g) < 1e-10
    if c.pattern == "full" and not causal:       # an all-PAD row is uniform over the keys
        assert _rel(c.exact["out"][0], eo._heads(c.qkv[..., 2 * c.E:].to(F64), c.H)[0].mean(1)
                    .view(1, c.E).expand(c.T, c.E)) < 1e-12


@pytest.mark.parametrize("case", [(16, 2, 20, 0.1, "left"), (16, 2, 63, 0.3, "full"),
                                  (32, 8, 25, 0.1, "lone"), (32, 1, 37, 0.0, "none"),
                                  (16, 2, 1, 0.1, "none")])
def test_encoder_block_bwd_matches_autograd(case):
    c = eo.enc_case(*case)
    x = c.x.to(F64).requires_grad_(True)
    ps = [p.to(F64).requires_grad_(True) for p in c.params]
    wqkv, bqkv, wo, bo, g1, be1, g2, be2, w1, b1, w2, b2 = ps
    m = c.masks
    qkv = _plain_ln(x, g1, be1) @ wqkv.t() + bqkv
    ctx = _plain_mha(qkv, c.valid, c.H, m.p, False)
    x1 = x + (ctx @ wo.t() + bo) * m.a
    f = torch.relu(_plain_ln(x1, g2, be2) @ w1.t() + b1)
    y = (x1 + ((f * m.f) @ w2.t() + b2) * m.g) * m.blk
    gr = torch.autograd.grad(y, [x] + ps, c.dy.to(F64))
    for k, t in (("y", y), ("qkv", qkv), ("ctx", ctx), ("x1", x1), ("f", f)):
        assert _rel(c.exact[k], t.detach()) < 1e-12, k
    for k, r in zip(["dx"] + ["d" + n for n in eo.PARAM_NAMES], gr):
        assert _rel(c.exact[k], r) < 1e-10, k


# ------------------------------------------------------- masks, bit for bit
@pytest.mark.parametrize("seed,step", [(0x5EED, 0), (123, 7), (0xFFFFFFFF, 1), (1, 1 << 33)])
@pytest.mark.parametrize("rate", [0.1, 0.25, 0.5])
def test_masks_equal_reference_bit_for_bit(seed, step, rate):
    B, H, T = 9, 8, 64                            # B * H = 72 > 64
    pairs = [(eo.attn_keep(B, H, T, rate, seed, step),
              ref.attn_keep_scale(B, H, T, rate, seed, step, "cpu"))]
    for site in (eo.SITE_A, eo.SITE_F, eo.SITE_G, eo.SITE_BLK):
        pairs.append((eo.site_keep(B, T, 64, rate, seed, step, site),
                      ref.enc_site_mul(B, T, 64, rate, seed, step, site, "cpu")))
    pairs.append((eo.prologue_keep(1030, 320, rate, seed, step),
                  ref.seq_prologue_mul(1030, 320, rate, seed, step, "cpu")))
    for keep, r in pairs:
        assert torch.equal(keep, r != 0)
        assert torch.equal(eo.mul(keep, rate).float(), r)
        assert abs(float(keep.double().mean()) - (1 - rate)) < 0.02
    assert bool(eo.attn_keep(2, 2, 8, 0.0, seed, step).all())


# ------------------------------------- the fp32 reference's own error (yardstick)
def _show(tag, e):
    print(tag + ": " + " ".join(f"{k}={v:.2e}" for k, v in e.items()))


@pytest.mark.parametrize("case", eo.ENC_CASES, ids=str)
def test_reference_error_encoder(case):
    """fp32 reference vs the oracle, and the ReLU-margin condition"""
    c = eo.enc_case(*case)
    assert c.margin >= eo.RELU_MARGIN
    e = eo.ref_err(c)
    _show(f"fp32 reference {case} margin={c.margin:.1e}", e)
    assert set(e) == set(c.exact) and len(e) == 18
    assert max(e.values()) < 2e-5                # a sane fp32 yardstick, far under today's 1e-4


def test_reference_error_encoder_pad_id():
    c = eo.enc_case(16, 2, 20, 0.1, "left", 7)
    assert bool((c.ids == 0).any()) and bool((c.ids == 7).any()) and c.margin >= eo.RELU_MARGIN
    assert max(eo.ref_err(c).values()) < 2e-5


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", eo.ATTN_CASES, ids=str)
def test_reference_error_attention(case, causal):
    e = eo.ref_err(eo.attn_case(*case, causal))
    _show(f"fp32 reference {case} causal={causal}", e)
    assert max(e.values()) < 2e-5


@pytest.mark.parametrize("M,n", eo.LN_CASES)
def test_reference_error_layernorm(M, n):
    for family in eo.ln_families(M, n):
        for rate in (None,) + eo.PRO_RATES:
            e = eo.ref_err(eo.ln_case(M, n, family, rate))
            _show(f"fp32 reference M={M} n={n} {family} rate={rate}", e)
            assert all(math.isfinite(v) for v in e.values())
            if family != "mean100" and n > 2:    # (n = 2: dx cancels to O(eps); mean 100: 1e-5)
                assert max(e["y"], e["rstd"], e["dx"]) < 2e-5


def test_layernorm_wide_cases_present():
    assert set(eo.LN_WIDE_CASES) <= set(eo.LN_CASES) and len(set(eo.LN_CASES)) == len(eo.LN_CASES)
    assert {(2, 32768), (2, 32767), (3, 12800), (3, 1279), (3, 1280), (3, 1281),
            (1030, 1025)} == set(eo.LN_WIDE_CASES)
    assert all(eo.ln_families(M, n) == ("randn", "const") for M, n in eo.LN_WIDE_CASES)
    assert all(eo.ln_families(M, n) == eo.LN_FAMILIES for M, n in eo.LN_CASES
               if (M, n) not in eo.LN_WIDE_CASES)


# ------------------------------------------------- tiled attention (T > 64)
def _plain_lse(qkv, valid, H, causal):
    B, T, E3 = qkv.shape
    E = E3 // 3
    q, k, _ = qkv.view(B, T, 3, H, E // H).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1) / math.sqrt(E // H)).masked_fill(~valid.view(B, 1, 1, T), -1e9)
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), -math.inf)
    return torch.logsumexp(s, -1)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("pattern", ["full", "lone"])
def test_mha_lse_matches_logsumexp(pattern, causal):
    c = eo.long_attn_case(2, 129, 16, 2, 0.0, pattern, causal, "randn")
    want = _plain_lse(c.qkv.to(F64), c.valid, c.H, causal)
    assert c.exact["lse"].shape == (2, 2, 129) and c.exact["lse"].dtype == F64
    assert float((c.exact["lse"] - want).abs().max()) < 1e-6     # (ulp of 1e9 in fp64: 1.2e-7)
    ordinary = want > eo.LSE_UNIFORM
    assert float((c.exact["lse"] - want)[ordinary].abs().max()) < 1e-12
    # sequence 0: every row uniform ("full"); its one valid key is the last, which every
    # row sees ("lone"), under the causal mask the last row only
    uni = c.exact["lse"][0] < eo.LSE_UNIFORM
    if pattern == "full":
        assert bool(uni.all())
    else:
        assert not bool(uni[:, -1].any()) and bool(uni[:, :-1].all()) == causal \
            and bool(uni[:, :-1].any()) == causal
    n = torch.arange(1, 130, dtype=F64) if causal else torch.full((129,), 129.0, dtype=F64)
    if pattern == "full":
        assert float((c.exact["lse"][0] - (-1e9 + torch.log(n))).abs().max()) < 1e-6


@pytest.mark.parametrize("T", [65, 512])
@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_long_attention_mask_equals_reference_bit_for_bit(T, rate):
    """row key stride 512 above T = 64; B * H = 6 > 1 so the stride matters"""
    keep = eo.attn_keep(3, 2, T, rate, eo.SEED, eo.STEP, stride=512)
    r = ref.attn_keep_scale(3, 2, T, rate, eo.SEED, eo.STEP, "cpu")
    assert torch.equal(keep, r != 0) and torch.equal(eo.mul(keep, rate).float(), r)
    assert not torch.equal(keep, eo.attn_keep(3, 2, T, rate, eo.SEED, eo.STEP, stride=64))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", [(2, 129, 16, 4, 0.1, "left", "randn"),
                                  (2, 129, 8, 2, 0.0, "left", "peaked"),
                                  (2, 129, 32, 2, 0.0, "none", "rising"),
                                  (2, 129, 128, 2, 0.0, "left", "falling")])
def test_long_mha_bwd_matches_autograd(case, causal):
    c = eo.long_attn_case(*case[:6], causal, case[6])
    qkv = c.qkv.to(F64).requires_grad_(True)
    out = _plain_mha(qkv, c.valid, c.H, c.m, causal)
    (g,) = torch.autograd.grad(out, qkv, c.dout.to(F64))
    assert _rel(c.exact["out"], out.detach()) < 1e-12
    assert _rel(c.exact["dqkv"], g) < 1e-10
    assert float((c.exact["lse"] - _plain_lse(qkv.detach(), c.valid, c.H, causal)).abs().max()) < 1e-6


def test_long_case_lists():
    """every case the tiled-attention test is to run is in LONG_CASES, once"""
    L = eo.LONG_CASES
    assert len(set(L)) == len(L)
    for dk in eo.LONG_DK:
        for T in (65, 128, 129, 511, 512):
            for p in eo.PATTERNS:
                for causal in (False, True):
                    assert (2, T, 2 * dk, 2, 0.0, p, causal, "randn", 0) in L
        for fam in ("peaked", "rising", "falling"):
            for T in (129, 512):
                for p in ("left", "none"):
                    for causal in (False, True):
                        assert (2, T, 2 * dk, 2, 0.0, p, causal, fam, 0) in L
    extra = {(T, E // 2) for B, T, E, H in eo.LONG_EDGE_SHAPES if T in (127, 192, 193, 320, 449)}
    assert {T for T, _ in extra} == {127, 192, 193, 320, 449}
    assert {dk for _, dk in extra} == set(eo.LONG_DK)
    for causal in (False, True):
        for s in [(2, 129, 16, 4), (2, 200, 64, 2), (1, 512, 64, 1)]:
            for r in (0.1, 0.5):
                assert s + (r, "left", causal, "randn", 0) in L
        for s in [(3, 65, 8, 1), (1, 200, 32, 1), (3, 129, 12, 3), (3, 129, 48, 3), (1, 65, 64, 1)]:
            assert s + (0.0, "left", causal, "randn", 0) in L
        assert (2, 129, 16, 2, 0.0, "left", causal, "randn", 7) in L
    # the causal grids of the tail shapes: B * H * nt forward, twice that backward; no forward
    # grid is a multiple of 8, and the backward grids have tails of 4, 0, 6, 6 and 4 blocks
    grids = [B * H * -(-T // 64) for B, T, E, H in eo.LONG_TAIL_SHAPES]
    assert grids == [6, 4, 27, 27, 2] and all(g % 8 for g in grids)
    assert [2 * g % 8 for g in grids] == [4, 0, 6, 6, 4]
    assert {E // H for B, T, E, H in eo.LONG_TAIL_SHAPES} == {4, 8, 16, 32, 64}
    c = eo.long_attn_case(2, 129, 16, 2, 0.0, "left", False, "randn", 7)
    assert bool((c.ids == 0).any()) and bool((c.ids == 7).any())
    assert bool(c.valid[c.ids == 0].all()) and not bool(c.valid[c.ids == 7].any())


@pytest.mark.parametrize("case", [c for c in eo.LONG_HARD_CASES if not c[6]], ids=str)
def test_long_family_conditions(case):
    """max |score| in [20, 80]; the per-tile maximum climbs (falls) from each
    64-key tile to the next (family_ok has the partial last tile of "rising")"""
    c = eo.long_attn_case(*case)
    print(f"{case} walk={c.walk} smax={c.smax:.1f} last={c.last:.3f} tiles="
          + " ".join(f"{t:.1f}" for t in c.tiles))
    assert eo.family_ok(c.family, c.T, c.smax, c.tiles, c.last)
    lo, hi = eo.LONG_SCORE_RANGE
    assert lo == 20.0 and hi == 80.0 and lo <= c.smax <= hi
    full = c.tiles[: c.T // 64]
    if c.family == "rising":
        assert all(b > a for a, b in zip(full, full[1:])) and (c.T % 64 == 0 or c.last >= 1 / 16)
    if c.family == "falling":
        assert all(b < a for a, b in zip(c.tiles, c.tiles[1:]))
    # the same inputs whatever the mask: the causal case shares them
    assert torch.equal(c.qkv, eo.long_attn_case(*case[:6], True, *case[7:]).qkv)


@pytest.mark.parametrize("case", eo.LONG_CASES, ids=str)
def test_reference_error_long_attention(case):
    """the yardstick of every tiled-attention case is finite and never 0, and
    the fp32 reference itself meets the uniform-row rule of lse"""
    c = eo.long_attn_case(*case)
    got = eo.ref_run(c)
    e = eo.errs(got, c.exact)
    _show(f"fp32 reference {case}", e)
    assert set(e) == {"out", "dqkv", "lse"}
    assert all(math.isfinite(v) and 0 < v < 1e-3 for v in e.values()), e
    eo.check_uniform_lse(got["lse"], c.exact["lse"])


def test_planted_lse_errors():
    c = eo.long_attn_case(2, 129, 16, 2, 0.0, "left", True, "randn")
    got = _clean(c)
    eo.check_uniform_lse(got["lse"], c.exact["lse"])
    uni = c.exact["lse"] < eo.LSE_UNIFORM
    assert bool(uni.any()) and not bool(uni.all())
    # an ordinary row off by 1e-4 relative: caught although uniform rows sit at -1e9
    bad = {k: v.clone() for k, v in got.items()}
    i = tuple(int(v[0]) for v in torch.nonzero(~uni, as_tuple=True))
    bad["lse"][i] += 1e-4 * max(1.0, abs(float(c.exact["lse"][i])))
    assert _rejected(bad, c, ["lse"])
    assert eo.row_err(bad["lse"], c.exact["lse"], "elem") < 1e-8     # ("elem" would pass it)
    # a uniform row a whole ulp off, and one that the backward would not recognise
    for v in (-1e9 + 128.0, -4e8):
        bad = {k: t.clone() for k, t in got.items()}
        bad["lse"][tuple(int(t[0]) for t in torch.nonzero(uni, as_tuple=True))] = v
        assert not _rejected(bad, c, ["lse"])
        with pytest.raises(AssertionError):
            eo.check_uniform_lse(bad["lse"], c.exact["lse"])
        with pytest.raises(AssertionError):
            eo.assert_within(bad, c, "planted")
    # a skipped rescale of the running sum: the early tiles' share of l kept at the old maximum
    r = eo.long_attn_case(2, 129, 16, 2, 0.0, "none", False, "rising")
    bad = _clean(r)
    bad["lse"] += 1e-3
    assert _rejected(bad, r, ["lse"])


# ------------------------------------------------------------- LDS formula
def test_max_fused_T_table():
    table = {(16, 4): 50, (16, 8): 63, (16, 16): 64,
             (32, 4): 25, (32, 8): 30, (32, 16): 34, (32, 32): 37}
    for E in (16, 32, 64):
        for dk in (4, 8, 16, 32):
            if E % dk == 0 and dk <= E:
                assert eo.max_fused_T(E, E // dk) == table.get((E, dk)), (E, dk)
    assert eo.param_floats(64) == 49984 and eo.param_floats(64) * 4 > eo.LDS_LIMIT
    assert all(eo.max_fused_T(64, H) is None for H in (1, 2, 4, 8, 16))
    assert eo.max_fused_T(16, 8) is None and eo.max_fused_T(48, 3) is None
    assert {(E, H, T) for E, H, T in eo.ENC_SHAPES if T > 20} == \
        {(E, E // dk, T) for (E, dk), T in table.items()}


# ---------------------------------------------- the checker rejects planted errors
def _rejected(got, case, names):
    ke, re_ = eo.errs(got, case.exact), eo.ref_err(case)
    return any(ke[k] > eo.bound(re_[k]) for k in names)


def _clean(case):
    got = {k: v.clone() for k, v in eo.ref_run(case).items()}
    assert not _rejected(got, case, list(case.exact))
    return got


def test_planted_y_row_scaled():
    c = eo.enc_case(16, 2, 20, 0.1, "left")
    got = _clean(c)
    t = int(got["y"][1].abs().amax(1).argmax())
    got["y"][1, t] *= 1 + 1e-4
    assert _rejected(got, c, ["y"])
    with pytest.raises(AssertionError):
        eo.assert_within(got, c, "planted")


def test_planted_ctx_head_from_another_head():
    c = eo.enc_case(32, 4, 30, 0.0, "left")
    got = _clean(c)
    got["ctx"][:, :, 8:16] = got["ctx"][:, :, 0:8]
    assert _rejected(got, c, ["ctx"])


def _oracle_with(c, masks):
    y, qkv, ctx, x1, f = eo.encoder_block_fwd(c.x, c.valid, c.params, c.H, masks)
    dx, grads = eo.encoder_block_bwd(c.x, c.valid, c.params, c.H, masks, c.dy)
    out = dict(y=y, qkv=qkv, ctx=ctx, x1=x1, f=f, dx=dx)
    out.update({"d" + n: t for n, t in zip(eo.PARAM_NAMES, grads)})
    return {k: v.float() for k, v in out.items()}


def test_planted_site_g_uses_site_f_constant():
    c = eo.enc_case(16, 2, 20, 0.1, "left")
    got = _oracle_with(c, eo.block_masks(c.B, c.T, c.E, c.H, c.rate, c.seed, c.step,
                                         site_g=eo.SITE_F))
    assert _rejected(got, c, ["y"]) and _rejected(got, c, ["dx"])
    assert not _rejected(_oracle_with(c, c.masks), c, list(c.exact))


def test_planted_row_key_stride_32():
    c = eo.enc_case(16, 2, 20, 0.1, "left")
    got = _oracle_with(c, eo.block_masks(c.B, c.T, c.E, c.H, c.rate, c.seed, c.step, stride=32))
    # (sequence 0, head 0 keeps its keys: the block-site masks of b = 0 are unchanged)
    assert torch.equal(got["y"][0] == 0, c.exact["y"][0] == 0)
    assert not torch.equal(got["y"][1] == 0, c.exact["y"][1] == 0)
    assert _rejected(got, c, ["y"]) and _rejected(got, c, ["ctx"])


def test_planted_ln_dgamma_swapped():
    c = eo.enc_case(16, 2, 20, 0.1, "left")
    got = _clean(c)
    got["dg1"], got["dg2"] = got["dg2"], got["dg1"]
    assert _rejected(got, c, ["dg1"]) and _rejected(got, c, ["dg2"])


@pytest.mark.parametrize("name", ["y", "dx", "mean"])
def test_planted_layernorm_rows_past_1024_left_at_fill(name):
    c = eo.ln_case(1030, 16, "randn", None)
    got = _clean(c)
    got[name][1024:] = 0.0
    assert _rejected(got, c, [name])


def test_planted_pad_key_dk():
    c = eo.attn_case(2, 33, 16, 4, 0.0, "left", False)
    got = _clean(c)
    E = c.E
    pad = (~c.valid)[:, :, None].expand(c.B, c.T, E)
    eo.check_exact_zero(got["dqkv"][..., E:2 * E], pad, "dK of PAD keys")
    assert not bool(c.exact["dqkv"][..., E:2 * E][pad].any())
    got["dqkv"][1, 0, E] = 1e-7
    with pytest.raises(AssertionError):
        eo.check_exact_zero(got["dqkv"][..., E:2 * E], pad, "dK of PAD keys")


def test_row_err_metric():
    e = torch.tensor([[1.0, 2.0], [1e-6, 0.0], [0.5, 0.25]], dtype=F64)
    g = e.clone()
    g[2, 1] += 0.05
    assert abs(eo.row_err(g, e) - 0.1) < 1e-12               # its own row's max
    g = e.clone()
    g[1, 1] += 1e-6
    assert abs(eo.row_err(g, e) - 1e-6 / 2e-3) < 1e-12       # a tiny row: 1e-3 of the global max
    assert eo.row_err(torch.tensor([1.0, math.nan]), torch.tensor([1.0, 2.0])) == math.inf
    v = torch.tensor([4.0, 1e-9], dtype=F64)
    assert abs(eo.row_err(v + 1e-3, v) - 1e-3 / 4.0) < 1e-9  # a bias: one row
    assert abs(eo.row_err(v + 1e-3, v, "elem") - 1e-3 / 4e-3) < 1e-9
    assert eo.bound(0.0) == 2.0 ** -20 and eo.bound(1e-6) == 8e-6

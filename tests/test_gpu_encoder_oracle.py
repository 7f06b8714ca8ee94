"""The Bert4Rec encoder kernels on MI355X against the float64 oracles of
tests/encoder_oracle.py, at every dispatch edge: the fused transformer block
(csrc/kernels/encoder.hip) at every reachable (E, d_k) and its LDS-limit T,
the one-wave attention core (attention.hip) at every d_k and T in {1, 2, 33,
63, 64}, and LayerNorm / the sequence prologue (layernorm.hip) at every
elements-per-lane class, its boundaries, the narrow-to-wide handover,
M > 1024 rows (the second grid-stride pass) and the wide path at its maximum
n = 32768, one short of it, around a multiple of its 256-thread stride and
with 1030 rows in its column pass. The tiled attention kernels (T > 64) have
tests/test_gpu_attention_long_oracle.py.

Bound, every checked tensor: row_err(kernel) <= max(8 * row_err(fp32
reference), 2^-20), the reference error measured on the CPU against the same
oracle (encoder_oracle.ref_err). Every test prints kernel error, reference
error and their ratio per tensor; profiles/encoder_oracle.md records the worst
ratios of one run."""
import pytest
import torch

from tdfo_amd import ops
from tests import encoder_oracle as eo

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _native():
    from tdfo_amd.ops import _ext

    assert _ext.load(), "native library must load on the GPU box"


def _dev(t):
    return t.to(DEV).contiguous()


def _step(v):
    return None if v is None else torch.tensor([v], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------- fused block
def _run_block(c, params=None, step="case", fill=NAN):
    """encoder_layer_fwd + encoder_layer_bwd on device copies of case ``c`` ->
    {y, qkv, ctx, x1, f, dx, d<param>...} on the CPU; outputs prefilled"""
    B, T, E, FF = c.B, c.T, c.E, 4 * c.E
    x, ids, dy = _dev(c.x), _dev(c.ids), _dev(c.dy)
    ps = [_dev(p) for p in (c.params if params is None else params)]
    st = _step(c.step if step == "case" else step)
    full = lambda *s: torch.full(s, fill, device=DEV)            # noqa: E731
    saved = [full(B, T, 3 * E), full(B, T, E), full(B, T, E), full(B, T, FF)]
    y = full(B, T, E)
    ops.encoder_layer_fwd(x, ids, st, ps, c.H, c.rate, c.seed, c.pad_id, eo.EPS, saved, y)
    P = ops.encoder_param_count(E, FF)
    assert P == eo.param_floats(E) == sum(p.numel() for p in c.params)
    dx, part, grad = full(B, T, E), full(B * P), full(P)
    ops.encoder_layer_bwd(x, ids, st, ps, c.H, c.rate, c.seed, c.pad_id, eo.EPS, saved, dy, dx,
                          part, grad)
    torch.cuda.synchronize()
    out = dict(y=y, qkv=saved[0], ctx=saved[1], x1=saved[2], f=saved[3], dx=dx)
    o = 0
    for n, p in zip(eo.PARAM_NAMES, c.params):
        out["d" + n] = grad[o:o + p.numel()].view(p.shape)
        o += p.numel()
    return {k: v.cpu() for k, v in out.items()}


def _check_block(c, got, tag):
    eo.assert_within(got, c, tag)
    eo.check_exact_zero(got["y"], c.masks.blk == 0, "y where the block dropout drops")
    assert bool((got["f"] >= 0).all())


@pytest.mark.parametrize("case", eo.ENC_CASES, ids=str)
def test_fused_block_matches_oracle(case):
    """y, the four saved intermediates, dx and the 12 parameter gradients"""
    c = eo.enc_case(*case)
    _check_block(c, _run_block(c), f"block {case}")


def test_fused_block_separate_qkv_bit_identical_e32():
    """the 16-tensor (separate Q / K / V) form equals the 12-tensor form"""
    c = eo.enc_case(32, 4, 30, 0.1, "left")
    E = c.E
    a = _run_block(c)
    sep = list(c.params[0].split(E, 0)) + list(c.params[1].split(E, 0)) + list(c.params[2:])
    b = _run_block(c, params=sep)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    _check_block(c, b, "block 16-tensor E=32")


def test_fused_block_pad_id_7():
    """pad_id = 7 with ids that hold both 0 (then an ordinary item) and 7"""
    c = eo.enc_case(16, 2, 20, 0.1, "left", 7)
    assert bool((c.ids == 0).any()) and bool((c.ids == 7).any())
    _check_block(c, _run_block(c), "block pad_id=7")


def test_fused_block_step_none_is_step_0_and_runs_repeat():
    c0 = eo.enc_case(16, 2, 20, 0.1, "left")
    none, zero, one = _run_block(c0, step=None), _run_block(c0, step=0), _run_block(c0, step=1)
    again = _run_block(c0, step=1)
    for k in none:
        assert torch.equal(none[k], zero[k]), k
        assert torch.equal(one[k], again[k]), k              # two runs: bit-identical
    assert not torch.equal(zero["y"], one["y"]) and not torch.equal(zero["dx"], one["dx"])
    assert torch.equal(zero["qkv"], one["qkv"])              # (before the first dropout site)
    # step 0 against the oracle with the step-0 masks
    m0 = eo.block_masks(c0.B, c0.T, c0.E, c0.H, c0.rate, c0.seed, 0)
    y0 = eo.encoder_block_fwd(c0.x, c0.valid, c0.params, c0.H, m0)[0]
    eo.check_exact_zero(zero["y"], m0.blk == 0, "y at step 0")
    assert eo.row_err(zero["y"], y0) <= eo.bound(eo.ref_err(c0)["y"])


def test_support_table_matches_lds_formula():
    """ops.encoder_layer_supported == T <= max_fused_T over the whole table"""
    for E in (16, 32, 64):
        for dk in (4, 8, 16, 32):
            if E % dk or dk > E:
                continue
            lim = eo.max_fused_T(E, E // dk)
            for T in range(1, 66):
                want = lim is not None and T <= lim
                assert ops.encoder_layer_supported(T, E, E // dk, 4 * E) == want, (T, E, dk)
    assert all(eo.max_fused_T(64, 64 // dk) is None for dk in (4, 8, 16, 32))
    assert not ops.encoder_layer_supported(20, 16, 2, 32)     # FF != 4E
    assert not ops.encoder_layer_supported(20, 16, 8, 64)     # d_k = 2
    assert not ops.encoder_layer_supported(0, 16, 2, 64)


@pytest.mark.parametrize("E,H,T", [(16, 4, 51), (16, 2, 64), (32, 8, 26), (32, 1, 38), (16, 1, 65),
                                   (64, 2, 1), (64, 16, 20), (64, 8, 8)])
def test_refused_shape_raises_on_host_and_device_stays_usable(E, H, T):
    """One past the LDS limit and every E = 64 shape: the host check raises,
    nothing is launched (the outputs keep their fill), and a valid call
    afterwards still matches the oracle."""
    lim = eo.max_fused_T(E, H)
    assert lim is None or T == lim + 1
    B, FF = 2, 4 * E
    g = torch.Generator().manual_seed(E + T)
    shapes = [(3 * E, E), (3 * E,), (E, E), (E,), (E,), (E,), (E,), (E,), (FF, E), (FF,), (E, FF),
              (E,)]
    ps = [torch.randn(*s, generator=g).to(DEV) for s in shapes]
    x = torch.randn(B, T, E, generator=g).to(DEV)
    ids = torch.ones(B, T, dtype=torch.int64, device=DEV)
    saved = [torch.full((B, T, w), 3.0, device=DEV) for w in (3 * E, E, E, FF)]
    y, dx = torch.full((B, T, E), 3.0, device=DEV), torch.full((B, T, E), 3.0, device=DEV)
    P = eo.param_floats(E)
    part, grad = torch.full((B * P,), 3.0, device=DEV), torch.full((P,), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.encoder_layer_fwd(x, ids, None, ps, H, 0.1, 1, 0, eo.EPS, saved, y)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.encoder_layer_bwd(x, ids, None, ps, H, 0.1, 1, 0, eo.EPS, saved, x, dx, part, grad)
    torch.cuda.synchronize()
    for t in saved + [y, dx, part, grad]:
        assert bool((t == 3.0).all())
    c = eo.enc_case(16, 2, 20, 0.1, "left")
    _check_block(c, _run_block(c), "block after a refused call")


# --------------------------------------------------------- short attention
SENTINEL = 12345.0


def _run_attn(c):
    qkv, ids, dout = _dev(c.qkv), _dev(c.ids), _dev(c.dout)
    out = torch.full((c.B, c.T, c.E), NAN, device=DEV)
    dqkv = torch.full((c.B, c.T, 3 * c.E), SENTINEL, device=DEV)
    st = _step(c.step)
    ops.attention_fwd(qkv, ids, c.H, c.rate, c.seed, st, 0, out, causal=c.causal)
    ops.attention_bwd(qkv, ids, dout, c.H, c.rate, c.seed, st, 0, dqkv, causal=c.causal)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), dqkv=dqkv.cpu())


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", eo.ATTN_CASES, ids=str)
def test_short_attention_matches_oracle(case, causal):
    """every d_k (4 .. 64) of the one-wave kernels, T in {1, 2, 33, 63, 64}"""
    c = eo.attn_case(*case, causal)
    got = _run_attn(c)
    assert not bool((got["dqkv"] == SENTINEL).any()), "dqkv not fully written"
    eo.assert_within(got, c, f"attention {case} causal={causal}")
    E = c.E
    pad = (~c.valid)[:, :, None].expand(c.B, c.T, E)
    eo.check_exact_zero(got["dqkv"][..., E:2 * E], pad, "dK rows of PAD keys")
    again = _run_attn(c)
    assert torch.equal(got["out"], again["out"]) and torch.equal(got["dqkv"], again["dqkv"])


# -------------------------------------------------- LayerNorm and prologue
def _run_ln(c, gidx=None, flat=None):
    M, n = c.M, c.n
    x, g, gamma, beta = _dev(c.x), _dev(c.g), _dev(c.gamma), _dev(c.beta)
    full = lambda *s: torch.full(s, NAN, device=DEV)             # noqa: E731
    y, mean, rstd, dx = full(M, n), full(M), full(M), full(M, n)
    k = 2 if c.rate is None else 3
    part = torch.empty(ops.layernorm_parts(M, n) * k * n, device=DEV)
    out = full(k * n) if flat is None else flat
    if c.rate is None:
        ops.layernorm_fwd(x, n, eo.EPS, gamma, beta, y, mean, rstd)
        ops.layernorm_bwd(x, g, n, gamma, mean, rstd, dx, part, out)
    else:
        pos, st = _dev(c.pos), _step(c.step)
        ops.seq_prologue_fwd(x, pos, n, eo.EPS, gamma, beta, c.rate, c.seed, st, y, mean, rstd)
        ops.seq_prologue_bwd(x, pos, g, n, gamma, mean, rstd, c.rate, c.seed, st, dx, part, out,
                             gidx=gidx)
    torch.cuda.synchronize()
    got = dict(y=y, mean=mean, rstd=rstd, dx=dx)
    if flat is None:
        got.update(dgamma=out[:n], dbeta=out[n:2 * n])
        if k == 3:
            got["dpos"] = out[2 * n:]
    return {k_: v.cpu() for k_, v in got.items()}


@pytest.mark.parametrize("M,n", eo.LN_CASES)
def test_layernorm_matches_oracle(M, n):
    """y, mean, rstd, dx, dgamma, dbeta on randn rows, rows of mean 100 and
    std 1, and a constant row with zeros in gamma (encoder_oracle.ln_families:
    the wide sizes past 3200 test indexing and run without mean 100)"""
    for family in eo.ln_families(M, n):
        c = eo.ln_case(M, n, family, None)
        eo.assert_within(_run_ln(c), c, f"layernorm M={M} n={n} {family}")


@pytest.mark.parametrize("M,n", eo.LN_CASES)
def test_seq_prologue_matches_oracle(M, n):
    """the same plus dpos, at dropout rates 0, 0.1 and 0.5; a dropped y is exactly 0"""
    for family in eo.ln_families(M, n):
        for rate in eo.PRO_RATES:
            c = eo.ln_case(M, n, family, rate)
            got = _run_ln(c)
            eo.assert_within(got, c, f"prologue M={M} n={n} {family} rate={rate}")
            eo.check_exact_zero(got["y"], c.m == 0, "dropped y")


@pytest.mark.parametrize("M,n", [(5, 320), (1030, 16)])
def test_seq_prologue_narrow_gidx_writes_through(M, n):
    """[dgamma | dbeta | dpos][j] lands at flat[gidx[j]] of a permuted flat
    buffer on the narrow path; untouched slots keep their fill"""
    c = eo.ln_case(M, n, "randn", 0.1)
    want = _run_ln(c)
    g = torch.Generator().manual_seed(n)
    gidx = (torch.randperm(4 * n, generator=g)[: 3 * n] + 17).to(DEV).contiguous()
    flat = torch.full((4 * n + 50,), 123.0, device=DEV)
    got = _run_ln(c, gidx=gidx, flat=flat)
    assert torch.equal(got["dx"], want["dx"])
    scattered = flat[gidx].cpu()
    assert torch.equal(scattered, torch.cat([want["dgamma"], want["dbeta"], want["dpos"]]))
    untouched = torch.ones_like(flat, dtype=torch.bool)
    untouched[gidx] = False
    assert bool((flat[untouched] == 123.0).all())
    got.update(dgamma=scattered[:n], dbeta=scattered[n:2 * n], dpos=scattered[2 * n:])
    eo.assert_within(got, c, f"prologue gidx M={M} n={n}")

"""float64 oracles of the Bert4Rec encoder kernels and the shared cases of
their tests: the counter-hash dropout masks, LayerNorm and the sequence
prologue, the multi-head attention core (with the row log-sum-exp the tiled
kernels save, and the hard input families of their cases), and the fused
pre-norm transformer block (forward with its four saved intermediates,
backward with dx and the 12 parameter gradients).

Everything is written out by hand in float64 without autograd and without
``tdfo_amd.ops.reference`` (tests/test_encoder_oracle.py checks the backwards
against torch.autograd of a plain composition and the masks against the
reference's, bit for bit). Only ``ref_err`` at the bottom runs the fp32
reference: its error against the oracle is the yardstick of the GPU bound.

    h1 = LN1(x)            qkv = h1 Wqkv^T + bqkv
    ctx = MHA(qkv)         x1 = x + m_a (ctx Wo^T + bo)
    h2 = LN2(x1)           z = h2 W1^T + b1,  f = relu(z)
    x2 = x1 + m_g ((m_f f) W2^T + b2)         y = m_blk x2

Dropout multiplier m = keep / (1 - rate); keep is decided in integers:
(hash >> 8) * 2^-24 >= float32(rate), both sides exact in float64.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

F64 = torch.float64
EPS = 1e-5
FLOOR = 2.0 ** -20       # see bound()
FACTOR = 8.0
RELU_MARGIN = 2e-5
LDS_LIMIT = 160 * 1024
_M32 = 0xFFFFFFFF

SITE_A, SITE_F, SITE_G, SITE_BLK = 1, 2, 3, 4
SITE_CONST = 0x27D4EB2F
STEP_CONST = 0x632BE5AB
PRO_CONST = 0x51ED270B
PARAM_NAMES = ("wqkv", "bqkv", "wo", "bo", "g1", "be1", "g2", "be2", "w1", "b1", "w2", "b2")


# ------------------------------------------------------------------ dropout
def hash3(a, b, c):
    """uint32 counter hash of the kernels, in int64 tensors / ints"""
    h = ((a * 0x9E3779B1) & _M32) ^ (((b + 0x7F4A7C15) * 0x85EBCA77) & _M32) \
        ^ (((c + 0x165667B1) * 0xC2B2AE3D) & _M32)
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def _keep(r, rate):
    """integer-exact keep decision: 24 bits scaled by 2^-24 (exact in fp64)
    against the rate as the kernel holds it, a float32"""
    return (r >> 8).to(F64) * 2.0 ** -24 >= float(np.float32(rate))


def _ar(n):
    return torch.arange(n, dtype=torch.int64)


def _seed(seed, step):
    return (seed ^ ((step * STEP_CONST) & _M32)) & _M32


def attn_keep(B, H, T, rate, seed, step, stride=64):
    """[B, H, T, T] bool; row key (b*H + h) * stride + i, column j"""
    if rate <= 0:
        return torch.ones(B, H, T, T, dtype=torch.bool)
    row = _ar(B * H).view(B, H, 1, 1) * stride + _ar(T).view(1, 1, T, 1)
    return _keep(hash3(torch.tensor(_seed(seed, step)), row, _ar(T).view(1, 1, 1, T)), rate)


def site_keep(B, T, N, rate, seed, step, site, stride=64):
    """[B, T, N] bool of a block-dropout site; row key b * stride + t"""
    if rate <= 0:
        return torch.ones(B, T, N, dtype=torch.bool)
    sd = (_seed(seed, step) ^ ((site * SITE_CONST) & _M32)) & _M32
    row = _ar(B).view(B, 1, 1) * stride + _ar(T).view(1, T, 1)
    return _keep(hash3(torch.tensor(sd), row, _ar(N).view(1, 1, N)), rate)


def prologue_keep(M, n, rate, seed, step):
    """[M, n] bool of the sequence prologue; key (row, element)"""
    if rate <= 0:
        return torch.ones(M, n, dtype=torch.bool)
    sd = ((seed & _M32) ^ ((step * STEP_CONST) & _M32) ^ PRO_CONST) & _M32
    return _keep(hash3(torch.tensor(sd), _ar(M).view(M, 1) & _M32, _ar(n).view(1, n)), rate)


def mul(keep, rate):
    return keep.to(F64) / (1.0 - rate) if rate > 0 else keep.to(F64)


def block_masks(B, T, E, H, rate, seed, step, stride=64, site_g=SITE_G):
    """the five multipliers of the fused block"""
    return SimpleNamespace(
        p=mul(attn_keep(B, H, T, rate, seed, step, stride), rate),
        a=mul(site_keep(B, T, E, rate, seed, step, SITE_A, stride), rate),
        f=mul(site_keep(B, T, 4 * E, rate, seed, step, SITE_F, stride), rate),
        g=mul(site_keep(B, T, E, rate, seed, step, site_g, stride), rate),
        blk=mul(site_keep(B, T, E, rate, seed, step, SITE_BLK, stride), rate))


# ---------------------------------------------------------------- LayerNorm
def layernorm_fwd(x, gamma, beta, eps=EPS):
    """x [M, n] -> y, mean [M], rstd [M] (biased variance)"""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    n = x.shape[-1]
    mean = x.sum(-1) / n
    d = x - mean[..., None]
    rstd = 1.0 / torch.sqrt((d * d).sum(-1) / n + eps)
    return d * rstd[..., None] * gamma + beta, mean, rstd


def layernorm_bwd(x, g, gamma, mean, rstd):
    """-> dx, dgamma, dbeta; x, g [M, n]"""
    x, g, gamma = x.to(F64), g.to(F64), gamma.to(F64)
    n = x.shape[-1]
    xh = (x - mean[..., None]) * rstd[..., None]
    gg = g * gamma
    m1 = gg.sum(-1, keepdim=True) / n
    m2 = (gg * xh).sum(-1, keepdim=True) / n
    dx = rstd[..., None] * (gg - m1 - xh * m2)
    lead = tuple(range(x.dim() - 1))
    return dx, (g * xh).sum(lead), g.sum(lead)


def seq_prologue_fwd(x, pos, gamma, beta, m, eps=EPS):
    """y = m * LN(x + pos) -> y, mean, rstd"""
    y, mean, rstd = layernorm_fwd(x.to(F64) + pos.to(F64), gamma, beta, eps)
    return y * m, mean, rstd


def seq_prologue_bwd(x, pos, g, gamma, mean, rstd, m):
    """-> dx, dgamma, dbeta, dpos"""
    dx, dg, db = layernorm_bwd(x.to(F64) + pos.to(F64), g.to(F64) * m, gamma, mean, rstd)
    return dx, dg, db, dx.sum(0)


# ---------------------------------------------------------------- attention
def _heads(t, H):
    B, T, E = t.shape
    return t.view(B, T, H, E // H).permute(0, 2, 1, 3)          # [B, H, T, dk]


def _masked_scores(qkv, valid, H, causal):
    """-> q, k, v [B, H, T, dk], the masked scores [B, H, T, T] and the mask of
    the keys that carry a gradient (visible and not PAD)"""
    B, T, E3 = qkv.shape
    E = E3 // 3
    q, k, v = (_heads(qkv[..., i * E:(i + 1) * E], H) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(E // H)
    keym = valid.view(B, 1, 1, T).expand(B, H, T, T)
    s = torch.where(keym, s, torch.full_like(s, -1e9))           # masked_fill, not -inf
    if causal:
        see = torch.ones(T, T, dtype=torch.bool).tril()
        s = torch.where(see, s, torch.full_like(s, -math.inf))
        keym = keym & see
    return q, k, v, s, keym


def _attn_probs(qkv, valid, H, causal):
    q, k, v, s, keym = _masked_scores(qkv, valid, H, causal)
    s = s - s.max(-1, keepdim=True).values
    e = torch.exp(s)
    return q, k, v, e / e.sum(-1, keepdim=True), keym


def mha_lse(qkv, valid, H, causal=False):
    """[B, H, T] log-sum-exp of the masked scores: PAD keys at -1e9, future
    keys excluded, no dropout (a row whose visible keys are all PAD: -1e9 +
    log of their number)"""
    _, _, _, s, _ = _masked_scores(qkv.to(F64), valid, H, causal)
    mx = s.max(-1).values
    return mx + torch.log(torch.exp(s - mx[..., None]).sum(-1))


def mha_fwd(qkv, valid, H, m, causal=False):
    """qkv [B, T, 3E], valid [B, T] bool (key is not PAD), m [B, H, T, T]
    dropout multiplier on P -> out [B, T, E]"""
    qkv = qkv.to(F64)
    B, T, E3 = qkv.shape
    q, k, v, p, _ = _attn_probs(qkv, valid, H, causal)
    return ((p * m) @ v).permute(0, 2, 1, 3).reshape(B, T, E3 // 3)


def mha_bwd(qkv, valid, dout, H, m, causal=False):
    """-> dqkv [B, T, 3E]; a masked key holds a constant score: no gradient"""
    qkv, dout = qkv.to(F64), dout.to(F64)
    B, T, E3 = qkv.shape
    E = E3 // 3
    q, k, v, p, keym = _attn_probs(qkv, valid, H, causal)
    do = _heads(dout, H)
    dp = (do @ v.transpose(-1, -2)) * m
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    ds = torch.where(keym, ds, torch.zeros_like(ds)) / math.sqrt(E // H)
    parts = (ds @ k, ds.transpose(-1, -2) @ q, (p * m).transpose(-1, -2) @ do)
    return torch.cat([t.permute(0, 2, 1, 3).reshape(B, T, E) for t in parts], -1)


# ------------------------------------------------------------- fused block
def encoder_block_fwd(x, valid, params, H, masks, eps=EPS, full=False):
    """-> y, qkv, ctx, x1, f (post-ReLU, pre-dropout); full: also z"""
    x = x.to(F64)
    wqkv, bqkv, wo, bo, g1, be1, g2, be2, w1, b1, w2, b2 = (p.to(F64) for p in params)
    h1, _, _ = layernorm_fwd(x, g1, be1, eps)
    qkv = h1 @ wqkv.t() + bqkv
    ctx = mha_fwd(qkv, valid, H, masks.p)
    x1 = x + (ctx @ wo.t() + bo) * masks.a
    h2, _, _ = layernorm_fwd(x1, g2, be2, eps)
    z = h2 @ w1.t() + b1
    f = torch.clamp_min(z, 0.0)
    x2 = x1 + ((f * masks.f) @ w2.t() + b2) * masks.g
    out = (x2 * masks.blk, qkv, ctx, x1, f)
    return out + (z,) if full else out


def encoder_block_bwd(x, valid, params, H, masks, dy, eps=EPS):
    """-> dx, [12 parameter gradients in the POff order]"""
    x, dy = x.to(F64), dy.to(F64)
    wqkv, bqkv, wo, bo, g1, be1, g2, be2, w1, b1, w2, b2 = (p.to(F64) for p in params)
    E = x.shape[-1]
    h1, mu1, rs1 = layernorm_fwd(x, g1, be1, eps)
    qkv = h1 @ wqkv.t() + bqkv
    ctx = mha_fwd(qkv, valid, H, masks.p)
    x1 = x + (ctx @ wo.t() + bo) * masks.a
    h2, mu2, rs2 = layernorm_fwd(x1, g2, be2, eps)
    z = h2 @ w1.t() + b1
    fd = torch.clamp_min(z, 0.0) * masks.f
    fl = lambda t: t.reshape(-1, t.shape[-1])                    # noqa: E731
    dx2 = dy * masks.blk
    dg = dx2 * masks.g
    dw2, db2 = fl(dg).t() @ fl(fd), fl(dg).sum(0)
    df = (dg @ w2) * masks.f * (z > 0)
    dw1, db1 = fl(df).t() @ fl(h2), fl(df).sum(0)
    d1, dg2, dbe2 = layernorm_bwd(x1, df @ w1, g2, mu2, rs2)
    dx1 = dx2 + d1
    da = dx1 * masks.a
    dwo, dbo = fl(da).t() @ fl(ctx), fl(da).sum(0)
    dqkv = mha_bwd(qkv, valid, da @ wo, H, masks.p)
    dwqkv, dbqkv = fl(dqkv).t() @ fl(h1), fl(dqkv).sum(0)
    d0, dg1, dbe1 = layernorm_bwd(x, dqkv @ wqkv, g1, mu1, rs1)
    return dx1 + d0, [dwqkv, dbqkv, dwo, dbo, dg1, dbe1, dg2, dbe2, dw1, db1, dw2, db2]


# -------------------------------------------------------------- LDS budget
def param_floats(E):
    """Wqkv bqkv Wo bo g1 be1 g2 be2 W1 b1 W2 b2 with FF = 4E"""
    return 3 * E * E + 3 * E + E * E + E + 4 * E + 4 * E * E + 4 * E + 4 * E * E + E


def fused_lds_bytes(T, E, H):
    """LDS of the fused block, the larger of its two kernels, from their
    layout comments. forward: x, LN out, ctx, x1 [T][E] each, qkv [T][3E],
    f [T][4E], scores [H][T][T], key flags [T], the staged parameters.
    backward: dx, temp, LN out, xhat, dLN, ctx [T][E] each, rstd [T], f and df
    [T][4E], qkv and dqkv [T][3E], P~ and dS [H][T][T], rowdot [H][T], x0
    [T][E], key flags [T], the staged parameters."""
    TE, FF, P = T * E, 4 * E, param_floats(E)
    fwd = 4 * TE + 3 * TE + T * FF + H * T * T + T + P
    bwd = 6 * TE + T + 2 * T * FF + 2 * 3 * TE + 2 * H * T * T + H * T + TE + T + P
    return 4 * max(fwd, bwd)


def max_fused_T(E, H):
    """largest supported T (<= 64: the kernels index keys by lane), or None"""
    if E not in (16, 32, 64) or H < 1 or E % H or E // H not in (4, 8, 16, 32):
        return None
    ok = [T for T in range(1, 65) if fused_lds_bytes(T, E, H) <= LDS_LIMIT]
    return max(ok) if ok else None


# ------------------------------------------------------------------ metrics
def _rows(t, kind):
    t = t.detach().cpu().to(F64)
    if kind == "vec":                      # a bias: the whole vector is one row
        return t.reshape(1, -1)
    if kind == "elem":                     # mean / rstd: every row's scalar on its own
        return t.reshape(-1, 1)
    return t.reshape(-1, t.shape[-1])      # a token of [B, T, .], an output row of a weight


def row_err(got, exact, kind=None):
    """max over rows of max|got - exact| / max(max|exact_row|, 1e-3 max|exact|)"""
    if kind is None:
        kind = "vec" if exact.dim() == 1 else "row"
    g, e = _rows(got, kind), _rows(exact, kind)
    assert g.shape == e.shape, (g.shape, e.shape)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    den = torch.clamp_min(e.abs().amax(1), 1e-3 * float(e.abs().max()))
    den = torch.where(den > 0, den, torch.ones_like(den))        # (exact all 0: absolute)
    return float(((g - e).abs().amax(1) / den).max())


def bound(ref_e):
    """8 x the fp32 reference's own error (the factor covers __expf, rsqrtf,
    the 4-chain FMA order and the wave / block reduction orders), floored at
    2^-20 so that an output the reference hits exactly stays passable."""
    return max(FACTOR * ref_e, FLOOR)


def check_exact_zero(got, where, what=""):
    """elements the maths makes exactly 0 (dropped outputs, dK of PAD keys)"""
    bad = got.detach().cpu()[where] != 0
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(where.sum())} elements not exactly 0"


# -------------------------------------------------------------------- cases
PATTERNS = ("left", "full", "lone", "none")
# fused block: every reachable (E, H) at its LDS-limit T, T = 1, the recipe shape
ENC_SHAPES = [(16, 4, 50), (16, 2, 63), (16, 1, 64), (32, 8, 25), (32, 4, 30), (32, 2, 34),
              (32, 1, 37), (16, 2, 1), (16, 2, 20)]
ENC_RATES = {s: (0.0, 0.1) for s in ENC_SHAPES}
ENC_RATES[(16, 2, 63)] = ENC_RATES[(32, 4, 30)] = (0.0, 0.1, 0.3)
ENC_CASES = [(E, H, T, r, p) for (E, H, T) in ENC_SHAPES for r in ENC_RATES[(E, H, T)]
             for p in PATTERNS]
# short attention (B, T, E, H)
ATTN_SHAPES = [(2, 64, 16, 4), (2, 33, 16, 4), (2, 1, 8, 2), (2, 2, 16, 2), (3, 63, 64, 4),
               (2, 64, 64, 2), (2, 64, 64, 1), (2, 63, 128, 2)]
ATTN_CASES = [s + (0.0, p) for s in ATTN_SHAPES for p in PATTERNS]
ATTN_CASES += [(2, 64, 16, 4, 0.25, "left"), (2, 64, 64, 1, 0.25, "left")]
# tiled attention (attention_long.hip, 64 < T <= 512): B = 2, H = 2, E = 2 d_k
LONG_DK = (4, 8, 16, 32, 64)
LONG_FAMILIES = ("randn", "peaked", "rising", "falling")
LONG_TILE = 64
# every operand width (d_k 4: scalar, 8: float2, >= 16: float4) and column-block
# count (1, 2, 4) at one key past a tile, whole tiles, one past two tiles, one
# short of the maximum and the maximum; five more T at one d_k each
LONG_EDGE_SHAPES = [(2, T, 2 * dk, 2) for dk in LONG_DK for T in (65, 128, 129, 511, 512)]
LONG_EDGE_SHAPES += [(2, T, 2 * dk, 2) for T, dk in zip((127, 192, 193, 320, 449), LONG_DK)]
# causal grids B * H * nt (forward) and twice that (backward) that are no
# multiple of 8: the blocks past the last whole group of 8 keep their index
LONG_TAIL_SHAPES = [(3, 65, 8, 1), (1, 200, 32, 1), (3, 129, 12, 3), (3, 129, 48, 3),
                    (1, 65, 64, 1)]
LONG_DROP_SHAPES = [(2, 129, 16, 4), (2, 200, 64, 2), (1, 512, 64, 1)]
LONG_PAD7_SHAPE = (2, 129, 16, 2)
# (B, T, E, H, rate, pattern, causal, family, pad_id)
LONG_CASES = [s + (0.0, p, c, "randn", 0) for s in LONG_EDGE_SHAPES for p in PATTERNS
              for c in (False, True)]
LONG_HARD_CASES = [(2, T, 2 * dk, 2, 0.0, p, c, f, 0) for f in LONG_FAMILIES[1:]
                   for T in (129, 512) for dk in LONG_DK for p in ("left", "none")
                   for c in (False, True)]
LONG_CASES += LONG_HARD_CASES
LONG_CASES += [s + (r, "left", c, "randn", 0) for s in LONG_DROP_SHAPES for r in (0.1, 0.5)
               for c in (False, True)]
LONG_CASES += [s + (0.0, "left", c, "randn", 0) for s in LONG_TAIL_SHAPES for c in (False, True)]
LONG_CASES += [LONG_PAD7_SHAPE + (0.0, "left", c, "randn", 7) for c in (False, True)]
# block order: the causal grid-tail cases and the paper shape
LONG_ORDER_CASES = [s + (0.0, "left", True, "randn", 0)
                    for s in LONG_TAIL_SHAPES + [(2, 200, 64, 2)]]
LONG_PEAK = 2.5          # "peaked": the q and k thirds times this
LONG_RAMP = 6.0          # "rising" / "falling": a = LONG_RAMP * d_k^(1/4)
LONG_SCORE_RANGE = (20.0, 80.0)

LN_N = (1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 512, 513, 1023, 1024, 1025, 3200)
LN_CASES = [(M, n) for n in LN_N for M in (1, 3, 5)] + [(1030, n) for n in (16, 320, 1024)]
LN_FAMILIES = ("randn", "mean100", "const")
# the wide path (ln_wide_*, 1024 < n <= 32768): the maximum width and one short
# of it, the paper's n = T E = 12800, n around a multiple of the 256-thread
# stride, and 1030 rows in the column pass. These sizes test indexing, not the
# variance formula (mean100 reaches the wide kernels at n = 1025 and 3200).
LN_WIDE_CASES = [(2, 32768), (2, 32767), (3, 12800), (3, 1279), (3, 1280), (3, 1281),
                 (1030, 1025)]
LN_CASES += LN_WIDE_CASES


def ln_families(M, n):
    return ("randn", "const") if (M, n) in LN_WIDE_CASES else LN_FAMILIES
PRO_RATES = (0.0, 0.1, 0.5)
# The constant row: variance 0, so rstd = eps^-1/2 = 316 multiplies whatever
# rounding the fp32 row mean carries (up to an ulp of the constant, e.g. from
# sum * fl(1/n)). That amplification is the operation's, not a kernel's; the
# constant 2^-8 keeps it at 316 * 2^-32 = 7e-8, below the 2^-20 floor, while a
# kernel that mishandles zero variance (NaN, inf, a wrong eps) still fails.
LN_CONST = 2.0 ** -8
SEED, STEP = 0x5EED + 7919, 5


def make_ids(B, T, pattern, g, pad_id=0, hi=50):
    """[B, T] int64: sequence 0 by ``pattern``, the others left-padded by T // 4"""
    ids = torch.randint(1, hi, (B, T), generator=g)
    ids[ids == pad_id] = hi
    ids[:, : T // 4] = pad_id
    if pattern == "full":
        ids[0] = pad_id
    elif pattern == "lone":
        ids[0, : T - 1] = pad_id
        ids[0, T - 1] = hi + 1
    elif pattern == "none":
        ids[0] = torch.randint(hi, 2 * hi, (T,), generator=g)
    return ids


def _enc_inputs(E, H, T, pattern, seed, pad_id):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=0.3: torch.randn(*s, generator=g) * sc     # noqa: E731
    FF, B = 4 * E, 2
    params = [r(3 * E, E), r(3 * E, sc=0.1), r(E, E), r(E, sc=0.1), 1 + r(E, sc=0.1),
              r(E, sc=0.1), 1 + r(E, sc=0.1), r(E, sc=0.1), r(FF, E), r(FF, sc=0.1), r(E, FF),
              r(E, sc=0.1)]
    x = torch.randn(B, T, E, generator=g)
    dy = torch.randn(B, T, E, generator=g)
    ids = make_ids(B, T, pattern, g, pad_id)
    if pad_id != 0:                 # ids hold both 0 and pad_id: 0 is then an ordinary item
        ids[1, T - 1] = 0
    return params, x, dy, ids


@functools.lru_cache(maxsize=None)
def enc_case(E, H, T, rate, pattern, pad_id=0):
    """CPU fp32 inputs and the fp64 oracle of one fused-block case. Walks at
    most 16 seeds for inputs whose FFN pre-activations all satisfy
    |z| >= RELU_MARGIN in fp64 (an fp32 dot product of 16-32 O(1) terms errs
    by a few 1e-7: a unit nearer 0 may legitimately flip its ReLU mask and
    move dW1 / dx by O(1)); a condition on the inputs, not a tolerance.
    Cached: treat as read-only."""
    base = 100000 * E + 1000 * H + 10 * T + int(rate * 10) + 7 * PATTERNS.index(pattern) + pad_id
    for k in range(16):
        params, x, dy, ids = _enc_inputs(E, H, T, pattern, base * 16 + k, pad_id)
        valid = ids != pad_id
        masks = block_masks(2, T, E, H, rate, SEED, STEP)
        y, qkv, ctx, x1, f, z = encoder_block_fwd(x, valid, params, H, masks, full=True)
        margin = float(z.abs().min())
        if margin >= RELU_MARGIN:
            break
    else:
        raise AssertionError(f"no seed of 16 gives a ReLU margin >= {RELU_MARGIN}")
    dx, grads = encoder_block_bwd(x, valid, params, H, masks, dy)
    exact = dict(y=y, qkv=qkv, ctx=ctx, x1=x1, f=f, dx=dx)
    exact.update({"d" + n: t for n, t in zip(PARAM_NAMES, grads)})
    return SimpleNamespace(E=E, H=H, T=T, B=2, rate=rate, pattern=pattern, pad_id=pad_id,
                           params=params, x=x, dy=dy, ids=ids, valid=valid, masks=masks,
                           margin=margin, seed=SEED, step=STEP, exact=exact)


@functools.lru_cache(maxsize=None)
def attn_case(B, T, E, H, rate, pattern, causal):
    """Cached: treat as read-only."""
    g = torch.Generator().manual_seed(1000 * T + 10 * E + H + 7 * PATTERNS.index(pattern))
    qkv = torch.randn(B, T, 3 * E, generator=g)
    dout = torch.randn(B, T, E, generator=g)
    ids = make_ids(B, T, pattern, g)
    valid = ids != 0
    m = mul(attn_keep(B, H, T, rate, SEED, STEP), rate)
    exact = dict(out=mha_fwd(qkv, valid, H, m, causal), dqkv=mha_bwd(qkv, valid, dout, H, m, causal))
    return SimpleNamespace(B=B, T=T, E=E, H=H, rate=rate, pattern=pattern, causal=causal, qkv=qkv,
                           dout=dout, ids=ids, valid=valid, m=m, seed=SEED, step=STEP, exact=exact)


def score_stats(qkv, H):
    """float64 scores q.k / sqrt(d_k) of every (query, key) pair, no mask ->
    (max |score|, [per 64-key tile: mean over all rows of the tile's maximum],
    fraction of the rows whose maximum lies in the last tile)"""
    qkv = qkv.to(F64)
    E = qkv.shape[-1] // 3
    q, k = _heads(qkv[..., :E], H), _heads(qkv[..., E:2 * E], H)
    s = q @ k.transpose(-1, -2) / math.sqrt(E // H)
    tmax = torch.stack([t.max(-1).values for t in s.split(LONG_TILE, -1)], -1)
    last = float((tmax.argmax(-1) == tmax.shape[-1] - 1).double().mean())
    return float(s.abs().max()), [float(v) for v in tmax.reshape(-1, tmax.shape[-1]).mean(0)], last


def family_ok(family, T, smax, tiles, last):
    """The conditions a hard input family is there for: max |score| within
    LONG_SCORE_RANGE, and for "rising" ("falling") the mean over rows of the
    tile's maximum score increases (decreases) from each 64-key tile to the
    next. A partial last tile is held to the same for "falling". For "rising"
    it cannot be: at T = 129 its one key carries the ramp's top, 36 * 128 / 129,
    but the tile before takes the maximum over 64 keys of ramp + noise (the
    terms q0.k0 and a u.k0 / sqrt(d_k), sigma 2.3 to 4.4), about 4 above the
    ramp, at every a that keeps max |score| under 80. What that tile is there
    for is a rescale in the last, partial tile, so it is required to hold the
    row's overall maximum in at least one row in 16 (``last`` is that
    fraction)."""
    lo, hi = LONG_SCORE_RANGE
    if not lo <= smax <= hi:
        return False
    full = T // LONG_TILE
    steps = [b - a for a, b in zip(tiles, tiles[1:])]
    if family == "rising":
        return all(d > 0 for d in steps[:full - 1]) and (T % LONG_TILE == 0 or last >= 1 / 16)
    if family == "falling":
        return all(d < 0 for d in steps)
    return True


@functools.lru_cache(maxsize=None)
def long_attn_case(B, T, E, H, rate, pattern, causal, family, pad_id=0):
    """CPU fp32 inputs and the fp64 oracle (out, dqkv, lse) of one case of the
    tiled attention kernels. Families: "randn"; "peaked", the q and k thirds
    times LONG_PEAK; "rising", a unit vector u per head, a (j / T) u added to
    key j and a u to every query, a = LONG_RAMP d_k^(1/4), so the scores climb
    by a^2 / sqrt(d_k) = 36 along the keys, the winning keys sit in the last
    tiles and the online softmax rescales by a small alpha at every tile;
    "falling", the ramp reversed ((T - 1 - j) / T), so every later tile adds
    terms that underflow against the running max. A hard family walks at most
    16 seeds for inputs that meet family_ok (at d_k = 4 the ramp's noise term
    a u.k0 / sqrt(d_k) is shared by all rows of a head and can reorder two
    neighbouring tiles): a condition on the inputs. Cached: read-only."""
    dk = E // H
    base = 1000 * T + 10 * E + H + 7 * PATTERNS.index(pattern) \
        + 100003 * LONG_FAMILIES.index(family) + 1009 * pad_id
    for walk in range(16):
        g = torch.Generator().manual_seed(base * 16 + walk)
        qkv = torch.randn(B, T, 3 * E, generator=g)
        dout = torch.randn(B, T, E, generator=g)
        ids = make_ids(B, T, pattern, g, pad_id)
        if pad_id != 0:             # ids hold both 0 and pad_id: 0 is then an ordinary item
            ids[B - 1, T - 1] = 0
        if family == "peaked":
            qkv[..., :2 * E] *= LONG_PEAK
        elif family in ("rising", "falling"):
            u = torch.randn(H, dk, generator=g)
            u = (u / u.norm(dim=-1, keepdim=True)).reshape(1, 1, E)
            a = LONG_RAMP * dk ** 0.25
            j = torch.arange(T, dtype=torch.float32)
            ramp = (j if family == "rising" else T - 1 - j) / T
            qkv[..., :E] += a * u
            qkv[..., E:2 * E] += a * ramp.view(1, T, 1) * u
        smax, tiles, last = score_stats(qkv, H)
        if family == "randn" or family_ok(family, T, smax, tiles, last):
            break
    else:
        raise AssertionError(f"no seed of 16 meets the conditions of {family}: {smax} {tiles} {last}")
    valid = ids != pad_id
    m = mul(attn_keep(B, H, T, rate, SEED, STEP, stride=512), rate)
    exact = dict(out=mha_fwd(qkv, valid, H, m, causal), dqkv=mha_bwd(qkv, valid, dout, H, m, causal),
                 lse=mha_lse(qkv, valid, H, causal))
    return SimpleNamespace(B=B, T=T, E=E, H=H, rate=rate, pattern=pattern, causal=causal,
                           family=family, pad_id=pad_id, qkv=qkv, dout=dout, ids=ids, valid=valid,
                           m=m, seed=SEED, step=STEP, smax=smax, tiles=tiles, last=last, walk=walk,
                           exact=exact)


@functools.lru_cache(maxsize=None)
def ln_case(M, n, family, rate=None):
    """LayerNorm (rate None) or sequence-prologue case. Cached: read-only."""
    g = torch.Generator().manual_seed(100 * n + M + LN_FAMILIES.index(family))
    x = torch.randn(M, n, generator=g)
    gamma, beta = torch.randn(n, generator=g), torch.randn(n, generator=g)
    pos = torch.randn(n, generator=g) if rate is not None else torch.zeros(n)
    if family == "mean100":
        x = x + 100.0
    elif family == "const":
        # x + pos == LN_CONST exactly on the last row: pos in multiples of 2^-8
        pos = torch.round(pos * 4) * LN_CONST if rate is not None else pos
        x[M - 1] = LN_CONST - pos
        gamma[::3] = 0.0
    gout = torch.randn(M, n, generator=g)
    m = mul(prologue_keep(M, n, rate or 0.0, SEED, STEP), rate or 0.0)
    y, mean, rstd = seq_prologue_fwd(x, pos, gamma, beta, m)
    dx, dg, db, dpos = seq_prologue_bwd(x, pos, gout, gamma, mean, rstd, m)
    exact = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dg, dbeta=db)
    if rate is not None:
        exact["dpos"] = dpos
    return SimpleNamespace(M=M, n=n, family=family, rate=rate, x=x, pos=pos, gamma=gamma, beta=beta,
                           g=gout, m=m, seed=SEED, step=STEP, exact=exact)


KINDS = {"rstd": "elem"}


def mean_err(got, mean, rstd):
    """max over rows of |got - mean| / max(|mean|, std), std = 1 / rstd.
    A row mean is a sum with cancellation: accumulated in fp32 it errs by
    eps * max|x|, however close to 0 it lands, so |mean| alone is no scale for
    it (the fp32 reference's mean is rounded once, an fp32-accumulating
    kernel's cannot be). What the mean is for is y = (x - mean) * rstd, which
    an error d moves by d * rstd: the error is measured in standard deviations
    of its row, or against the mean itself where that is larger."""
    g, m = got.detach().cpu().to(F64).reshape(-1), mean.reshape(-1)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    return float(((g - m).abs() / torch.maximum(m.abs(), 1.0 / rstd.reshape(-1))).max())


LSE_UNIFORM = -5e8       # the tiled backward takes a row with lse below this for uniform
LSE_UNIFORM_TOL = 32.0   # half an f32 ulp at 1e9


def lse_err(got, exact):
    """max |got - exact| / max(1, |exact|) over the rows that see a valid key.
    The rows whose visible keys are all PAD (exact = -1e9 + log n) are left to
    check_uniform_lse: through row_err(kind="elem") their 1e-3 * 1e9 would be
    every ordinary row's denominator."""
    g, e = got.detach().cpu().to(F64).reshape(-1), exact.reshape(-1)
    assert g.shape == e.shape, (g.shape, e.shape)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    rows = e >= LSE_UNIFORM
    if not bool(rows.any()):
        return 0.0
    return float(((g - e).abs() / e.abs().clamp_min(1.0))[rows].max())


def check_uniform_lse(got, exact, what="lse"):
    """rows whose visible keys are all PAD: below the backward's threshold and
    within half an f32 ulp of the exact -1e9 + log n"""
    g, e = got.detach().cpu().to(F64).reshape(-1), exact.reshape(-1)
    rows = e < LSE_UNIFORM
    bad = rows & ~((g < LSE_UNIFORM) & ((g - e).abs() <= LSE_UNIFORM_TOL))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(rows.sum())} uniform rows off"


def errs(got, exact):
    """{name: row_err} over the tensors of ``exact`` present in ``got``"""
    out = {k: row_err(got[k], e, KINDS.get(k)) for k, e in exact.items()
           if k in got and k != "lse"}
    if "mean" in out:
        out["mean"] = mean_err(got["mean"], exact["mean"], exact["rstd"])
    if "lse" in exact and "lse" in got:
        out["lse"] = lse_err(got["lse"], exact["lse"])
    return out


# --------------------------------------------- the fp32 reference's own error
def ref_run(case):
    """ops.reference in float32 on the CPU on ``case`` -> {name: tensor}"""
    from tdfo_amd.ops import reference as ref

    c = case
    if hasattr(c, "params"):
        x = c.x.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in c.params]
        wqkv, bqkv, wo, bo, g1, be1 = ps[:6]
        # the saved intermediates, by the reference's own ops
        h1 = torch.nn.functional.layer_norm(x, (c.E,), g1, be1, EPS)
        qkv = h1 @ wqkv.t() + bqkv
        ctx = ref.attention_core(qkv, c.ids, c.H, c.rate, c.seed, c.step, c.pad_id)
        x1 = x + (ctx @ wo.t() + bo) * ref.enc_site_mul(c.B, c.T, c.E, c.rate, c.seed, c.step,
                                                        ref.ENC_SITE_A, "cpu")
        h2 = torch.nn.functional.layer_norm(x1, (c.E,), ps[6], ps[7], EPS)
        f = torch.relu(h2 @ ps[8].t() + ps[9])
        y = ref.encoder_layer(x, c.ids, ps, c.H, c.rate, c.seed, c.step, c.pad_id, EPS)
        gr = torch.autograd.grad(y, [x] + ps, c.dy)
        out = dict(y=y, qkv=qkv, ctx=ctx, x1=x1, f=f, dx=gr[0])
        out.update({"d" + n: t for n, t in zip(PARAM_NAMES, gr[1:])})
        return {k: v.detach() for k, v in out.items()}
    if hasattr(c, "qkv"):
        out, dqkv = torch.empty(c.B, c.T, c.E), torch.empty_like(c.qkv)
        step, pad = torch.tensor([c.step]), getattr(c, "pad_id", 0)
        ref.attention_fwd(c.qkv, c.ids, c.H, c.rate, c.seed, step, pad, out, causal=c.causal)
        ref.attention_bwd(c.qkv, c.ids, c.dout, c.H, c.rate, c.seed, step, pad, dqkv,
                          causal=c.causal)
        if "lse" not in c.exact:
            return dict(out=out, dqkv=dqkv)
        # fp32 log-sum-exp of the reference's own score maths (attention_core)
        dk = c.E // c.H
        q, k, _ = c.qkv.view(c.B, c.T, 3, c.H, dk).permute(2, 0, 3, 1, 4)
        s = (q / math.sqrt(dk)) @ k.transpose(-2, -1)
        s = s.masked_fill(~(c.ids != pad).view(c.B, 1, 1, c.T), -1e9)
        if c.causal:
            s = s.masked_fill(torch.ones(c.T, c.T, dtype=torch.bool).triu(1), float("-inf"))
        return dict(out=out, dqkv=dqkv, lse=torch.logsumexp(s, -1))
    M, n = c.M, c.n
    y, mean, rstd, dx = torch.empty(M, n), torch.empty(M), torch.empty(M), torch.empty(M, n)
    if c.rate is None:
        dgb = torch.empty(2 * n)
        ref.layernorm_fwd(c.x, n, EPS, c.gamma, c.beta, y, mean, rstd)
        ref.layernorm_bwd(c.x, c.g, n, c.gamma, mean, rstd, dx, dgb)
        return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgb[:n], dbeta=dgb[n:])
    out3, step = torch.empty(3 * n), torch.tensor([c.step])
    ref.seq_prologue_fwd(c.x, c.pos, n, EPS, c.gamma, c.beta, c.rate, c.seed, step, y, mean, rstd)
    ref.seq_prologue_bwd(c.x, c.pos, c.g, n, c.gamma, mean, rstd, c.rate, c.seed, step, dx, out3)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=out3[:n], dbeta=out3[n:2 * n],
                dpos=out3[2 * n:])


_REF_ERR = {}


def ref_err(case):
    """{name: row_err of the fp32 reference against the oracle}: the yardstick
    of the GPU bound, computed on the CPU and stored with the case."""
    if id(case) not in _REF_ERR:
        _REF_ERR[id(case)] = (case, errs(ref_run(case), case.exact))
    return _REF_ERR[id(case)][1]


def assert_within(got, case, tag):
    """print kernel error, reference error and their ratio per tensor, then
    assert row_err(kernel) <= bound(row_err(reference)) for every one"""
    ke, re_ = errs(got, case.exact), ref_err(case)
    assert set(ke) == set(case.exact), sorted(set(case.exact) - set(ke))
    bad = []
    for k, v in ke.items():
        ratio = v / re_[k] if re_[k] > 0 else (math.inf if v > 0 else 0.0)
        print(f"{tag} {k}: kernel={v:.3e} ref={re_[k]:.3e} ratio={ratio:.2f}")
        if not v <= bound(re_[k]):
            bad.append((k, v, re_[k]))
    assert not bad, (tag, bad)
    if "lse" in case.exact:
        check_uniform_lse(got["lse"], case.exact["lse"], tag + " lse")

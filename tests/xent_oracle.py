"""float64 oracle of Linear(E -> V) + label-smoothed cross-entropy and the
shared cases of its kernel tests: the wide-hidden kernels (WIDTHS, E = 128 /
256) and the narrow ones (NARROW_WIDTHS, E = 16 / 32 / 64) run the same CASES,
built per width by ``make_case`` / ``oracle_case``.

The oracle materialises the [N, V] logits in fp64, so shapes stay small. It
is written out by hand (no autograd) to be independent of
``ops.reference.linear_xent``:
    z = H W^T + b,  lse_n = logsumexp_v z_nv,
    loss_n = lse_n - (1 - eps) z_{n, y_n} - eps * mean_v z_nv   (0 if ignored)
    dz = (softmax(z) - eps / V - (1 - eps) onehot(y)) / n_valid (0 if ignored)
    dH = dz W,  dW = dz^T H,  db = sum_n dz,  mean = sum_n loss_n / n_valid
"""
import functools

import torch

EPS = 0.1
IGNORE = 0
BOUND = 2e-4          # against the fp64 oracle, every output
NAMES = ("dH", "loss", "dW", "db")

# (V, N, hs): hs scales H (large logits exercise the running-max rescale)
CASES = [(50, 7, 1.0), (130, 65, 1.0), (1000, 320, 1.0), (4099, 1030, 1.0), (5003, 200, 4.0),
         (5003, 200, 12.0), (70001, 320, 1.0)]
WIDTHS = (128, 256)             # linear_xent_mfma.hip
NARROW_WIDTHS = (16, 32, 64)    # linear_xent.hip (16), linear_xent_wide.hip (32 / 64)
# further shapes of the split test
SPLIT_CASES = [(4099, 320), (130, 65)]


def rel_err(a: torch.Tensor, r: torch.Tensor) -> float:
    """max|a - r| / (max|r| + 1e-12), the metric of tests/test_gpu_bert4rec.py"""
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    return float((a - r).abs().max() / (r.abs().max() + 1e-12))


@functools.lru_cache(maxsize=None)
def make_case(V: int, N: int, hs: float, E: int):
    """CPU fp32 inputs (H, W, b, y); about 60 % of the labels ignored, one
    label at V - 1 and one at 1, and at (4099, 1030) labels on the first and
    last row of an interior 64-row W tile. Cached: treat as read-only."""
    g = torch.Generator().manual_seed(1000 * E + N + V)
    H = torch.randn(N, E, generator=g) * hs
    W = torch.randn(V, E, generator=g) * 0.2
    b = torch.randn(V, generator=g) * 0.1
    y = torch.randint(1, V, (N,), generator=g)
    y[torch.rand(N, generator=g) < 0.6] = IGNORE
    y[0], y[N - 1] = V - 1, 1
    if (V, N) == (4099, 1030):
        y[3], y[700] = 2048, 2048 + 63
    return H, W, b, y


def oracle(H, W, b, y, eps=EPS, ignore=IGNORE):
    """-> (dH, lossv, dW, db, mean loss), float64"""
    H, W, b = H.double(), W.double(), b.double()
    V = W.shape[0]
    valid = y != ignore
    nv = max(1, int(valid.sum()))
    z = H @ W.t() + b
    lse = torch.logsumexp(z, 1)
    zy = z.gather(1, y.view(-1, 1)).view(-1)
    lossv = torch.where(valid, lse - (1 - eps) * zy - eps * z.mean(1), torch.zeros_like(lse))
    dz = torch.exp(z - lse[:, None]) - eps / V
    dz[torch.arange(len(y)), y] -= 1 - eps
    dz = dz * valid[:, None] / nv
    return dz @ W, lossv, dz.t() @ H, dz.sum(0), lossv.sum() / nv


@functools.lru_cache(maxsize=None)
def oracle_case(V: int, N: int, hs: float, E: int):
    """Cached: treat as read-only."""
    return oracle(*make_case(V, N, hs, E))

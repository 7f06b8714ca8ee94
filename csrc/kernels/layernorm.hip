// LayerNorm over the last n elements of each row, forward and backward
// (K13/K16 in SURVEY.md §2.3). Bert4Rec uses it twice: over E = 16 per token
// inside every pre-norm sublayer (torchrec/models.py:91-106) and jointly over
// [T, E] = 320 elements after the positional encoding (models.py:147, quirk
// Q10). One wave per row; lane l owns elements l, l+64, ... (NPL per lane) so
// the row statistics are two wave reductions. fp32 throughout.
//   fwd : y = (x - mean) * rstd * gamma + beta; saves mean, rstd per row
//   bwd : dx = rstd * (g' - mean(g') - xhat * mean(g' * xhat)), g' = g * gamma
//         dgamma / dbeta: per-block partials [block][2n] (fixed row order),
//         summed by reduce_rows -> deterministic
// Sequence prologue (PRO = true): the Bert4Rec input block
//   y = dropout(LN(x + pos))   (torchrec/models.py:147-150: item embedding +
// positional encoding, LayerNorm over [T, E], embedding dropout) in one pass;
// the dropout mask is the counter hash of encoder.hip (nothing stored, the
// backward regenerates it) and the backward also emits d_pos = sum over rows
// of dx as a third partial column block [block][3n].
#include "tdfo_common.h"
#include "tdfo_kernels.h"

namespace tdfo {
namespace {

constexpr int LN_WAVES = 4;

// Optional prologue inputs of the PRO kernels.
struct ProArgs {
  const float* pos;        // [n] added to every row
  float rate;              // dropout rate on the output (0: none)
  uint32_t seed;
  const int64_t* step;     // device step counter mixed into the seed
};

__device__ __forceinline__ uint32_t pro_hash3(uint32_t a, uint32_t b, uint32_t c) {
  // the counter hash of encoder.hip / attention.hip
  uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u ^ (c + 0x165667B1u) * 0xC2B2AE3Du;
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

__device__ __forceinline__ float pro_mul(const ProArgs& p, uint32_t sd, int64_t r, int e) {
  if (p.rate <= 0.f) return 1.f;
  const uint32_t h = pro_hash3(sd, (uint32_t)r, (uint32_t)e);
  return (float)(h >> 8) * (1.0f / 16777216.0f) >= p.rate ? 1.f / (1.f - p.rate) : 0.f;
}

__device__ __forceinline__ uint32_t pro_seed(const ProArgs& p) {
  const uint32_t step = p.step ? (uint32_t)p.step[0] : 0u;
  return p.seed ^ (step * 0x632BE5ABu) ^ 0x51ED270Bu;
}

template <int NPL, bool PRO>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, int64_t M,
                                                     int n, float eps,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ beta,
                                                     float* __restrict__ y,
                                                     float* __restrict__ mean,
                                                     float* __restrict__ rstd, ProArgs pa) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const float invn = 1.f / (float)n;
  const uint32_t sd = PRO ? pro_seed(pa) : 0u;
  for (int64_t r = wave; r < M; r += nw) {
    const float* xr = x + r * n;
    float v[NPL];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int e = lane + 64 * k;
      v[k] = e < n ? xr[e] + (PRO ? pa.pos[e] : 0.f) : 0.f;
      s += v[k];
    }
    const float mu = wave_sum(s) * invn;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int e = lane + 64 * k;
      const float d = e < n ? v[k] - mu : 0.f;
      q += d * d;
    }
    const float rs = rsqrtf(wave_sum(q) * invn + eps);
    float* yr = y + r * n;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int e = lane + 64 * k;
      if (e < n) {
        const float o = (v[k] - mu) * rs * gamma[e] + beta[e];
        yr[e] = PRO ? o * pro_mul(pa, sd, r, e) : o;
      }
    }
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
  }
}

template <int NPL, bool PRO>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x,
                                                     const float* __restrict__ g, int64_t M,
                                                     int n, const float* __restrict__ gamma,
                                                     const float* __restrict__ mean,
                                                     const float* __restrict__ rstd,
                                                     float* __restrict__ dx,
                                                     float* __restrict__ part, ProArgs pa,
                                                     int nb, EncRedJob job) {
  constexpr int NP = PRO ? 3 : 2;                  // partial blocks: dgamma | dbeta (| dpos)
  __shared__ float red[LN_WAVES][NP * NPL * 64];
  if ((int)blockIdx.x >= nb) {   // a parked encoder reduction's extra blocks (no barrier)
    enc_red_col(job, ((int)blockIdx.x - nb) * (int)blockDim.x + (int)threadIdx.x);
    return;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)nb * blockDim.x) >> 6;
  const float invn = 1.f / (float)n;
  const uint32_t sd = PRO ? pro_seed(pa) : 0u;
  float dg[NPL], db[NPL], dp[NPL];
#pragma unroll
  for (int k = 0; k < NPL; ++k) { dg[k] = 0.f; db[k] = 0.f; dp[k] = 0.f; }
  for (int64_t r = wave; r < M; r += nw) {
    const float mu = mean[r], rs = rstd[r];
    float xh[NPL], gg[NPL];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int e = lane + 64 * k;
      const bool ok = e < n;
      float gv = ok ? g[r * n + e] : 0.f;
      if (PRO && ok) gv *= pro_mul(pa, sd, r, e);
      xh[k] = ok ? (x[r * n + e] + (PRO ? pa.pos[e] : 0.f) - mu) * rs : 0.f;
      gg[k] = ok ? gv * gamma[e] : 0.f;
      s1 += gg[k];
      s2 += gg[k] * xh[k];
      dg[k] += gv * xh[k];
      db[k] += gv;
    }
    const float m1 = wave_sum(s1) * invn, m2 = wave_sum(s2) * invn;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int e = lane + 64 * k;
      if (e < n) {
        const float d = rs * (gg[k] - m1 - xh[k] * m2);
        dx[r * n + e] = d;
        if (PRO) dp[k] += d;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    red[w][k * 64 + lane] = dg[k];
    red[w][NPL * 64 + k * 64 + lane] = db[k];
    if (PRO) red[w][2 * NPL * 64 + k * 64 + lane] = dp[k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < NP * n; e += blockDim.x) {
    const int blk = e / n, c = e - blk * n;
    const int idx = blk * NPL * 64 + c;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < LN_WAVES; ++q) s += red[q][idx];
    part[(int64_t)blockIdx.x * NP * n + e] = s;
  }
}

// ---- wide rows, 1024 < n <= 32768 (Bert4Rec's joint [T, E] LayerNorm at the
// published shapes: n = 3200 at max_len 50, 12800 at 200). There are only
// M = batch rows, so one workgroup owns a row; the row is re-read from L1/L2
// (<= 128 KiB) instead of held in registers. Statistics are block reductions
// in a fixed order. The parameter gradients come from a column-parallel pass
// (one thread per element, rows in ascending order: deterministic) instead of
// the [blocks][3n] partial buffer + reduce_rows of the narrow path, which
// would be tens of MB here; `part` is unused.
constexpr int LNW_THREADS = 64 * LN_WAVES;
constexpr int LNW_CHUNK = 32;               // rows per partial sum of the column pass

// sum over the workgroup, the same value in every thread: wave sums, then the
// waves in order
__device__ __forceinline__ float lnw_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                  // red may still be read
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < LN_WAVES; ++q) s += red[q];
  return s;
}

template <bool PRO>
__global__ __launch_bounds__(LNW_THREADS) void ln_wide_fwd_kernel(
    const float* __restrict__ x, int n, float eps, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ mean,
    float* __restrict__ rstd, ProArgs pa) {
  __shared__ float red[LN_WAVES];
  const int64_t r = blockIdx.x;
  const float* xr = x + r * n;
  const float invn = 1.f / (float)n;
  const uint32_t sd = PRO ? pro_seed(pa) : 0u;
  float s = 0.f;
  for (int e = threadIdx.x; e < n; e += LNW_THREADS) s += xr[e] + (PRO ? pa.pos[e] : 0.f);
  const float mu = lnw_block_sum(s, red) * invn;
  float q = 0.f;
  for (int e = threadIdx.x; e < n; e += LNW_THREADS) {
    const float d = xr[e] + (PRO ? pa.pos[e] : 0.f) - mu;
    q += d * d;
  }
  const float rs = rsqrtf(lnw_block_sum(q, red) * invn + eps);
  float* yr = y + r * n;
  for (int e = threadIdx.x; e < n; e += LNW_THREADS) {
    const float v = xr[e] + (PRO ? pa.pos[e] : 0.f);
    const float o = (v - mu) * rs * gamma[e] + beta[e];
    yr[e] = PRO ? o * pro_mul(pa, sd, r, e) : o;
  }
  if (threadIdx.x == 0) { mean[r] = mu; rstd[r] = rs; }
}

// dx of one row per workgroup
template <bool PRO>
__global__ __launch_bounds__(LNW_THREADS) void ln_wide_dx_kernel(
    const float* __restrict__ x, const float* __restrict__ g, int n,
    const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ dx, ProArgs pa) {
  __shared__ float red[LN_WAVES];
  const int64_t r = blockIdx.x;
  const float* xr = x + r * n;
  const float* gr = g + r * n;
  const float invn = 1.f / (float)n, mu = mean[r], rs = rstd[r];
  const uint32_t sd = PRO ? pro_seed(pa) : 0u;
  float s1 = 0.f, s2 = 0.f;
  for (int e = threadIdx.x; e < n; e += LNW_THREADS) {
    const float gv = PRO ? gr[e] * pro_mul(pa, sd, r, e) : gr[e];
    const float xh = (xr[e] + (PRO ? pa.pos[e] : 0.f) - mu) * rs;
    const float gg = gv * gamma[e];
    s1 += gg;
    s2 += gg * xh;
  }
  const float m1 = lnw_block_sum(s1, red) * invn;
  const float m2 = lnw_block_sum(s2, red) * invn;
  float* dr = dx + r * n;
  for (int e = threadIdx.x; e < n; e += LNW_THREADS) {
    const float gv = PRO ? gr[e] * pro_mul(pa, sd, r, e) : gr[e];
    const float xh = (xr[e] + (PRO ? pa.pos[e] : 0.f) - mu) * rs;
    dr[e] = rs * (gv * gamma[e] - m1 - xh * m2);
  }
}

// out[e] = dgamma, out[n + e] = dbeta (, out[2n + e] = dpos = sum of dx over the
// rows): thread e walks the M rows in order, coalesced across e. idx: the
// write-through into a flat gradient buffer, as reduce_rows(..., idx) (the
// value overwrites). Blocks >= nb run a parked encoder reduction's columns.
template <bool PRO>
__global__ __launch_bounds__(LNW_THREADS) void ln_wide_col_kernel(
    const float* __restrict__ x, const float* __restrict__ g, int64_t M, int n,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ dx, float* __restrict__ out, const int64_t* __restrict__ idx,
    ProArgs pa, int nb, EncRedJob job) {
  if ((int)blockIdx.x >= nb) {
    enc_red_col(job, ((int)blockIdx.x - nb) * (int)blockDim.x + (int)threadIdx.x);
    return;
  }
  const int e = (int)blockIdx.x * LNW_THREADS + (int)threadIdx.x;
  if (e >= n) return;
  const uint32_t sd = PRO ? pro_seed(pa) : 0u;
  const float pe = PRO ? pa.pos[e] : 0.f;
  // Rows in ascending order, in chunks of LNW_CHUNK whose sums are then added
  // up: one chain over M = 1030 rows carried 1030 roundings at the running
  // total's size (dbeta 11.5 x the reference's error); chunked, each of the
  // two levels carries 32. M <= LNW_CHUNK is the single chain it was.
  float dg = 0.f, db = 0.f, dp = 0.f;
  for (int64_t r0 = 0; r0 < M; r0 += LNW_CHUNK) {
    const int64_t r1 = r0 + LNW_CHUNK < M ? r0 + LNW_CHUNK : M;
    float cg = 0.f, cb = 0.f, cp = 0.f;
#pragma unroll 4
    for (int64_t r = r0; r < r1; ++r) {
      const float gv = PRO ? g[r * n + e] * pro_mul(pa, sd, r, e) : g[r * n + e];
      const float xh = (x[r * n + e] + pe - mean[r]) * rstd[r];
      cg += gv * xh;
      cb += gv;
      if (PRO) cp += dx[r * n + e];
    }
    dg += cg;
    db += cb;
    dp += cp;
  }
  out[idx ? idx[e] : e] = dg;
  out[idx ? idx[n + e] : n + e] = db;
  if (PRO) out[idx ? idx[2 * n + e] : 2 * n + e] = dp;
}

void ln_check_wide(int n) {
  if (n > LN_WIDE_MAXN) throw std::runtime_error("layernorm: n > 32768");
}

}  // namespace

int layernorm_parts(int64_t M) {
  const int64_t b = (M + LN_WAVES - 1) / LN_WAVES;
  return (int)(b < 256 ? (b < 1 ? 1 : b) : 256);
}

#define TDFO_LN_DISPATCH(KERNEL, PRO, ...)                                          \
  {                                                                                 \
    const int npl = (n + 63) / 64;                                                  \
    if (npl <= 1) hipLaunchKernelGGL((KERNEL<1, PRO>), __VA_ARGS__);                \
    else if (npl <= 2) hipLaunchKernelGGL((KERNEL<2, PRO>), __VA_ARGS__);           \
    else if (npl <= 4) hipLaunchKernelGGL((KERNEL<4, PRO>), __VA_ARGS__);           \
    else if (npl <= 8) hipLaunchKernelGGL((KERNEL<8, PRO>), __VA_ARGS__);           \
    else if (npl <= 16) hipLaunchKernelGGL((KERNEL<16, PRO>), __VA_ARGS__);         \
    else throw std::runtime_error("layernorm: n > 1024");                           \
  }

void layernorm_fwd(const float* x, int64_t M, int n, float eps, const float* gamma,
                   const float* beta, float* y, float* mean, float* rstd, hipStream_t s) {
  if (M <= 0) return;
  if (n > LN_NARROW_MAXN) {
    ln_check_wide(n);
    hipLaunchKernelGGL((ln_wide_fwd_kernel<false>), dim3((unsigned)M), dim3(LNW_THREADS), 0, s, x,
                       n, eps, gamma, beta, y, mean, rstd, ProArgs{});
    TDFO_CHECK_HIP(hipGetLastError());
    return;
  }
  const dim3 grid(layernorm_parts(M)), block(64 * LN_WAVES);
  TDFO_LN_DISPATCH(ln_fwd_kernel, false, grid, block, 0, s, x, M, n, eps, gamma, beta, y, mean,
                   rstd, ProArgs{});
  TDFO_CHECK_HIP(hipGetLastError());
}

void layernorm_bwd(const float* x, const float* g, int64_t M, int n, const float* gamma,
                   const float* mean, const float* rstd, float* dx, float* part,
                   float* dgamma_dbeta, hipStream_t s) {
  if (M <= 0) return;
  if (n > LN_NARROW_MAXN) {
    ln_check_wide(n);
    const int cb = (n + LNW_THREADS - 1) / LNW_THREADS;
    hipLaunchKernelGGL((ln_wide_dx_kernel<false>), dim3((unsigned)M), dim3(LNW_THREADS), 0, s, x,
                       g, n, gamma, mean, rstd, dx, ProArgs{});
    hipLaunchKernelGGL((ln_wide_col_kernel<false>), dim3(cb), dim3(LNW_THREADS), 0, s, x, g, M, n,
                       mean, rstd, dx, dgamma_dbeta, (const int64_t*)nullptr, ProArgs{}, cb,
                       EncRedJob{});
    TDFO_CHECK_HIP(hipGetLastError());
    return;
  }
  const int nb = layernorm_parts(M);
  const dim3 grid(nb), block(64 * LN_WAVES);
  TDFO_LN_DISPATCH(ln_bwd_kernel, false, grid, block, 0, s, x, g, M, n, gamma, mean, rstd, dx,
                   part, ProArgs{}, nb, EncRedJob{});
  TDFO_CHECK_HIP(hipGetLastError());
  reduce_rows(part, nb, 2 * n, 2 * n, dgamma_dbeta, 0, 1.f, s);
}

void seq_prologue_fwd(const float* x, const float* pos, int64_t M, int n, float eps,
                      const float* gamma, const float* beta, float rate, uint32_t seed,
                      const int64_t* step, float* y, float* mean, float* rstd, hipStream_t s) {
  if (M <= 0) return;
  const ProArgs pa{pos, rate, seed, step};
  if (n > LN_NARROW_MAXN) {
    ln_check_wide(n);
    hipLaunchKernelGGL((ln_wide_fwd_kernel<true>), dim3((unsigned)M), dim3(LNW_THREADS), 0, s, x,
                       n, eps, gamma, beta, y, mean, rstd, pa);
    TDFO_CHECK_HIP(hipGetLastError());
    return;
  }
  const dim3 grid(layernorm_parts(M)), block(64 * LN_WAVES);
  TDFO_LN_DISPATCH(ln_fwd_kernel, true, grid, block, 0, s, x, M, n, eps, gamma, beta, y, mean,
                   rstd, pa);
  TDFO_CHECK_HIP(hipGetLastError());
}

void seq_prologue_bwd(const float* x, const float* pos, const float* g, int64_t M, int n,
                      const float* gamma, const float* mean, const float* rstd, float rate,
                      uint32_t seed, const int64_t* step, float* dx, float* part,
                      float* dgamma_dbeta_dpos, hipStream_t s, const int64_t* idx) {
  if (M <= 0) return;
  const ProArgs pa{pos, rate, seed, step};
  if (n > LN_NARROW_MAXN) {
    ln_check_wide(n);
    // A parked encoder reduction is taken here exactly as on the narrow path
    // (extra blocks of the column pass). The fused block does not fit its LDS
    // budget at these row widths today, so nothing is normally parked, but the
    // job must not be dropped if that ever changes.
    EncRedJob job;
    const int extra = encoder_reduce_take(&job) ? (job.P + LNW_THREADS - 1) / LNW_THREADS : 0;
    const int cb = (n + LNW_THREADS - 1) / LNW_THREADS;
    hipLaunchKernelGGL((ln_wide_dx_kernel<true>), dim3((unsigned)M), dim3(LNW_THREADS), 0, s, x, g,
                       n, gamma, mean, rstd, dx, pa);
    hipLaunchKernelGGL((ln_wide_col_kernel<true>), dim3(cb + extra), dim3(LNW_THREADS), 0, s, x, g,
                       M, n, mean, rstd, dx, dgamma_dbeta_dpos, idx, pa, cb, job);
    TDFO_CHECK_HIP(hipGetLastError());
    return;
  }
  const int nb = layernorm_parts(M);
  // the last encoder layer's parked parameter-gradient reduction, if any,
  // rides in extra blocks of this launch
  EncRedJob job;
  const int extra = encoder_reduce_take(&job) ? (job.P + 64 * LN_WAVES - 1) / (64 * LN_WAVES) : 0;
  const dim3 grid(nb + extra), block(64 * LN_WAVES);
  TDFO_LN_DISPATCH(ln_bwd_kernel, true, grid, block, 0, s, x, g, M, n, gamma, mean, rstd, dx,
                   part, pa, nb, job);
  TDFO_CHECK_HIP(hipGetLastError());
  reduce_rows(part, nb, 3 * n, 3 * n, dgamma_dbeta_dpos, 0, 1.f, s, idx);
}
#undef TDFO_LN_DISPATCH

}  // namespace tdfo

// Fused Linear + label-smoothed cross-entropy over a gathered candidate subset
// of the output layer's rows (sampled softmax), hidden widths 16 / 32 / 64 /
// 128 / 256, and the id sampler that feeds it.
//
//   z[n, c] = H[n] . W[cand[c]] + bias[cand[c]] + corr[c]     (c a valid candidate)
//   loss_n  = lse_c z - (1 - eps) z[n, target[n]] - eps mean_c z
//   dz      = (softmax_c z - eps / Mv - (1 - eps)[c == target[n]]) / nv
// A candidate slot whose id is outside [0, V) is a hole: it is skipped and
// never dereferenced. A token whose target is outside [0, M) or names a hole is
// ignored (zero dH / lossv). Mv = valid candidates, nv = valid tokens; both stay
// on the device, so the launch sequence does not depend on them and is
// graph-capturable. dW / db rows named by a valid candidate are assigned by
// their one owner (when a token is valid); every other row is left as it was.
// No [N, M] scores in HBM,
// no float atomics, every reduction in a fixed order.
//
// The stages and the tiling are those of linear_xent_mfma.hip with the
// candidate list in the place of the vocabulary:
//   compact : block 0: valid tokens -> idx[], nv (and zeros for the ignored);
//             block 1: valid candidates -> crow[] (W row), cslot[] (slot in
//             cand), cbias[] (bias + corr), Mv, and the split geometry
//   pass1   : grid (64-token tile, candidate split s), W rows fetched through
//             crow[] into the LDS tile, the next tile's loads in flight;
//             part[token][s] = (m, sum, O = sum_c e^{z_c - m} W_c); the first
//             token tile also emits sum_c W_c and sum_c cbias_c of the split
//   merge   : one wave per valid token, splits in ascending order -> lse,
//             loss, dH
//   wgrad   : grid (64-candidate tile), valid tokens streamed in ascending
//             order; each owner stores its row at dW + crow * E
//   loss    : fixed-tree mean over the valid tokens (+ fp64 running sum)
// One workgroup = 4 waves = 64 own rows held as exact-f32 MFMA 16x16x4 B
// operands; the other side streams through LDS in tiles of ROWS x (E + 4)
// floats (the operand layout is described in linear_xent_mfma.hip).
//
// Streamed tile: ROWS = min(8192 / E, 128), i.e. 128 rows at E = 16 / 32 / 64,
// 64 at E = 128, 32 at E = 256. The uncapped 8192 / E would be 512 rows at
// E = 16 = 128 score VGPRs per lane; with the cap a lane holds at most 32 score
// registers, 64 operand and 64 accumulator registers (E = 256), the LDS tile is
// at most 34.8 KB (E = 64), and every width fits two workgroups per CU
// (__launch_bounds__(256, 2)).
//
// Splits are cut from Mv on the device (whole tiles per split, as xm_splits
// does from V, the host's capacity M only bounding the grid), so a call with
// holes and the same call with the holes removed run the same arithmetic.
#include "tdfo_xent_rows_dev.h"

namespace tdfo {
namespace {

constexpr float XR_OOR = -3.0e38f;          // rows past the split: below every real score

// block 0: tokens; block 1: candidates and the split geometry.
// want: auto (forced == 0): the host's bound on the split count; forced: the
// forced count. smax: the grid's split dimension.
template <int E>
__global__ __launch_bounds__(1024) void xr_compact_kernel(
    const int64_t* __restrict__ cand, const float* __restrict__ bias,
    const float* __restrict__ corr, const int64_t* __restrict__ target, int N, int M, int64_t V,
    int want, int forced, int32_t* __restrict__ idx, int32_t* __restrict__ crow,
    int32_t* __restrict__ cslot, float* __restrict__ cbias, int32_t* __restrict__ counts,
    float* __restrict__ dH, float* __restrict__ lossv) {
  __shared__ int wsum[16];
  __shared__ int base;
  if (blockIdx.x == 0) {
    const int nv = xr_compact(
        N, wsum, &base,
        [&](int j) {
          const int64_t y = target[j];
          bool ok = y >= 0 && y < M;
          if (ok) {
            const int64_t r = cand[y];
            ok = r >= 0 && r < V;
          }
          if (!ok) {
            lossv[j] = 0.f;
            for (int k = 0; k < E; k += 4)
              *(float4*)(dH + (int64_t)j * E + k) = make_float4(0, 0, 0, 0);
          }
          return ok;
        },
        [&](int j, int p) { idx[p] = j; });
    if (threadIdx.x == 0) counts[XR_NV] = nv;
    return;
  }
  const int mv = xr_compact(
      M, wsum, &base,
      [&](int j) {
        const int64_t r = cand[j];
        return r >= 0 && r < V;
      },
      [&](int j, int p) {
        const int64_t r = cand[j];
        crow[p] = (int)r;
        cslot[p] = j;
        cbias[p] = bias[r] + (corr ? corr[j] : 0.f);
      });
  if (threadIdx.x == 0) xr_cut_splits<E>(mv, want, forced, counts);
}

// compacted candidates [r0, r0 + ROWS) of the split ending at v1 -> registers
// (W rows gathered through crow); rows past v1 are zeros
template <int E>
__device__ __forceinline__ void xr_fetch_w(const float* __restrict__ W,
                                           const int32_t* __restrict__ crow,
                                           const float* __restrict__ cbias, int r0, int v1,
                                           XrRegs<E>& R, float& b) {
  using G = XrGeo<E>;
#pragma unroll
  for (int k = 0; k < G::NV; ++k) {
    const int e = (int)threadIdx.x + k * XR_THREADS, r = e / G::V4, c = e - r * G::V4;
    R.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < v1) R.v[k] = *(const float4*)(W + (int64_t)crow[r0 + r] * E + 4 * c);
  }
  b = 0.f;
  if ((int)threadIdx.x < G::ROWS && r0 + (int)threadIdx.x < v1) b = cbias[r0 + (int)threadIdx.x];
}

template <int E>
__global__ __launch_bounds__(XR_THREADS, 2) void xr_pass1_kernel(
    const float* __restrict__ H, const float* __restrict__ W, int S,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ crow,
    const float* __restrict__ cbias, const int32_t* __restrict__ counts,
    float* __restrict__ part, float* __restrict__ wpart) {
  using G = XrGeo<E>;
  constexpr int XP = E + 4;             // partial record: m, sum, pad, pad, O[E]
  __shared__ __attribute__((aligned(16))) float ws[G::ROWS * G::LD];
  __shared__ float bs[G::ROWS];
  const int tile = blockIdx.x, s = blockIdx.y;  // x = token tile: neighbours share W rows in L2
  const int nv = counts[XR_NV], mv = counts[XR_MV], VS = counts[XR_VS];
  if (s >= counts[XR_SV] || tile * XR_OWN >= nv) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int v0 = s * VS, v1 = min(mv, v0 + VS);
  const int j = tile * XR_OWN + 16 * w + t;            // this lane's valid token
  const bool jok = j < nv;

  float h[G::NS];
  xr_own<E>(H + (int64_t)(jok ? idx[j] : 0) * E, g, jok, h);
  f32x4_t o[G::M];
#pragma unroll
  for (int m = 0; m < G::M; ++m) o[m] = {0.f, 0.f, 0.f, 0.f};
  float mx = XR_OOR, l = 0.f;           // l: this lane's share of the token's sum
  float colsum = 0.f, bsum = 0.f;       // tile 0: thread c < E sums column c, thread 0 the bias

  XrRegs<E> wreg;
  float breg;
  xr_fetch_w<E>(W, crow, cbias, v0, v1, wreg, breg);
  for (int r0 = v0; r0 < v1; r0 += G::ROWS) {
    __syncthreads();                    // the previous tile is consumed
    xr_put<E>(wreg, ws);
    if ((int)threadIdx.x < G::ROWS) bs[threadIdx.x] = breg;
    __syncthreads();
    if (r0 + G::ROWS < v1)              // the next tile's loads fly during this one
      xr_fetch_w<E>(W, crow, cbias, r0 + G::ROWS, v1, wreg, breg);
    if (tile == 0) {                    // ascending rows: a fixed summation order
      if ((int)threadIdx.x < E)
        for (int r = 0; r < G::ROWS; ++r) colsum += ws[r * G::LD + threadIdx.x];
      if (threadIdx.x == 0)
        for (int r = 0; r < G::ROWS; ++r) bsum += bs[r];
    }
    f32x4_t x[G::NB];
#pragma unroll
    for (int n = 0; n < G::NB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[n][r] = bs[16 * n + 4 * g + r];
    xr_dot_tile<E>(ws, h, t, g, x);     // x[n][r] = z[token][candidate r0 + 16n + 4g + r]
    float tmx = XR_OOR;
#pragma unroll
    for (int n = 0; n < G::NB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = r0 + 16 * n + 4 * g + r < v1 ? x[n][r] : XR_OOR;
        x[n][r] = v;
        tmx = fmaxf(tmx, v);
      }
    const float mnew = fmaxf(mx, xr_max4(tmx));        // (every tile holds a row < v1)
    const float alpha = __expf(mx - mnew);
    mx = mnew;
    l *= alpha;
#pragma unroll
    for (int m = 0; m < G::M; ++m) o[m] *= alpha;
#pragma unroll
    for (int n = 0; n < G::NB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = r0 + 16 * n + 4 * g + r < v1 ? __expf(x[n][r] - mx) : 0.f;
        l += p;
        x[n][r] = p;
      }
    xr_acc_tile<E>(ws, x, t, g, o);     // O[token][:] += P[token][tile] . W[tile]
  }
  if (tile == 0) {
    if ((int)threadIdx.x < E) wpart[(int64_t)s * (E + 1) + threadIdx.x] = colsum;
    if (threadIdx.x == 0) wpart[(int64_t)s * (E + 1) + E] = bsum;
  }
  l = xr_sum4(l);
  if (jok) {
    float* p = part + ((int64_t)j * S + s) * XP;
    if (g == 0) { p[0] = mx; p[1] = l; }
#pragma unroll
    for (int m = 0; m < G::M; ++m)
      *(float4*)(p + 4 + 16 * m + 4 * g) = make_float4(o[m][0], o[m][1], o[m][2], o[m][3]);
  }
}

// one wave per valid token; lane k owns hidden dims k, k + 64, ... (< E)
template <int E>
__global__ __launch_bounds__(64) void xr_merge_kernel(
    const float* __restrict__ H, const float* __restrict__ W, const float* __restrict__ bias,
    const float* __restrict__ corr, const int64_t* __restrict__ cand,
    const int64_t* __restrict__ target, int S, float eps, const int32_t* __restrict__ idx,
    const int32_t* __restrict__ counts, const float* __restrict__ part,
    const float* __restrict__ wpart, float* __restrict__ lse_out, float* __restrict__ dH,
    float* __restrict__ lossv) {
  constexpr int XP = E + 4, Q = XrGeo<E>::Q;
  const int lane = threadIdx.x, j = blockIdx.x;
  const int nv = counts[XR_NV], mv = counts[XR_MV], sv = counts[XR_SV];
  if (j >= nv) return;                  // (nv > 0 implies mv > 0: a valid target names a candidate)
  const float scale = 1.f / (float)max(1, nv);
  const float* p0 = part + (int64_t)j * S * XP;
  float mx = -INFINITY;
  for (int s = lane; s < sv; s += 64) mx = fmaxf(mx, p0[(int64_t)s * XP]);
  mx = wave_max(mx);
  float sum = 0.f, wsb = 0.f, acc[Q], ws[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) { acc[q] = 0.f; ws[q] = 0.f; }
  for (int s = 0; s < sv; ++s) {        // split order: deterministic
    const float* p = p0 + (int64_t)s * XP;
    const float c = __expf(p[0] - mx);
    sum += c * p[1];
    wsb += wpart[(int64_t)s * (E + 1) + E];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int k = lane + 64 * q;
      if (k < E) {
        acc[q] += c * p[4 + k];
        ws[q] += wpart[(int64_t)s * (E + 1) + k];
      }
    }
  }
  const int n = idx[j];
  const int64_t slot = target[n];       // valid by the compaction: in [0, M), not a hole
  const int64_t y = cand[slot];
  float wy[Q], dzy = 0.f, dzm = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int k = lane + 64 * q;
    wy[q] = 0.f;
    if (k < E) {
      const float hk = H[(int64_t)n * E + k];
      wy[q] = W[y * E + k];
      dzy += wy[q] * hk;
      dzm += ws[q] * hk;
    }
  }
  const float zy = bias[y] + (corr ? corr[slot] : 0.f) + wave_sum(dzy);
  const float zmean = (wsb + wave_sum(dzm)) / (float)mv;
  const float lse = mx + __logf(sum);
  if (lane == 0) {
    lse_out[j] = lse;
    lossv[n] = lse - (1.f - eps) * zy - eps * zmean;
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int k = lane + 64 * q;
    if (k < E)
      dH[(int64_t)n * E + k] =
          scale * (acc[q] / sum - (1.f - eps) * wy[q] - eps * ws[q] / (float)mv);
  }
}

// valid tokens [x0, x0 + ROWS) -> registers (H rows gathered through idx, lse,
// target slot); tokens past nv are zeros
template <int E>
__device__ __forceinline__ void xr_fetch_h(const float* __restrict__ H,
                                           const int64_t* __restrict__ target,
                                           const int32_t* __restrict__ idx,
                                           const float* __restrict__ lse, int x0, int nv,
                                           XrRegs<E>& R, float& l, int& y) {
  using G = XrGeo<E>;
#pragma unroll
  for (int k = 0; k < G::NV; ++k) {
    const int e = (int)threadIdx.x + k * XR_THREADS, r = e / G::V4, c = e - r * G::V4;
    R.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x0 + r < nv) R.v[k] = *(const float4*)(H + (int64_t)idx[x0 + r] * E + 4 * c);
  }
  l = 0.f;
  y = -1;
  const int x = x0 + (int)threadIdx.x;
  if ((int)threadIdx.x < G::ROWS && x < nv) {
    l = lse[x];
    y = (int)target[idx[x]];            // M < 2^31
  }
}

template <int E>
__global__ __launch_bounds__(XR_THREADS, 2) void xr_wgrad_kernel(
    const float* __restrict__ H, const float* __restrict__ W, const int64_t* __restrict__ target,
    float eps, const int32_t* __restrict__ idx, const int32_t* __restrict__ crow,
    const int32_t* __restrict__ cslot, const float* __restrict__ cbias,
    const int32_t* __restrict__ counts, const float* __restrict__ lse, float* __restrict__ dW,
    float* __restrict__ db) {
  using G = XrGeo<E>;
  __shared__ __attribute__((aligned(16))) float hs[G::ROWS * G::LD];
  __shared__ float ls[G::ROWS];
  __shared__ int ys[G::ROWS];
  const int nv = counts[XR_NV], mv = counts[XR_MV];
  if (nv == 0 || (int)blockIdx.x * XR_OWN >= mv) return;   // (no valid token: nothing is written)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int c = (int)blockIdx.x * XR_OWN + 16 * w + t;     // this lane's compacted candidate
  const bool vok = c < mv;
  const int64_t v = vok ? crow[c] : 0;                      // its row of W
  const int slot = vok ? cslot[c] : -2;                     // (-1 is fetch_h's "no token")
  const float scale = 1.f / (float)max(1, nv);
  const float off = eps / (float)mv, hit = 1.f - eps;

  float wr[G::NS];
  xr_own<E>(W + v * E, g, vok, wr);
  const float b = vok ? cbias[c] : 0.f;
  f32x4_t gw[G::M];
#pragma unroll
  for (int m = 0; m < G::M; ++m) gw[m] = {0.f, 0.f, 0.f, 0.f};
  float gb = 0.f;                       // this lane's share of db_v

  XrRegs<E> hreg;
  float lreg;
  int yreg;
  xr_fetch_h<E>(H, target, idx, lse, 0, nv, hreg, lreg, yreg);
  for (int x0 = 0; x0 < nv; x0 += G::ROWS) {           // ascending: a fixed summation order
    __syncthreads();
    xr_put<E>(hreg, hs);
    if ((int)threadIdx.x < G::ROWS) { ls[threadIdx.x] = lreg; ys[threadIdx.x] = yreg; }
    __syncthreads();
    if (x0 + G::ROWS < nv) xr_fetch_h<E>(H, target, idx, lse, x0 + G::ROWS, nv, hreg, lreg, yreg);
    f32x4_t z[G::NB];
#pragma unroll
    for (int n = 0; n < G::NB; ++n) z[n] = {b, b, b, b};
    xr_dot_tile<E>(hs, wr, t, g, z);    // z[n][r] = z[token x0 + 16n + 4g + r][candidate c]
#pragma unroll
    for (int n = 0; n < G::NB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int xl = 16 * n + 4 * g + r;
        float dz = __expf(z[n][r] - ls[xl]) - off;
        if (ys[xl] == slot) dz -= hit;
        dz = x0 + xl < nv ? dz * scale : 0.f;
        gb += dz;
        z[n][r] = dz;
      }
    xr_acc_tile<E>(hs, z, t, g, gw);    // dW[v][:] += dz[tile][c] . H[tile]
  }
  gb = xr_sum4(gb);
  if (!vok) return;
#pragma unroll
  for (int m = 0; m < G::M; ++m)
    *(float4*)(dW + v * E + 16 * m + 4 * g) = make_float4(gw[m][0], gw[m][1], gw[m][2], gw[m][3]);
  if (g == 0) db[v] = gb;
}

struct XrLayout {
  size_t idx, crow, cslot, counts, cbias, lse, part, wpart, total;
};

XrLayout xr_layout(int N, int M, int E, int S) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  XrLayout L;
  size_t o = 0;
  L.idx = o;    o = up(o + (size_t)N * 4);
  L.crow = o;   o = up(o + (size_t)M * 4);
  L.cslot = o;  o = up(o + (size_t)M * 4);
  L.counts = o; o = up(o + 16 * 4);
  L.cbias = o;  o = up(o + (size_t)M * 4);
  L.lse = o;    o = up(o + (size_t)N * 4);
  L.part = o;   o = up(o + (size_t)N * S * (E + 4) * 4);
  L.wpart = o;  o = up(o + (size_t)S * (E + 1) * 4);
  L.total = o + 16;                     // (the base is aligned up to 16 bytes)
  return L;
}

template <int E>
void xr_run(const LinearXentRowsArgs& a, hipStream_t s) {
  int S, want, forced;
  xr_splits(a.N, a.M, E, &S, &want, &forced);
  const XrLayout L = xr_layout(a.N, a.M, E, S);
  char* ws = (char*)(((uintptr_t)a.workspace + 15) & ~(uintptr_t)15);
  int32_t* idx = (int32_t*)(ws + L.idx);
  int32_t* crow = (int32_t*)(ws + L.crow);
  int32_t* cslot = (int32_t*)(ws + L.cslot);
  int32_t* counts = (int32_t*)(ws + L.counts);
  float* cbias = (float*)(ws + L.cbias);
  float* lse = (float*)(ws + L.lse);
  float* part = (float*)(ws + L.part);
  float* wpart = (float*)(ws + L.wpart);
  hipLaunchKernelGGL(xr_compact_kernel<E>, dim3(2), dim3(1024), 0, s, a.cand, a.bias, a.corr,
                     a.target, a.N, a.M, a.V, want, forced, idx, crow, cslot, cbias, counts, a.dH,
                     a.lossv);
  const int tiles = (a.N + XR_OWN - 1) / XR_OWN;
  hipLaunchKernelGGL(xr_pass1_kernel<E>, dim3(tiles, S), dim3(XR_THREADS), 0, s, a.H, a.W, S, idx,
                     crow, cbias, counts, part, wpart);
  hipLaunchKernelGGL(xr_merge_kernel<E>, dim3(a.N), dim3(64), 0, s, a.H, a.W, a.bias, a.corr,
                     a.cand, a.target, S, a.eps, idx, counts, part, wpart, lse, a.dH, a.lossv);
  if (a.dW)
    hipLaunchKernelGGL(xr_wgrad_kernel<E>, dim3((unsigned)((a.M + XR_OWN - 1) / XR_OWN)),
                       dim3(XR_THREADS), 0, s, a.H, a.W, a.target, a.eps, idx, crow, cslot, cbias,
                       counts, lse, a.dW, a.db);
  if (a.loss)
    hipLaunchKernelGGL(xr_loss_kernel, dim3(1), dim3(1024), 0, s, a.lossv, a.N, counts, a.loss,
                       a.loss_acc);
  TDFO_CHECK_HIP(hipGetLastError());
}

// out[i] = lo + ((hash(seed, *step mod 2^32, i) * span) >> 32)
__global__ __launch_bounds__(256) void xr_sample_kernel(uint32_t seed,
                                                        const int64_t* __restrict__ step,
                                                        int64_t lo, uint32_t span, int64_t n,
                                                        int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t h = sr_hash3(seed, (uint32_t)(uint64_t)step[0], (uint32_t)i);
  out[i] = lo + (int64_t)(((uint64_t)h * span) >> 32);
}

}  // namespace

size_t linear_xent_rows_workspace(int N, int M, int E) {
  if (N <= 0 || M <= 0) return 16;
  int S, want, forced;
  xr_splits(N, M, E, &S, &want, &forced);
  return xr_layout(N, M, E, S).total;
}

void linear_xent_rows(const LinearXentRowsArgs& a, int E, hipStream_t s) {
  if (a.N <= 0 || a.M <= 0) return;
  if (a.V <= 0 || a.V >= (int64_t(1) << 31))
    throw std::runtime_error("linear_xent_rows: vocab must be in [1, 2^31)");
  switch (E) {
    case 16: xr_run<16>(a, s); break;
    case 32: xr_run<32>(a, s); break;
    case 64: xr_run<64>(a, s); break;
    case 128: xr_run<128>(a, s); break;
    case 256: xr_run<256>(a, s); break;
    default:
      throw std::runtime_error("linear_xent_rows: hidden width must be 16, 32, 64, 128 or 256");
  }
}

void sample_ids(uint32_t seed, const int64_t* step, int64_t lo, int64_t hi, int64_t n,
                int64_t* out, hipStream_t s) {
  if (n <= 0) return;
  if (hi <= lo || hi - lo >= (int64_t(1) << 31))
    throw std::runtime_error("sample_ids: need 0 < hi - lo < 2^31");
  hipLaunchKernelGGL(xr_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, seed,
                     step, lo, (uint32_t)(hi - lo), n, out);
  TDFO_CHECK_HIP(hipGetLastError());
}

}  // namespace tdfo

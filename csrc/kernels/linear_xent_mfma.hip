// Fused output projection + label-smoothed cross-entropy for hidden widths 128
// and 256 (Bert4Rec at hidden 128 / 256). The contract, the maths and the four
// stages are those of linear_xent.hip / linear_xent_wide.hip; no [tokens, V]
// logits, no float atomics, every reduction in a fixed order:
//   compact : valid tokens (label != ignore) -> idx[], n_valid (device)
//   pass1   : grid (64-token tile, vocab split s), online softmax over the
//             split: part[token][s] = (m, sum, O = sum_v e^{z_v - m} W_v); the
//             first token tile also emits sum_v W_v, sum_v b_v of the split
//   merge   : one wave per valid token, the splits combined in ascending order
//             -> lse, loss, dH = scale * (E_p[W] - (1-eps) W_y - eps/V sum_v W_v)
//   wgrad   : grid (64-row vocab tile), tokens streamed in ascending order:
//             dz = scale * (e^{z - lse} - eps/V - (1-eps)[v == y]),
//             dW_v = sum_n dz H_n, db_v = sum_n dz, each written by its owner
//   loss    : mean over the valid tokens in a fixed tree (+ fp64 running sum)
// With a fused optimizer step the flat optimizer's kernel runs on W and bias
// right after wgrad, as linear_xent_wide.hip does.
//
// pass1 and wgrad are the tiling of attention_long.hip with E in the place of
// d_k. One workgroup = 4 waves = 64 rows of the "own" side (tokens in pass1,
// vocab rows in wgrad); wave w owns 16 of them, held as MFMA B operands in
// registers (E / 4 VGPRs per lane). The other side streams through LDS in
// tiles of 8192 / E rows x (E + 4) floats (64 rows at E = 128, 32 at E = 256:
// the tile, the staging registers and the score registers then cost the same
// at both widths, and E = 256 keeps 2 workgroups per CU), the next tile's
// global loads in flight while the current one is computed on. All products
// run on the exact-f32 MFMA 16x16x4 (lane l: t = l & 15, g = l >> 4;
// A[i=t][k=g], B[k=g][j=t], D[row 4g+r][col t] in register r):
//   X^T = stream . own^T : A = a streamed row (16n + t), B = the own row t,
//                          C = the bias; lane (t, g) then holds
//                          X[streamed row 16n+4g+r][own row t]
//   Y^T = stream^T . P   : A = column 16m + t of the streamed tile, B = P's
//                          registers as they stand; lane (t, g) ends with
//                          Y[own row t][16m+4g .. +3], one float4 of the output
// The own row sits on the lane column, so a softmax statistic is one value per
// lane, reduced over the four g-groups by two shuffles.
#include "tdfo_common.h"
#include "tdfo_kernels.h"

#include <algorithm>

namespace tdfo {
namespace {

constexpr int XM_OWN = 64;                  // own rows per workgroup (16 per wave)
constexpr int XM_THREADS = 256;
constexpr float XM_OOR = -3.0e38f;          // rows past the split: below every real score

int g_xm_splits = 0;                        // 0 auto; n > 0 forced (linear_xent_splits)

template <int E>
struct XmGeo {
  static constexpr int NS = E / 4;          // k-steps = operand floats per lane
  static constexpr int M = E / 16;          // 16-wide output column blocks
  static constexpr int LD = E + 4;          // LDS row stride (16-B aligned; 4 LD = 16 mod 32)
  static constexpr int ROWS = 8192 / E;     // streamed rows per tile
  static constexpr int NB = ROWS / 16;      // 16-row blocks per tile
  static constexpr int V4 = E / 4;          // float4s per row
  static constexpr int NV = ROWS * V4 / XM_THREADS;   // float4s per thread and tile (= 8)
};

__device__ __forceinline__ f32x4_t xm_mfma(float a, float b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float xm_max4(float v) {     // over lanes t, t+16, t+32, t+48
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}

__device__ __forceinline__ float xm_sum4(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// a lane's B operands of one E-float row: k-step 4c + s <-> element 16c + 4g + s
template <int E>
__device__ __forceinline__ void xm_own(const float* __restrict__ row, int g, bool ok,
                                       float (&f)[XmGeo<E>::NS]) {
#pragma unroll
  for (int c = 0; c < E / 16; ++c) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) v = *(const float4*)(row + 16 * c + 4 * g);
    f[4 * c] = v.x; f[4 * c + 1] = v.y; f[4 * c + 2] = v.z; f[4 * c + 3] = v.w;
  }
}

template <int E>
struct XmRegs { float4 v[XmGeo<E>::NV]; };  // this thread's float4s of one streamed tile

// acc[n][r] = c[n][r] + (streamed row 16n + 4g + r) . (own row t)
template <int E>
__device__ __forceinline__ void xm_dot_tile(const float* tile, const float (&own)[XmGeo<E>::NS],
                                            int t, int g, f32x4_t (&acc)[XmGeo<E>::NB]) {
  using G = XmGeo<E>;
#pragma unroll
  for (int n = 0; n < G::NB; ++n) {
    const float* row = tile + (16 * n + t) * G::LD + 4 * g;
    f32x4_t c = acc[n];
#pragma unroll
    for (int k = 0; k < E / 16; ++k) {
      const float4 a = *(const float4*)(row + 16 * k);
      c = xm_mfma(a.x, own[4 * k], c);
      c = xm_mfma(a.y, own[4 * k + 1], c);
      c = xm_mfma(a.z, own[4 * k + 2], c);
      c = xm_mfma(a.w, own[4 * k + 3], c);
    }
    acc[n] = c;
  }
}

// out[m][r] (column 16m + 4g + r of own row t) += sum over the streamed rows x
// of tile[x][column] * val(x, t); val is in the layout xm_dot_tile leaves
template <int E>
__device__ __forceinline__ void xm_acc_tile(const float* tile, const f32x4_t (&val)[XmGeo<E>::NB],
                                            int t, int g, f32x4_t (&out)[XmGeo<E>::M]) {
  using G = XmGeo<E>;
#pragma unroll
  for (int n = 0; n < G::NB; ++n) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* row = tile + (16 * n + 4 * g + r) * G::LD + t;
#pragma unroll
      for (int m = 0; m < G::M; ++m) out[m] = xm_mfma(row[16 * m], val[n][r], out[m]);
    }
  }
}

template <int E>
__device__ __forceinline__ void xm_put(const XmRegs<E>& R, float* tile) {
  using G = XmGeo<E>;
#pragma unroll
  for (int k = 0; k < G::NV; ++k) {
    const int e = (int)threadIdx.x + k * XM_THREADS, r = e / G::V4, c = e - r * G::V4;
    *(float4*)(tile + r * G::LD + 4 * c) = R.v[k];
  }
}

template <int E>
__global__ __launch_bounds__(1024) void xm_compact_kernel(const int64_t* __restrict__ labels,
                                                          int N, int ignore,
                                                          int32_t* __restrict__ idx,
                                                          int32_t* __restrict__ count,
                                                          float* __restrict__ dH,
                                                          float* __restrict__ lossv) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) base = 0;
  __syncthreads();
  for (int s0 = 0; s0 < N; s0 += 1024) {
    const int j = s0 + t;
    const bool v = j < N && labels[j] != ignore;
    if (j < N && !v) {
      lossv[j] = 0.f;
      for (int k = 0; k < E; k += 4) *(float4*)(dH + (int64_t)j * E + k) = make_float4(0, 0, 0, 0);
    }
    const uint64_t bal = __ballot(v);
    const int pre = __popcll(bal & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int q = 0; q < w; ++q) off += wsum[q];
    if (v) idx[off + pre] = j;
    __syncthreads();
    if (t == 0) {
      int tot = 0;
      for (int q = 0; q < 16; ++q) tot += wsum[q];
      base += tot;
    }
    __syncthreads();
  }
  if (t == 0) *count = base;
}

// W rows [v0 + r0, v0 + r0 + ROWS) of the split [v0, v1) -> registers; rows
// past v1 are zeros
template <int E>
__device__ __forceinline__ void xm_fetch_w(const float* __restrict__ W,
                                           const float* __restrict__ bias, int64_t r0, int64_t v1,
                                           XmRegs<E>& R, float& b) {
  using G = XmGeo<E>;
#pragma unroll
  for (int k = 0; k < G::NV; ++k) {
    const int e = (int)threadIdx.x + k * XM_THREADS, r = e / G::V4, c = e - r * G::V4;
    R.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < v1) R.v[k] = *(const float4*)(W + (r0 + r) * E + 4 * c);
  }
  b = 0.f;
  if ((int)threadIdx.x < G::ROWS && r0 + (int)threadIdx.x < v1) b = bias[r0 + (int)threadIdx.x];
}

template <int E>
__global__ __launch_bounds__(XM_THREADS, 2) void xm_pass1_kernel(
    const float* __restrict__ H, const float* __restrict__ W, const float* __restrict__ bias,
    int64_t V, int64_t VS, int S, const int32_t* __restrict__ idx,
    const int32_t* __restrict__ count, float* __restrict__ part, float* __restrict__ wpart) {
  using G = XmGeo<E>;
  constexpr int XP = E + 4;             // partial record: m, sum, pad, pad, O[E]
  __shared__ __attribute__((aligned(16))) float ws[G::ROWS * G::LD];
  __shared__ float bs[G::ROWS];
  const int tile = blockIdx.x, s = blockIdx.y;  // x = token tile: neighbours share W rows in L2
  const int nv = *count;
  if (tile > 0 && tile * XM_OWN >= nv) return;         // (tile 0 always sums the split's W, b)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int64_t v0 = (int64_t)s * VS, v1 = min(V, v0 + VS);
  const int j = tile * XM_OWN + 16 * w + t;            // this lane's valid token
  const bool jok = j < nv;

  float h[G::NS];
  xm_own<E>(H + (int64_t)(jok ? idx[j] : 0) * E, g, jok, h);
  f32x4_t o[G::M];
#pragma unroll
  for (int m = 0; m < G::M; ++m) o[m] = {0.f, 0.f, 0.f, 0.f};
  float mx = XM_OOR, l = 0.f;           // l: this lane's share of the token's sum
  float colsum = 0.f, bsum = 0.f;       // tile 0: thread c < E sums column c, thread 0 the bias

  XmRegs<E> wreg;
  float breg;
  xm_fetch_w<E>(W, bias, v0, v1, wreg, breg);
  for (int64_t r0 = v0; r0 < v1; r0 += G::ROWS) {
    __syncthreads();                    // the previous tile is consumed
    xm_put<E>(wreg, ws);
    if ((int)threadIdx.x < G::ROWS) bs[threadIdx.x] = breg;
    __syncthreads();
    if (r0 + G::ROWS < v1)              // the next tile's loads fly during this one
      xm_fetch_w<E>(W, bias, r0 + G::ROWS, v1, wreg, breg);
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
    xm_dot_tile<E>(ws, h, t, g, x);     // x[n][r] = z[token][r0 + 16n + 4g + r]
    float tmx = XM_OOR;
#pragma unroll
    for (int n = 0; n < G::NB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = r0 + 16 * n + 4 * g + r < v1 ? x[n][r] : XM_OOR;
        x[n][r] = v;
        tmx = fmaxf(tmx, v);
      }
    const float mnew = fmaxf(mx, xm_max4(tmx));        // (every tile holds a row < v1)
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
    xm_acc_tile<E>(ws, x, t, g, o);     // O[token][:] += P[token][tile] . W[tile]
  }
  if (tile == 0) {
    if ((int)threadIdx.x < E) wpart[(int64_t)s * (E + 1) + threadIdx.x] = colsum;
    if (threadIdx.x == 0) wpart[(int64_t)s * (E + 1) + E] = bsum;
  }
  l = xm_sum4(l);
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
__global__ __launch_bounds__(64) void xm_merge_kernel(
    const float* __restrict__ H, const float* __restrict__ W, const float* __restrict__ bias,
    const int64_t* __restrict__ labels, int64_t V, int S, float eps,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
    const float* __restrict__ part, const float* __restrict__ wpart, float* __restrict__ lse_out,
    float* __restrict__ dH, float* __restrict__ lossv) {
  constexpr int XP = E + 4, Q = E / 64;
  const int lane = threadIdx.x, j = blockIdx.x;
  const int nv = *count;
  if (j >= nv) return;
  const float scale = 1.f / (float)max(1, nv);
  const float* p0 = part + (int64_t)j * S * XP;
  float mx = -INFINITY;
  for (int s = lane; s < S; s += 64) mx = fmaxf(mx, p0[(int64_t)s * XP]);
  mx = wave_max(mx);
  float sum = 0.f, wsb = 0.f, acc[Q], ws[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) { acc[q] = 0.f; ws[q] = 0.f; }
  for (int s = 0; s < S; ++s) {         // split order: deterministic
    const float* p = p0 + (int64_t)s * XP;
    const float c = __expf(p[0] - mx);  // (an empty split cannot occur: every split holds a row)
    sum += c * p[1];
    wsb += wpart[(int64_t)s * (E + 1) + E];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      acc[q] += c * p[4 + lane + 64 * q];
      ws[q] += wpart[(int64_t)s * (E + 1) + lane + 64 * q];
    }
  }
  const int n = idx[j];
  int64_t y = labels[n];
  if (y < 0 || y >= V) y = 0;           // host validates; never read out of bounds
  float wy[Q], dzy = 0.f, dzm = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const float hk = H[(int64_t)n * E + lane + 64 * q];
    wy[q] = W[y * E + lane + 64 * q];
    dzy += wy[q] * hk;
    dzm += ws[q] * hk;
  }
  const float zy = bias[y] + wave_sum(dzy);
  const float zmean = (wsb + wave_sum(dzm)) / (float)V;
  const float lse = mx + __logf(sum);
  if (lane == 0) {
    lse_out[j] = lse;
    lossv[n] = lse - (1.f - eps) * zy - eps * zmean;
  }
#pragma unroll
  for (int q = 0; q < Q; ++q)
    dH[(int64_t)n * E + lane + 64 * q] =
        scale * (acc[q] / sum - (1.f - eps) * wy[q] - eps * ws[q] / (float)V);
}

// valid tokens [x0, x0 + ROWS) -> registers (H rows gathered through idx, lse,
// label); tokens past nv are zeros
template <int E>
__device__ __forceinline__ void xm_fetch_h(const float* __restrict__ H,
                                           const int64_t* __restrict__ labels,
                                           const int32_t* __restrict__ idx,
                                           const float* __restrict__ lse, int x0, int nv,
                                           XmRegs<E>& R, float& l, int& y) {
  using G = XmGeo<E>;
#pragma unroll
  for (int k = 0; k < G::NV; ++k) {
    const int e = (int)threadIdx.x + k * XM_THREADS, r = e / G::V4, c = e - r * G::V4;
    R.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x0 + r < nv) R.v[k] = *(const float4*)(H + (int64_t)idx[x0 + r] * E + 4 * c);
  }
  l = 0.f;
  y = -1;
  const int x = x0 + (int)threadIdx.x;
  if ((int)threadIdx.x < G::ROWS && x < nv) {
    l = lse[x];
    y = (int)labels[idx[x]];            // V < 2^31
  }
}

template <int E>
__global__ __launch_bounds__(XM_THREADS, 2) void xm_wgrad_kernel(
    const float* __restrict__ H, const float* __restrict__ W, const float* __restrict__ bias,
    const int64_t* __restrict__ labels, int64_t V, float eps, const int32_t* __restrict__ idx,
    const int32_t* __restrict__ count, const float* __restrict__ lse, float* __restrict__ dW,
    float* __restrict__ db) {
  using G = XmGeo<E>;
  __shared__ __attribute__((aligned(16))) float hs[G::ROWS * G::LD];
  __shared__ float ls[G::ROWS];
  __shared__ int ys[G::ROWS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int64_t v = (int64_t)blockIdx.x * XM_OWN + 16 * w + t;     // this lane's vocab row
  const bool vok = v < V;
  const int nv = *count;
  const float scale = 1.f / (float)max(1, nv);
  const float off = eps / (float)V, hit = 1.f - eps;

  float wr[G::NS];
  xm_own<E>(W + (vok ? v : 0) * E, g, vok, wr);
  const float b = vok ? bias[v] : 0.f;
  f32x4_t gw[G::M];
#pragma unroll
  for (int m = 0; m < G::M; ++m) gw[m] = {0.f, 0.f, 0.f, 0.f};
  float gb = 0.f;                       // this lane's share of db_v

  XmRegs<E> hreg;
  float lreg;
  int yreg;
  xm_fetch_h<E>(H, labels, idx, lse, 0, nv, hreg, lreg, yreg);
  for (int x0 = 0; x0 < nv; x0 += G::ROWS) {           // ascending: a fixed summation order
    __syncthreads();
    xm_put<E>(hreg, hs);
    if ((int)threadIdx.x < G::ROWS) { ls[threadIdx.x] = lreg; ys[threadIdx.x] = yreg; }
    __syncthreads();
    if (x0 + G::ROWS < nv) xm_fetch_h<E>(H, labels, idx, lse, x0 + G::ROWS, nv, hreg, lreg, yreg);
    f32x4_t z[G::NB];
#pragma unroll
    for (int n = 0; n < G::NB; ++n) z[n] = {b, b, b, b};
    xm_dot_tile<E>(hs, wr, t, g, z);    // z[n][r] = z[token x0 + 16n + 4g + r][vocab row v]
#pragma unroll
    for (int n = 0; n < G::NB; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int xl = 16 * n + 4 * g + r;
        float dz = __expf(z[n][r] - ls[xl]) - off;
        if ((int64_t)ys[xl] == v) dz -= hit;
        dz = x0 + xl < nv ? dz * scale : 0.f;
        gb += dz;
        z[n][r] = dz;
      }
    xm_acc_tile<E>(hs, z, t, g, gw);    // dW[v][:] += dz[tile][v] . H[tile]
  }
  gb = xm_sum4(gb);
  if (!vok) return;
#pragma unroll
  for (int m = 0; m < G::M; ++m)
    *(float4*)(dW + v * E + 16 * m + 4 * g) = make_float4(gw[m][0], gw[m][1], gw[m][2], gw[m][3]);
  if (g == 0) db[v] = gb;
}

// mean loss over the valid tokens, fixed reduction tree (as linear_xent.hip)
__global__ __launch_bounds__(1024) void xm_loss_kernel(const float* __restrict__ lossv, int N,
                                                       const int32_t* __restrict__ count,
                                                       float* __restrict__ loss,
                                                       double* __restrict__ acc) {
  __shared__ float red[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float v = 0.f;
  for (int i = tid; i < N; i += 1024) v += lossv[i];
  v = wave_sum(v);
  if (lane == 0) red[w] = v;
  __syncthreads();
  if (w == 0) {
    float t = lane < 16 ? red[lane] : 0.f;
    t = wave_sum(t);
    if (lane == 0) {
      const float L = t / (float)max(1, *count);
      loss[0] = L;
      if (acc) acc[0] += (double)L;
    }
  }
}

// Vocab splits of pass1. Auto: about 2048 workgroups over the whole grid (the
// number of valid tokens is device-side, so the grid is sized for the capacity
// N; with a fifth of the tokens masked, as in Bert4Rec training, some 400 of
// them find work on the 256 CUs x 2), whole W tiles per split, at most 64. Forced (linear_xent_splits):
// n ranges of ceil(V / n) rows, which need not be whole tiles.
void xm_splits(int N, int64_t V, int E, int64_t* VS, int* S) {
  const int64_t rows = 8192 / E;
  const int64_t tiles = (V + rows - 1) / rows;
  int64_t vs;
  if (g_xm_splits > 0) {
    const int64_t want = std::min<int64_t>({g_xm_splits, V, 65535});
    vs = (V + want - 1) / want;
  } else {
    const int64_t ttiles = std::max(1, (N + XM_OWN - 1) / XM_OWN);
    const int64_t want = std::min<int64_t>({64, tiles, std::max<int64_t>(1, 2048 / ttiles)});
    vs = (tiles + want - 1) / want * rows;
  }
  *VS = vs;
  *S = (int)((V + vs - 1) / vs);
}

template <int E>
void xm_run(const LinearXentArgs& a, hipStream_t s) {
  constexpr int XP = E + 4;
  int64_t VS;
  int S;
  xm_splits(a.N, a.V, E, &VS, &S);
  char* ws = (char*)a.workspace;
  int32_t* idx = (int32_t*)ws;
  int32_t* count = idx + a.N;
  float* lse = (float*)(count + 16);
  float* part = lse + a.N;
  part = (float*)(((uintptr_t)part + 15) & ~(uintptr_t)15);
  float* wpart = part + (int64_t)a.N * S * XP;
  hipLaunchKernelGGL(xm_compact_kernel<E>, dim3(1), dim3(1024), 0, s, a.labels, a.N, a.ignore,
                     idx, count, a.dH, a.lossv);
  const int tiles = (a.N + XM_OWN - 1) / XM_OWN;
  hipLaunchKernelGGL(xm_pass1_kernel<E>, dim3(tiles, S), dim3(XM_THREADS), 0, s, a.H, a.W, a.bias,
                     a.V, VS, S, idx, count, part, wpart);
  hipLaunchKernelGGL(xm_merge_kernel<E>, dim3(a.N), dim3(64), 0, s, a.H, a.W, a.bias, a.labels,
                     a.V, S, a.eps, idx, count, part, wpart, lse, a.dH, a.lossv);
  if (a.dW) {
    hipLaunchKernelGGL(xm_wgrad_kernel<E>, dim3((unsigned)((a.V + XM_OWN - 1) / XM_OWN)),
                       dim3(XM_THREADS), 0, s, a.H, a.W, a.bias, a.labels, a.V, a.eps, idx, count,
                       lse, a.dW, a.db);
    if (a.okind >= 0) {                 // the flat optimizer's kernel on W, bias
      for (int p = 0; p < 2; ++p) {
        DenseOptArgs o{};
        o.p = p ? (float*)a.bias : (float*)a.W;
        o.g = p ? a.db : a.dW;
        o.m = p ? a.mb : a.mW;
        o.v = p ? a.vb : a.vW;
        o.n = p ? (a.V + 3) / 4 * 4 : a.V * E;       // (flat buffers are padded)
        o.opt = a.okind; o.hyper = a.ohyper;
        o.beta1 = a.beta1; o.beta2 = a.beta2; o.eps = a.oeps; o.weight_decay = a.owd;
        dense_optimizer(o, s);
      }
    }
  }
  if (a.loss)
    hipLaunchKernelGGL(xm_loss_kernel, dim3(1), dim3(1024), 0, s, a.lossv, a.N, count, a.loss,
                       a.loss_acc);
  TDFO_CHECK_HIP(hipGetLastError());
}

}  // namespace

int linear_xent_splits(int n) {
  const int prev = g_xm_splits;
  if (n >= 0) g_xm_splits = n;
  return prev;
}

size_t linear_xent_mfma_workspace(int N, int64_t V, int E) {
  int64_t VS;
  int S;
  xm_splits(N, V, E, &VS, &S);
  // idx[N] + count (16 ints) + lse[N] + part[N][S][E + 4] + wpart[S][E + 1]
  return (size_t)(2 * N + 16) * 4 + 16 + (size_t)N * S * (E + 4) * 4 + (size_t)S * (E + 1) * 4 + 512;
}

void linear_xent_mfma(const LinearXentArgs& a, int E, hipStream_t s) {
  if (a.N <= 0) return;
  if (a.V <= 0 || a.V >= (int64_t(1) << 31))
    throw std::runtime_error("linear_xent: vocab must be in [1, 2^31)");
  if (E == 128) xm_run<128>(a, s);
  else if (E == 256) xm_run<256>(a, s);
  else throw std::runtime_error("linear_xent (MFMA): hidden width must be 128 or 256");
}

}  // namespace tdfo

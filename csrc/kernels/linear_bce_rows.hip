// Fused Linear + binary cross-entropy (BCE / gBCE) of every token against its
// own positive row and a shared list of negative rows of the output layer,
// hidden widths 16 / 32 / 64 / 128 / 256.
//
//   z[n, c] = H[n] . W[negs[c]] + bias[negs[c]]         (c a valid negative)
//   zy[n]   = H[n] . W[y] + bias[y]                      (y = labels[n])
//   K[n]    = Sv - [y is a valid negative]
//   loss_n  = (beta softplus(-zy) + sum_{c: negs[c] != y} softplus(z[n, c])) / (K[n] + 1)
//   dz      = sigmoid(z[n, c]) / ((K[n] + 1) nv)         (0 where negs[c] == y)
//   dzy     = -beta sigmoid(-zy) / ((K[n] + 1) nv)
// A negative slot whose id is outside [0, V) is a hole: it is skipped and never
// dereferenced. A token whose label is `ignore` or outside [0, V) is ignored
// (zero dH / lossv). Sv = valid negatives, nv = valid tokens; both stay on the
// device, so the launch sequence does not depend on them and is
// graph-capturable. dW / db rows named by a valid negative or by a valid
// token's label are assigned their full gradient (when a token is valid); every
// other row is left as it was. No [N, S] scores in HBM, no float atomics, every
// reduction in a fixed order. softplus and sigmoid come from one exp(-|z|), so
// nothing overflows for a finite z.
//
// The stages and the tiling are those of linear_xent_rows.hip (helpers in
// tdfo_xent_rows_dev.h); no normaliser links the candidates, so there is no
// running maximum, no rescale and no saved lse:
//   compact : block 0: valid tokens -> idx[], nv (and zeros for the ignored);
//             block 1: valid negatives -> crow[] (W row), cbias[], Sv, and the
//             split geometry
//   pass1   : grid (64-token tile, negative split s), W rows fetched through
//             crow[] into the LDS tile, the next tile's loads in flight;
//             part[token][s] = (sum softplus, label seen, O = sum_c sigmoid(z_c) W_c)
//             over the negatives that are not the token's label
//   merge   : one wave per valid token, splits in ascending order, plus the
//             positive's row -> loss, dH, dzy[token], kinv[valid token]
//   wgrad_n : grid (64-negative tile, token split k), the split's valid tokens
//             streamed in ascending order, scores recomputed. A call of at most
//             br_tok tokens has one split and each owner stores its row at
//             dW + crow * E; a longer one cuts the valid tokens into splits of
//             br_tok (one workgroup per 64 negatives streaming every token is
//             a serial walk that leaves the GPU empty), each owner stores its
//             partial row in the workspace, and
//   reduce  : one wave per valid negative adds the partial rows in ascending
//             split order and stores the row
//   wgrad_p : one wave per position of `order` (token indices, equal labels
//             adjacent, ascending inside a run); the wave at the head of a run
//             of valid tokens walks it and writes the label's row: added to what
//             wgrad_n stored when the row is also a valid negative (binary
//             search in crow[], ascending because the valid negs are), else
//             assigned
//   loss    : fixed-tree mean over the valid tokens (+ fp64 running sum)
#include "tdfo_xent_rows_dev.h"

namespace tdfo {
namespace {

// a = exp(-|z|): softplus(z) = max(z, 0) + log(1 + a), sigmoid(z) = (z >= 0 ? 1 : a) / (1 + a)
__device__ __forceinline__ void br_sp_sig(float z, float& sp, float& sg) {
  const float a = __expf(-fabsf(z)), d = 1.f + a;
  sp = fmaxf(z, 0.f) + __logf(d);
  sg = (z >= 0.f ? 1.f : a) * __builtin_amdgcn_rcpf(d);
}

// valid tokens per split of the negatives' wgrad: 8 / 32 / 64 streamed tiles;
// the partial rows are N / br_tok x S x (E + 4) floats, 6 - 13 % of [N, S] scores
template <int E>
constexpr int br_tok() { return E <= 64 ? 1024 : 2048; }

__device__ __forceinline__ bool br_label_ok(int64_t y, int64_t ignore, int64_t V) {
  return y != ignore && y >= 0 && y < V;
}

// block 0: tokens; block 1: negatives and the split geometry (want / forced as
// in xr_compact_kernel)
template <int E>
__global__ __launch_bounds__(1024) void br_compact_kernel(
    const int64_t* __restrict__ negs, const float* __restrict__ bias,
    const int64_t* __restrict__ labels, int N, int S, int64_t V, int64_t ignore, int want,
    int forced, int32_t* __restrict__ idx, int32_t* __restrict__ crow, float* __restrict__ cbias,
    int32_t* __restrict__ counts, float* __restrict__ dH, float* __restrict__ lossv) {
  __shared__ int wsum[16];
  __shared__ int base;
  if (blockIdx.x == 0) {
    const int nv = xr_compact(
        N, wsum, &base,
        [&](int j) {
          const bool ok = br_label_ok(labels[j], ignore, V);
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
      S, wsum, &base,
      [&](int j) {
        const int64_t r = negs[j];
        return r >= 0 && r < V;
      },
      [&](int j, int p) {
        const int64_t r = negs[j];
        crow[p] = (int)r;
        cbias[p] = bias[r];
      });
  if (threadIdx.x == 0) xr_cut_splits<E>(mv, want, forced, counts);
}

// compacted negatives [r0, r0 + ROWS) of the split ending at v1 -> registers
// (W rows gathered through crow); rows past v1 are zeros with row id -1
template <int E>
__device__ __forceinline__ void br_fetch_w(const float* __restrict__ W,
                                           const int32_t* __restrict__ crow,
                                           const float* __restrict__ cbias, int r0, int v1,
                                           XrRegs<E>& R, float& b, int& row) {
  using G = XrGeo<E>;
#pragma unroll
  for (int k = 0; k < G::NV; ++k) {
    const int e = (int)threadIdx.x + k * XR_THREADS, r = e / G::V4, c = e - r * G::V4;
    R.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < v1) R.v[k] = *(const float4*)(W + (int64_t)crow[r0 + r] * E + 4 * c);
  }
  b = 0.f;
  row = -1;
  if ((int)threadIdx.x < G::ROWS && r0 + (int)threadIdx.x < v1) {
    b = cbias[r0 + (int)threadIdx.x];
    row = crow[r0 + (int)threadIdx.x];
  }
}

template <int E>
__global__ __launch_bounds__(XR_THREADS, 2) void br_pass1_kernel(
    const float* __restrict__ H, const float* __restrict__ W, const int64_t* __restrict__ labels,
    int S, const int32_t* __restrict__ idx, const int32_t* __restrict__ crow,
    const float* __restrict__ cbias, const int32_t* __restrict__ counts,
    float* __restrict__ part) {
  using G = XrGeo<E>;
  constexpr int XP = E + 4;             // partial record: sum softplus, label seen, pad, pad, O[E]
  __shared__ __attribute__((aligned(16))) float ws[G::ROWS * G::LD];
  __shared__ float bs[G::ROWS];
  __shared__ int rs[G::ROWS];
  const int tile = blockIdx.x, s = blockIdx.y;  // x = token tile: neighbours share W rows in L2
  const int nv = counts[XR_NV], mv = counts[XR_MV], VS = counts[XR_VS];
  if (s >= counts[XR_SV] || tile * XR_OWN >= nv) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int v0 = s * VS, v1 = min(mv, v0 + VS);
  const int j = tile * XR_OWN + 16 * w + t;            // this lane's valid token
  const bool jok = j < nv;
  const int n = jok ? idx[j] : 0;
  const int y = jok ? (int)labels[n] : -2;              // (-1 is fetch_w's "no row"; V < 2^31)

  float h[G::NS];
  xr_own<E>(H + (int64_t)n * E, g, jok, h);
  f32x4_t o[G::M];
#pragma unroll
  for (int m = 0; m < G::M; ++m) o[m] = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f, seen = 0.f;            // this lane's share of the token's sum / label seen

  XrRegs<E> wreg;
  float breg;
  int rreg;
  br_fetch_w<E>(W, crow, cbias, v0, v1, wreg, breg, rreg);
  for (int r0 = v0; r0 < v1; r0 += G::ROWS) {
    __syncthreads();                    // the previous tile is consumed
    xr_put<E>(wreg, ws);
    if ((int)threadIdx.x < G::ROWS) { bs[threadIdx.x] = breg; rs[threadIdx.x] = rreg; }
    __syncthreads();
    if (r0 + G::ROWS < v1)              // the next tile's loads fly during this one
      br_fetch_w<E>(W, crow, cbias, r0 + G::ROWS, v1, wreg, breg, rreg);
    f32x4_t x[G::NB];
#pragma unroll
    for (int nb = 0; nb < G::NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[nb][r] = bs[16 * nb + 4 * g + r];
    xr_dot_tile<E>(ws, h, t, g, x);     // x[nb][r] = z[token][negative r0 + 16nb + 4g + r]
#pragma unroll
    for (int nb = 0; nb < G::NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rs[16 * nb + 4 * g + r];        // -1 past v1
        float sp, sg;
        br_sp_sig(x[nb][r], sp, sg);
        const bool neg = row >= 0 && row != y;
        if (row == y) seen = 1.f;
        l += neg ? sp : 0.f;
        x[nb][r] = neg ? sg : 0.f;
      }
    xr_acc_tile<E>(ws, x, t, g, o);     // O[token][:] += sigmoid(z)[token][tile] . W[tile]
  }
  l = xr_sum4(l);
  seen = xr_max4(seen);
  if (jok) {
    float* p = part + ((int64_t)j * S + s) * XP;
    if (g == 0) { p[0] = l; p[1] = seen; }
#pragma unroll
    for (int m = 0; m < G::M; ++m)
      *(float4*)(p + 4 + 16 * m + 4 * g) = make_float4(o[m][0], o[m][1], o[m][2], o[m][3]);
  }
}

// one wave per valid token; lane k owns hidden dims k, k + 64, ... (< E)
template <int E>
__global__ __launch_bounds__(64) void br_merge_kernel(
    const float* __restrict__ H, const float* __restrict__ W, const float* __restrict__ bias,
    const int64_t* __restrict__ labels, int S, float beta, const int32_t* __restrict__ idx,
    const int32_t* __restrict__ counts, const float* __restrict__ part, float* __restrict__ dzy,
    float* __restrict__ kinv, float* __restrict__ dH, float* __restrict__ lossv) {
  constexpr int XP = E + 4, Q = XrGeo<E>::Q;
  const int lane = threadIdx.x, j = blockIdx.x;
  const int nv = counts[XR_NV], mv = counts[XR_MV], sv = counts[XR_SV];
  if (j >= nv) return;
  const float* p0 = part + (int64_t)j * S * XP;
  float sum = 0.f, seen = 0.f, acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.f;
  for (int s = 0; s < sv; ++s) {        // split order: deterministic
    const float* p = p0 + (int64_t)s * XP;
    sum += p[0];
    seen += p[1];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int k = lane + 64 * q;
      if (k < E) acc[q] += p[4 + k];
    }
  }
  const int n = idx[j];
  const int64_t y = labels[n];          // valid by the compaction: in [0, V)
  float wy[Q], dot = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int k = lane + 64 * q;
    wy[q] = 0.f;
    if (k < E) {
      wy[q] = W[y * E + k];
      dot += wy[q] * H[(int64_t)n * E + k];
    }
  }
  const float zy = bias[y] + wave_sum(dot);
  const float k1 = (float)(mv - (seen > 0.f ? 1 : 0) + 1);           // K + 1
  const float ki = 1.f / (k1 * (float)nv);
  const float a = expf(-fabsf(zy)), d = 1.f + a;
  const float spn = fmaxf(-zy, 0.f) + logf(d);                       // softplus(-zy)
  const float sgn = (zy >= 0.f ? a : 1.f) / d;                       // sigmoid(-zy)
  const float gy = -beta * sgn * ki;
  if (lane == 0) {
    lossv[n] = (beta * spn + sum) / k1;
    dzy[n] = gy;
    kinv[j] = ki;
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int k = lane + 64 * q;
    if (k < E) dH[(int64_t)n * E + k] = ki * acc[q] + gy * wy[q];
  }
}

// valid tokens [x0, x0 + ROWS) -> registers (H rows gathered through idx, kinv,
// label); tokens past nv are zeros with label -1
template <int E>
__device__ __forceinline__ void br_fetch_h(const float* __restrict__ H,
                                           const int64_t* __restrict__ labels,
                                           const int32_t* __restrict__ idx,
                                           const float* __restrict__ kinv, int x0, int nv,
                                           XrRegs<E>& R, float& ki, int& y) {
  using G = XrGeo<E>;
#pragma unroll
  for (int k = 0; k < G::NV; ++k) {
    const int e = (int)threadIdx.x + k * XR_THREADS, r = e / G::V4, c = e - r * G::V4;
    R.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (x0 + r < nv) R.v[k] = *(const float4*)(H + (int64_t)idx[x0 + r] * E + 4 * c);
  }
  ki = 0.f;
  y = -1;
  const int x = x0 + (int)threadIdx.x;
  if ((int)threadIdx.x < G::ROWS && x < nv) {
    ki = kinv[x];
    y = (int)labels[idx[x]];            // V < 2^31
  }
}

template <int E>
__global__ __launch_bounds__(XR_THREADS, 2) void br_wgrad_neg_kernel(
    const float* __restrict__ H, const float* __restrict__ W, const int64_t* __restrict__ labels,
    const int32_t* __restrict__ idx, const int32_t* __restrict__ crow,
    const float* __restrict__ cbias, const int32_t* __restrict__ counts,
    const float* __restrict__ kinv, int S, float* __restrict__ wpart, float* __restrict__ dW,
    float* __restrict__ db) {
  using G = XrGeo<E>;
  constexpr int TOK = br_tok<E>();
  __shared__ __attribute__((aligned(16))) float hs[G::ROWS * G::LD];
  __shared__ float ks[G::ROWS];
  __shared__ int ys[G::ROWS];
  const int nv = counts[XR_NV], mv = counts[XR_MV];
  const int split = blockIdx.y, t0 = split * TOK, t1 = min(nv, t0 + TOK);   // this split's tokens
  if (t0 >= nv || (int)blockIdx.x * XR_OWN >= mv) return;  // (no valid token: nothing is written)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int c = (int)blockIdx.x * XR_OWN + 16 * w + t;     // this lane's compacted negative
  const bool vok = c < mv;
  const int64_t v = vok ? crow[c] : 0;                      // its row of W
  const int vrow = vok ? (int)v : -2;                       // (-1 is fetch_h's "no token")

  float wr[G::NS];
  xr_own<E>(W + v * E, g, vok, wr);
  const float b = vok ? cbias[c] : 0.f;
  f32x4_t gw[G::M];
#pragma unroll
  for (int m = 0; m < G::M; ++m) gw[m] = {0.f, 0.f, 0.f, 0.f};
  float gb = 0.f;                       // this lane's share of db_v

  XrRegs<E> hreg;
  float kreg;
  int yreg;
  br_fetch_h<E>(H, labels, idx, kinv, t0, t1, hreg, kreg, yreg);
  for (int x0 = t0; x0 < t1; x0 += G::ROWS) {          // ascending: a fixed summation order
    __syncthreads();
    xr_put<E>(hreg, hs);
    if ((int)threadIdx.x < G::ROWS) { ks[threadIdx.x] = kreg; ys[threadIdx.x] = yreg; }
    __syncthreads();
    if (x0 + G::ROWS < t1) br_fetch_h<E>(H, labels, idx, kinv, x0 + G::ROWS, t1, hreg, kreg, yreg);
    f32x4_t z[G::NB];
#pragma unroll
    for (int nb = 0; nb < G::NB; ++nb) z[nb] = {b, b, b, b};
    xr_dot_tile<E>(hs, wr, t, g, z);    // z[nb][r] = z[token x0 + 16nb + 4g + r][negative c]
#pragma unroll
    for (int nb = 0; nb < G::NB; ++nb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int xl = 16 * nb + 4 * g + r;
        float sp, sg;
        br_sp_sig(z[nb][r], sp, sg);
        const int y = ys[xl];                               // -1 past t1 (ks = 0 there)
        const float dz = (y >= 0 && y != vrow) ? sg * ks[xl] : 0.f;
        gb += dz;
        z[nb][r] = dz;
      }
    xr_acc_tile<E>(hs, z, t, g, gw);    // dW[v][:] += dz[tile][c] . H[tile]
  }
  gb = xr_sum4(gb);
  if (!vok) return;
  // one split: the row itself; more: this split's partial row (E floats, then db)
  float* row = wpart ? wpart + ((int64_t)split * S + c) * (E + 4) : dW + v * E;
#pragma unroll
  for (int m = 0; m < G::M; ++m)
    *(float4*)(row + 16 * m + 4 * g) = make_float4(gw[m][0], gw[m][1], gw[m][2], gw[m][3]);
  if (g == 0) (wpart ? row + E : db + v)[0] = gb;
}

// one wave per valid negative: its partial rows in ascending split order
template <int E>
__global__ __launch_bounds__(64) void br_wgrad_reduce_kernel(
    int S, const int32_t* __restrict__ crow, const int32_t* __restrict__ counts,
    const float* __restrict__ wpart, float* __restrict__ dW, float* __restrict__ db) {
  constexpr int Q = XrGeo<E>::Q, TOK = br_tok<E>();
  const int lane = threadIdx.x, c = blockIdx.x;
  const int nv = counts[XR_NV], mv = counts[XR_MV];
  if (nv == 0 || c >= mv) return;
  const int splits = (nv + TOK - 1) / TOK;
  float acc[Q], gb = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float* p = wpart + ((int64_t)s * S + c) * (E + 4);
    gb += p[E];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int k = lane + 64 * q;
      if (k < E) acc[q] += p[k];
    }
  }
  const int64_t v = crow[c];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int k = lane + 64 * q;
    if (k < E) dW[v * E + k] = acc[q];
  }
  if (lane == 0) db[v] = gb;
}

// one wave per position of order; lane k owns hidden dims k, k + 64, ... (< E)
template <int E>
__global__ __launch_bounds__(64) void br_wgrad_pos_kernel(
    const float* __restrict__ H, const int64_t* __restrict__ labels,
    const int32_t* __restrict__ order, int N, int64_t V, int64_t ignore,
    const int32_t* __restrict__ crow, const int32_t* __restrict__ counts,
    const float* __restrict__ dzy, float* __restrict__ dW, float* __restrict__ db) {
  constexpr int Q = XrGeo<E>::Q;
  const int lane = threadIdx.x, p = blockIdx.x;
  const int n0 = order[p];
  if (n0 < 0 || n0 >= N) return;
  const int64_t y = labels[n0];
  if (!br_label_ok(y, ignore, V)) return;
  if (p > 0) {                          // not the head of its run
    const int np = order[p - 1];
    if (np >= 0 && np < N && labels[np] == y) return;
  }
  float acc[Q], gb = 0.f;
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.f;
  for (int x = p; x < N; ++x) {         // the run, in order: a fixed summation order
    const int n = order[x];
    if (n < 0 || n >= N || labels[n] != y) break;
    const float gy = dzy[n];
    gb += gy;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int k = lane + 64 * q;
      if (k < E) acc[q] += gy * H[(int64_t)n * E + k];
    }
  }
  int lo = 0, hi = counts[XR_MV];       // is the row a valid negative (crow ascending)?
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (crow[mid] < (int)y) lo = mid + 1; else hi = mid;
  }
  const bool add = lo < counts[XR_MV] && crow[lo] == (int)y;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int k = lane + 64 * q;
    if (k < E) dW[y * E + k] = (add ? dW[y * E + k] : 0.f) + acc[q];
  }
  if (lane == 0) db[y] = (add ? db[y] : 0.f) + gb;
}

struct BrLayout {
  size_t idx, crow, counts, cbias, kinv, dzy, part, wpart, total;
};

// token splits of the negatives' wgrad for the capacity N (the grid's bound;
// the device cuts them from nv)
int br_tsplits(int N, int E) {
  const int tok = E <= 64 ? br_tok<64>() : br_tok<128>();
  return std::max(1, (N + tok - 1) / tok);
}

BrLayout br_layout(int N, int S, int E, int SP) {
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  BrLayout L;
  size_t o = 0;
  L.idx = o;    o = up(o + (size_t)N * 4);
  L.crow = o;   o = up(o + (size_t)S * 4);
  L.counts = o; o = up(o + 16 * 4);
  L.cbias = o;  o = up(o + (size_t)S * 4);
  L.kinv = o;   o = up(o + (size_t)N * 4);
  L.dzy = o;    o = up(o + (size_t)N * 4);
  L.part = o;   o = up(o + (size_t)N * SP * (E + 4) * 4);
  const int ts = br_tsplits(N, E);
  L.wpart = o;  o = up(o + (ts > 1 ? (size_t)ts * S * (E + 4) * 4 : 0));
  L.total = o + 16;                     // (the base is aligned up to 16 bytes)
  return L;
}

template <int E>
void br_run(const LinearBceRowsArgs& a, hipStream_t s) {
  int SP, want, forced;
  xr_splits(a.N, a.S, E, &SP, &want, &forced);
  const BrLayout L = br_layout(a.N, a.S, E, SP);
  char* ws = (char*)(((uintptr_t)a.workspace + 15) & ~(uintptr_t)15);
  int32_t* idx = (int32_t*)(ws + L.idx);
  int32_t* crow = (int32_t*)(ws + L.crow);
  int32_t* counts = (int32_t*)(ws + L.counts);
  float* cbias = (float*)(ws + L.cbias);
  float* kinv = (float*)(ws + L.kinv);
  float* dzy = (float*)(ws + L.dzy);
  float* part = (float*)(ws + L.part);
  hipLaunchKernelGGL(br_compact_kernel<E>, dim3(2), dim3(1024), 0, s, a.negs, a.bias, a.labels,
                     a.N, a.S, a.V, a.ignore, want, forced, idx, crow, cbias, counts, a.dH,
                     a.lossv);
  const int tiles = (a.N + XR_OWN - 1) / XR_OWN;
  hipLaunchKernelGGL(br_pass1_kernel<E>, dim3(tiles, SP), dim3(XR_THREADS), 0, s, a.H, a.W,
                     a.labels, SP, idx, crow, cbias, counts, part);
  hipLaunchKernelGGL(br_merge_kernel<E>, dim3(a.N), dim3(64), 0, s, a.H, a.W, a.bias, a.labels, SP,
                     a.beta, idx, counts, part, dzy, kinv, a.dH, a.lossv);
  if (a.dW) {
    const int ts = br_tsplits(a.N, E);
    float* wpart = ts > 1 ? (float*)(ws + L.wpart) : nullptr;
    hipLaunchKernelGGL(br_wgrad_neg_kernel<E>, dim3((unsigned)((a.S + XR_OWN - 1) / XR_OWN), ts),
                       dim3(XR_THREADS), 0, s, a.H, a.W, a.labels, idx, crow, cbias, counts, kinv,
                       a.S, wpart, a.dW, a.db);
    if (wpart)
      hipLaunchKernelGGL(br_wgrad_reduce_kernel<E>, dim3(a.S), dim3(64), 0, s, a.S, crow, counts,
                         wpart, a.dW, a.db);
    hipLaunchKernelGGL(br_wgrad_pos_kernel<E>, dim3(a.N), dim3(64), 0, s, a.H, a.labels, a.order,
                       a.N, a.V, a.ignore, crow, counts, dzy, a.dW, a.db);
  }
  if (a.loss)
    hipLaunchKernelGGL(xr_loss_kernel, dim3(1), dim3(1024), 0, s, a.lossv, a.N, counts, a.loss,
                       a.loss_acc);
  TDFO_CHECK_HIP(hipGetLastError());
}

}  // namespace

size_t linear_bce_rows_workspace(int N, int S, int E) {
  if (N <= 0 || S <= 0) return 16;
  int SP, want, forced;
  xr_splits(N, S, E, &SP, &want, &forced);
  return br_layout(N, S, E, SP).total;
}

void linear_bce_rows(const LinearBceRowsArgs& a, int E, hipStream_t s) {
  if (a.N <= 0 || a.S <= 0) return;
  if (a.V <= 0 || a.V >= (int64_t(1) << 31))
    throw std::runtime_error("linear_bce_rows: vocab must be in [1, 2^31)");
  if (br_tsplits(a.N, E) > 65535)       // (the grid's y dimension)
    throw std::runtime_error("linear_bce_rows: too many tokens for one call");
  switch (E) {
    case 16: br_run<16>(a, s); break;
    case 32: br_run<32>(a, s); break;
    case 64: br_run<64>(a, s); break;
    case 128: br_run<128>(a, s); break;
    case 256: br_run<256>(a, s); break;
    default:
      throw std::runtime_error("linear_bce_rows: hidden width must be 16, 32, 64, 128 or 256");
  }
}

}  // namespace tdfo

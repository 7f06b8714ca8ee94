// Device helpers shared by the gathered-row loss kernels (linear_xent_rows.hip:
// sampled softmax; linear_bce_rows.hip: BCE / gBCE): the tile geometry, the
// exact-f32 MFMA 16x16x4 tile products, the order-preserving compaction, the
// split rule and the mean-loss kernel. One workgroup = 4 waves = 64 own rows
// held as MFMA B operands; the other side streams through LDS in tiles of
// ROWS x (E + 4) floats (the operand layout is described in
// linear_xent_mfma.hip).
#pragma once
#include "tdfo_common.h"
#include "tdfo_kernels.h"

#include <algorithm>

namespace tdfo {
namespace {

constexpr int XR_OWN = 64;                  // own rows per workgroup (16 per wave)
constexpr int XR_THREADS = 256;
// counts[]: device-side sizes left by the compaction
constexpr int XR_NV = 0, XR_MV = 1, XR_VS = 2, XR_SV = 3;

template <int E>
struct XrGeo {
  static constexpr int NS = E / 4;          // k-steps = operand floats per lane
  static constexpr int M = E / 16;          // 16-wide output column blocks
  static constexpr int LD = E + 4;          // LDS row stride (16-B aligned; 4 LD = 16 mod 32)
  static constexpr int ROWS = 8192 / E < 128 ? 8192 / E : 128;   // streamed rows per tile
  static constexpr int NB = ROWS / 16;      // 16-row blocks per tile
  static constexpr int V4 = E / 4;          // float4s per row
  static constexpr int NV = ROWS * V4 / XR_THREADS;   // float4s per thread and tile
  static constexpr int Q = E < 64 ? 1 : E / 64;       // merge: hidden dims per lane
};

inline int xr_rows(int E) { return 8192 / E < 128 ? 8192 / E : 128; }

__device__ __forceinline__ f32x4_t xr_mfma(float a, float b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float xr_max4(float v) {     // over lanes t, t+16, t+32, t+48
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}

__device__ __forceinline__ float xr_sum4(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// a lane's B operands of one E-float row: k-step 4c + s <-> element 16c + 4g + s
template <int E>
__device__ __forceinline__ void xr_own(const float* __restrict__ row, int g, bool ok,
                                       float (&f)[XrGeo<E>::NS]) {
#pragma unroll
  for (int c = 0; c < E / 16; ++c) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) v = *(const float4*)(row + 16 * c + 4 * g);
    f[4 * c] = v.x; f[4 * c + 1] = v.y; f[4 * c + 2] = v.z; f[4 * c + 3] = v.w;
  }
}

template <int E>
struct XrRegs { float4 v[XrGeo<E>::NV]; };  // this thread's float4s of one streamed tile

// acc[n][r] = c[n][r] + (streamed row 16n + 4g + r) . (own row t)
template <int E>
__device__ __forceinline__ void xr_dot_tile(const float* tile, const float (&own)[XrGeo<E>::NS],
                                            int t, int g, f32x4_t (&acc)[XrGeo<E>::NB]) {
  using G = XrGeo<E>;
#pragma unroll
  for (int n = 0; n < G::NB; ++n) {
    const float* row = tile + (16 * n + t) * G::LD + 4 * g;
    f32x4_t c = acc[n];
#pragma unroll
    for (int k = 0; k < E / 16; ++k) {
      const float4 a = *(const float4*)(row + 16 * k);
      c = xr_mfma(a.x, own[4 * k], c);
      c = xr_mfma(a.y, own[4 * k + 1], c);
      c = xr_mfma(a.z, own[4 * k + 2], c);
      c = xr_mfma(a.w, own[4 * k + 3], c);
    }
    acc[n] = c;
  }
}

// out[m][r] (column 16m + 4g + r of own row t) += sum over the streamed rows x
// of tile[x][column] * val(x, t); val is in the layout xr_dot_tile leaves
template <int E>
__device__ __forceinline__ void xr_acc_tile(const float* tile, const f32x4_t (&val)[XrGeo<E>::NB],
                                            int t, int g, f32x4_t (&out)[XrGeo<E>::M]) {
  using G = XrGeo<E>;
#pragma unroll
  for (int n = 0; n < G::NB; ++n) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* row = tile + (16 * n + 4 * g + r) * G::LD + t;
#pragma unroll
      for (int m = 0; m < G::M; ++m) out[m] = xr_mfma(row[16 * m], val[n][r], out[m]);
    }
  }
}

template <int E>
__device__ __forceinline__ void xr_put(const XrRegs<E>& R, float* tile) {
  using G = XrGeo<E>;
#pragma unroll
  for (int k = 0; k < G::NV; ++k) {
    const int e = (int)threadIdx.x + k * XR_THREADS, r = e / G::V4, c = e - r * G::V4;
    *(float4*)(tile + r * G::LD + 4 * c) = R.v[k];
  }
}

// Order-preserving compaction by one workgroup: out position of every item j
// with keep(j), through emit(j, position); returns the count (in every thread).
template <class Keep, class Emit>
__device__ __forceinline__ int xr_compact(int n, int* wsum, int* base, Keep keep, Emit emit) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) *base = 0;
  __syncthreads();
  for (int s0 = 0; s0 < n; s0 += 1024) {
    const int j = s0 + t;
    const bool v = j < n && keep(j);
    const uint64_t bal = __ballot(v);
    const int pre = __popcll(bal & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int off = *base;
    for (int q = 0; q < w; ++q) off += wsum[q];
    if (v) emit(j, off + pre);
    __syncthreads();
    if (t == 0) {
      int tot = 0;
      for (int q = 0; q < 16; ++q) tot += wsum[q];
      *base += tot;
    }
    __syncthreads();
  }
  return *base;
}

// The split geometry of mv compacted rows, cut by thread 0 of the compaction
// (whole tiles per split unless the count is forced): counts[MV / VS / SV]
template <int E>
__device__ __forceinline__ void xr_cut_splits(int mv, int want, int forced,
                                              int32_t* __restrict__ counts) {
  constexpr int rows = XrGeo<E>::ROWS;
  int vs = 1, sv = 0;
  if (mv > 0) {
    if (forced) {
      const int w = max(1, min(want, mv));
      vs = (mv + w - 1) / w;
    } else {
      const int tiles = (mv + rows - 1) / rows;
      const int w = max(1, min(want, tiles));
      vs = (tiles + w - 1) / w * rows;
    }
    sv = (mv + vs - 1) / vs;
  }
  counts[XR_MV] = mv;
  counts[XR_VS] = vs;
  counts[XR_SV] = sv;
}

// mean loss over the valid tokens, fixed reduction tree (as linear_xent.hip)
__global__ __launch_bounds__(1024) void xr_loss_kernel(const float* __restrict__ lossv, int N,
                                                       const int32_t* __restrict__ counts,
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
      const float L = t / (float)max(1, counts[XR_NV]);
      loss[0] = L;
      if (acc) acc[0] += (double)L;
    }
  }
}

// Splits of pass1 over the streamed side for the capacity (N, M): the grid's
// split dimension S, the count the device aims at (want) and whether it is
// forced. Auto: about 2048 workgroups over the grid, whole tiles per split, at
// most 64 (xm_splits of linear_xent_mfma.hip with M in the place of V). The
// device cuts the splits from the valid count with the same rule and never
// needs more than S of them.
inline void xr_splits(int N, int M, int E, int* S, int* want, int* forced) {
  const int rows = xr_rows(E);
  const int tiles = std::max(1, (M + rows - 1) / rows);
  const int force = linear_xent_splits(-1);
  if (force > 0) {
    *want = *S = std::max(1, std::min({force, M, 65535}));
    *forced = 1;
  } else {
    const int ttiles = std::max(1, (N + XR_OWN - 1) / XR_OWN);
    *want = std::min(64, std::max(1, 2048 / ttiles));
    *S = std::min(*want, tiles);
    *forced = 0;
  }
}

}  // namespace
}  // namespace tdfo

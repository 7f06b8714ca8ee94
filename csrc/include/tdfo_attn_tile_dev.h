// Device helpers shared by the tiled attention kernels (attention_long.hip:
// 64 < T <= 512, per-row data of the whole sequence in LDS;
// attention_stream.hip: T up to 4096, per-row data travels with its tile): the
// dropout hash, the head-dim geometry, the two-step global -> registers -> LDS
// tile path, the exact-f32 MFMA 16x16x4 tile products and the causal block
// order. The operand layout is described at the top of attention_long.hip.
#pragma once
#include <cstdlib>
#include <string>

#include "tdfo_common.h"
#include "tdfo_kernels.h"

namespace tdfo {
namespace {

constexpr int AL_TILE = 64;                 // rows per tile, both sides
constexpr int AL_THREADS = 256;
constexpr float AL_MASKED = -1e9f;          // masked_fill value of the reference model
constexpr float AL_OOR = -3.0e38f;          // keys past T: below every real score

__device__ __forceinline__ uint32_t al_hash3(uint32_t a, uint32_t b, uint32_t c) {
  // the counter hash of attention.hip
  uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u ^ (c + 0x165667B1u) * 0xC2B2AE3Du;
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// dropout multiplier of element (row key rk = (b*H+h)*stride + i, key j); the
// stride is 512 for T <= 512 and 4096 above (attention_stream.hip)
__device__ __forceinline__ float al_keep(uint32_t sd, uint32_t rk, int j, float rate,
                                         float kscale) {
  if (rate <= 0.f) return 1.f;
  const uint32_t r = al_hash3(sd, rk, (uint32_t)j);
  return (float)(r >> 8) * (1.0f / 16777216.0f) >= rate ? kscale : 0.f;
}

__device__ __forceinline__ f32x4_t al_mfma(float a, float b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float al_max4(float v) {     // over lanes t, t+16, t+32, t+48
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}

__device__ __forceinline__ float al_sum4(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// Head-dim geometry. The contraction over d is walked as (chunk c, step s) <->
// d = 4W c + W g + s, so a lane's operands of one chunk are W contiguous
// floats: one float4 at d_k >= 16, a float2 at 8, a scalar at 4.
template <int DK>
struct AlGeo {
  static constexpr int W = DK >= 16 ? 4 : DK / 4;
  static constexpr int C = DK / (4 * W);
  static constexpr int NS = DK / 4;            // k-steps = operand floats per lane
  static constexpr int LD = DK + 4;            // LDS row stride (16-B aligned; 4 LD = 16 mod 32)
  static constexpr int M = (DK + 15) / 16;     // 16-wide output column blocks
};

// a lane's fragment of one DK-float row (global or LDS), times mul
template <int DK, typename P>
__device__ __forceinline__ void al_frag(P row, int g, bool ok, float mul,
                                        float (&f)[AlGeo<DK>::NS]) {
  using G = AlGeo<DK>;
#pragma unroll
  for (int c = 0; c < G::C; ++c) {
    if constexpr (G::W == 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok) v = *(const float4*)(row + 16 * c + 4 * g);
      f[4 * c] = v.x * mul; f[4 * c + 1] = v.y * mul;
      f[4 * c + 2] = v.z * mul; f[4 * c + 3] = v.w * mul;
    } else if constexpr (G::W == 2) {
      float2 v = make_float2(0.f, 0.f);
      if (ok) v = *(const float2*)(row + 2 * g);
      f[0] = v.x * mul; f[1] = v.y * mul;
    } else {
      f[0] = ok ? row[g] * mul : 0.f;
    }
  }
}

// A streamed tile (64 rows x DK floats, row stride `stride` floats, first row
// r0 of a T-row matrix) goes global -> registers -> LDS in two steps, so the
// loads of tile k + 1 are in flight while tile k is computed on. Rows past T
// are zeros.
template <int DK>
struct AlRegs { float4 v[(DK + 15) / 16]; };   // this thread's float4s of one tile

template <int DK>
__device__ __forceinline__ void al_fetch(const float* __restrict__ src, int64_t stride, int r0,
                                         int T, AlRegs<DK>& R) {
  constexpr int V4 = DK / 4;                   // float4s per row
#pragma unroll
  for (int k = 0; k < (DK + 15) / 16; ++k) {
    const int e = (int)threadIdx.x + k * AL_THREADS, r = e / V4, c = e - r * V4;
    R.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < AL_TILE * V4 && r0 + r < T)
      R.v[k] = *(const float4*)(src + (int64_t)(r0 + r) * stride + 4 * c);
  }
}

template <int DK>
__device__ __forceinline__ void al_put(const AlRegs<DK>& R, float mul, float* tile) {
  using G = AlGeo<DK>;
  constexpr int V4 = DK / 4;
#pragma unroll
  for (int k = 0; k < (DK + 15) / 16; ++k) {
    const int e = (int)threadIdx.x + k * AL_THREADS, r = e / V4, c = e - r * V4;
    if (e < AL_TILE * V4)
      *(float4*)(tile + r * G::LD + 4 * c) =
          make_float4(R.v[k].x * mul, R.v[k].y * mul, R.v[k].z * mul, R.v[k].w * mul);
  }
}

// acc[n][r] = (streamed row 16n + 4g + r) . (own row t), n = 0..3
template <int DK>
__device__ __forceinline__ void al_dot_tile(const float* tile, const float (&own)[AlGeo<DK>::NS],
                                            int t, int g, f32x4_t (&acc)[4]) {
  using G = AlGeo<DK>;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    float sf[G::NS];
    al_frag<DK>(tile + (16 * n + t) * G::LD, g, true, 1.f, sf);
    f32x4_t c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < G::NS; ++k) c = al_mfma(sf[k], own[k], c);
    acc[n] = c;
  }
}

// out[m][r] (column 16m + 4g + r of own row t) += sum over the 64 streamed
// rows x of tile[x][column] * val(x, t); val is in the layout al_dot_tile leaves
template <int DK>
__device__ __forceinline__ void al_acc_tile(const float* tile, const f32x4_t (&val)[4], int t,
                                            int g, f32x4_t (&out)[AlGeo<DK>::M]) {
  using G = AlGeo<DK>;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int m = 0; m < G::M; ++m) {
        const bool ok = DK >= 16 || t < DK;    // columns past d_k: zero rows of A
        const float a = ok ? tile[(16 * n + 4 * g + r) * G::LD + 16 * m + (ok ? t : 0)] : 0.f;
        out[m] = al_mfma(a, val[n][r], out[m]);
      }
    }
  }
}

// a_t . b_t of the wave's 16 rows (row t on lane column t; fa / fb: al_frag of
// that row), returned to all four lanes of column t. It is the diagonal of the
// MFMA chain al_dot_tile runs (lane (t, g) holds X[4g + r][t]: the diagonal of
// column t sits in lane g = t >> 2, register r = t & 3), so D = dO . O rounds
// exactly as dP = dO . V does. Where P is one-hot (one valid key) O is that
// key's V bit for bit, and dS = P (dP - D) is then exactly 0, as it is in the
// reference; a D summed in another order leaves dP - D at an ulp of |dO| |V|,
// which leaked 1e-6 .. 3e-6 into dQ and dK rows that are exactly 0.
template <int DK>
__device__ __forceinline__ float al_rowdot(const float (&fa)[AlGeo<DK>::NS],
                                           const float (&fb)[AlGeo<DK>::NS], int t) {
  f32x4_t c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < AlGeo<DK>::NS; ++k) c = al_mfma(fa[k], fb[k], c);
  const int r = t & 3;
  const float d = r == 0 ? c[0] : r == 1 ? c[1] : r == 2 ? c[2] : c[3];
  return __shfl(d, t + 16 * (t >> 2));
}

// one float4 per (lane, m): dst row pointer at column 0 of this head
template <int DK>
__device__ __forceinline__ void al_store(float* dst, const f32x4_t (&v)[AlGeo<DK>::M], int g,
                                         float mul) {
  using G = AlGeo<DK>;
#pragma unroll
  for (int m = 0; m < G::M; ++m) {
    const int d = 16 * m + 4 * g;
    if (d < DK)
      *(float4*)(dst + d) = make_float4(v[m][0] * mul, v[m][1] * mul, v[m][2] * mul, v[m][3] * mul);
  }
}

// Causal block order. The dispatcher is observed to deal consecutive
// workgroups round-robin over the 8 XCDs, so with nt = 8 (or 4) tiles per
// (b, h) the tile index would select the XCD: one XCD would get every longest
// block and the launch would take as long as the full kernel. Hardware block
// b therefore takes logical block (b % 8) * (G / 8) + b / 8 (the tail G % 8
// maps to itself): an XCD works through whole (b, h) groups, which also keeps
// a group's K / V in one L2. Only speed depends on the placement.
__device__ __forceinline__ int al_causal_block(int b, int G) {
  const int g8 = G & ~7;
  return b < g8 ? (b & 7) * (g8 >> 3) + (b >> 3) : b;
}

// Blocks of one (b, h) do unequal work under the causal mask. TDFO_ATTN_CAUSAL_ORDER
// = "natural" keeps the block order of the full kernels; anything else (the
// default) groups a (b, h)'s blocks on one XCD, longest first.
inline int attn_causal_heavy_first() {
  static const int v = [] {
    const char* e = std::getenv("TDFO_ATTN_CAUSAL_ORDER");
    return e && std::string(e) == "natural" ? 0 : 1;
  }();
  return v;
}

}  // namespace
}  // namespace tdfo

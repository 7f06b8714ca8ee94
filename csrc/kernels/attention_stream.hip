// Streaming multi-head self-attention core for 64 < T <= 4096 (long user
// histories of a causal next-item model). The maths, layouts, masked_fill(-1e9)
// semantics, dropout hash, tile geometry and MFMA operand maps are those of
// attention_long.hip (see the top of that file); the helpers both share are in
// tdfo_attn_tile_dev.h. qkv [B,T,3E], out/dout [B,T,E], dqkv [B,T,3E],
// lse [B,H,T], delta [B,H,T], fp32. Nothing of size [B,H,T,T] reaches HBM,
// there are no atomics (results are bit-reproducible) and no scratch.
//
// What differs from attention_long.hip: nothing in a block depends on T but
// the length of its tile loop.
//   - The per-row data of the streamed side travels with its 64-row tile,
//     through the same global -> registers -> LDS path and one tile ahead:
//     key validity (forward, dQ role), lse and D of the streamed queries
//     (dK/dV role). LDS holds two tiles and 64 or 128 row values.
//   - D_i = dO_i . O_i comes from a pre-pass (attn_stream_delta_kernel) that
//     writes the [B,H,T] workspace AttnArgs::delta on the same stream before
//     the two-role backward. It runs al_rowdot, the MFMA chain of dP = dO . V,
//     so a one-hot row's dS is exactly 0 as in attention_long.hip.
//   - The dQ role also accumulates e = rowsum(dS) and U = P.K over its tile
//     loop and stores dQ - e U: the first-order correction from D = dO . O to
//     the rowsum(P o dP~) of its own P and dP~ (see the end of
//     attn_stream_bwd_block). One more tile product in that role.
//   - The dropout row key is (b*H + h) * stride + i with stride 512 for
//     T <= 512 (the mask attention_long.hip draws at the same shape) and 4096
//     above: with 512 there, row (h, i >= 512) would take the mask of
//     (h + 1, i - 512).
#include "tdfo_attn_tile_dev.h"

namespace tdfo {
namespace {

// validity of key j0 + threadIdx.x (threads 0..63; ids: this sample's row)
__device__ __forceinline__ int as_fetch_valid(const int64_t* __restrict__ ids, int64_t pad_id,
                                              int j0, int T) {
  const int j = j0 + (int)threadIdx.x;
  return (int)threadIdx.x < AL_TILE && j < T ? (int)(ids[j] != pad_id) : 0;
}

template <int DK, bool CAUSAL>
__global__ __launch_bounds__(AL_THREADS) void attn_stream_fwd_kernel(AttnArgs a, int heavy,
                                                                     int rowkey) {
  using G = AlGeo<DK>;
  __shared__ __attribute__((aligned(16))) float ks[AL_TILE * G::LD];
  __shared__ __attribute__((aligned(16))) float vs[AL_TILE * G::LD];
  __shared__ int kvalid[AL_TILE];              // the keys of the tile in ks / vs
  const int T = a.T, E = a.H * DK;
  const int nt = (T + AL_TILE - 1) / AL_TILE;
  int bid = blockIdx.x;
  if constexpr (CAUSAL) bid = heavy ? al_causal_block(bid, gridDim.x) : bid;
  const int u = bid % nt, bh = bid / nt;
  const int tile = CAUSAL && heavy ? nt - 1 - u : u;   // (causal: the last tile streams most)
  const int b = bh / a.H, h = bh - b * a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int i = tile * AL_TILE + 16 * w + t;           // this lane's query row
  const int jend = CAUSAL ? min(T, (tile + 1) * AL_TILE) : T;     // keys streamed
  const int jlim = CAUSAL ? min(T, i + 1) : T;                    // keys this query sees
  const bool iok = i < T;
  const float* base = a.qkv + (int64_t)b * T * 3 * E + h * DK;
  const int64_t* idb = a.ids + (int64_t)b * T;
  const uint32_t step = a.step ? (uint32_t)a.step[0] : 0u;
  const uint32_t sd = (uint32_t)a.seed ^ (step * 0x632BE5ABu);
  const uint32_t rk = (uint32_t)(bh * rowkey + i);
  const float kscale = 1.f / (1.f - a.rate);

  float q[G::NS];
  al_frag<DK>(base + (int64_t)(iok ? i : 0) * 3 * E, g, iok, a.scale, q);
  f32x4_t o[G::M];
#pragma unroll
  for (int m = 0; m < G::M; ++m) o[m] = {0.f, 0.f, 0.f, 0.f};
  float mx = AL_OOR, l = 0.f;                 // l: this lane's share of the row sum

  AlRegs<DK> kreg, vreg;
  al_fetch<DK>(base + E, 3 * E, 0, T, kreg);
  al_fetch<DK>(base + 2 * E, 3 * E, 0, T, vreg);
  int kvreg = as_fetch_valid(idb, a.pad_id, 0, T);
  for (int j0 = 0; j0 < jend; j0 += AL_TILE) {
    __syncthreads();                           // the previous tile is consumed
    al_put<DK>(kreg, 1.f, ks);
    al_put<DK>(vreg, 1.f, vs);
    if (threadIdx.x < AL_TILE) kvalid[threadIdx.x] = kvreg;
    __syncthreads();
    if (j0 + AL_TILE < jend) {                  // the next tile's loads fly during this one
      al_fetch<DK>(base + E, 3 * E, j0 + AL_TILE, T, kreg);
      al_fetch<DK>(base + 2 * E, 3 * E, j0 + AL_TILE, T, vreg);
      kvreg = as_fetch_valid(idb, a.pad_id, j0 + AL_TILE, T);
    }
    f32x4_t s[4];
    al_dot_tile<DK>(ks, q, t, g, s);           // s[n][r] = S[i][j0 + 16n + 4g + r]
    float tmx = AL_OOR;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jl = 16 * n + 4 * g + r;
        float v = kvalid[jl] ? s[n][r] : AL_MASKED;
        v = j0 + jl < jlim ? v : AL_OOR;
        s[n][r] = v;
        tmx = fmaxf(tmx, v);
      }
    const float mnew = fmaxf(mx, al_max4(tmx));      // (every tile holds a key < T: mnew >= -1e9)
    const float alpha = __expf(mx - mnew);
    mx = mnew;
    float ln[4];                               // the tile's share of l, summed as a tree
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      float pr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jl = 16 * n + 4 * g + r;
        pr[r] = j0 + jl < jlim ? __expf(s[n][r] - mx) : 0.f;
        s[n][r] = pr[r] * al_keep(sd, rk, j0 + jl, a.rate, kscale);
      }
      ln[n] = (pr[0] + pr[1]) + (pr[2] + pr[3]);
    }
    l = fmaf(l, alpha, (ln[0] + ln[1]) + (ln[2] + ln[3]));
    // The tile's product and its sum of p are formed on their own and join O
    // and l in one fma each: one rounding at |O| (at l) per tile, 64 per row at
    // T = 4096. Accumulated into O and l directly it would be 16 per tile, and
    // the backward's D = dO . O carries the error of O and of its 1 / l into
    // every dS of the row (attention_long.hip has the measured case).
    f32x4_t acc[G::M];
#pragma unroll
    for (int m = 0; m < G::M; ++m) acc[m] = {0.f, 0.f, 0.f, 0.f};
    al_acc_tile<DK>(vs, s, t, g, acc);
#pragma unroll
    for (int m = 0; m < G::M; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[m][r] = fmaf(o[m][r], alpha, acc[m][r]);
  }
  l = al_sum4(l);
  if (iok) {
    al_store<DK>(a.out + ((int64_t)b * T + i) * E + h * DK, o, g, 1.f / l);
    if (g == 0) a.lse[(int64_t)bh * T + i] = mx + __logf(l);
  }
}

// delta[b, h, i] = dO_i . O_i; grid (b, h) x nt, 16 rows per wave
template <int DK>
__global__ __launch_bounds__(AL_THREADS) void attn_stream_delta_kernel(AttnArgs a) {
  using G = AlGeo<DK>;
  const int T = a.T, E = a.H * DK;
  const int nt = (T + AL_TILE - 1) / AL_TILE;
  const int u = blockIdx.x % nt, bh = blockIdx.x / nt;
  const int b = bh / a.H, h = bh - b * a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int i = u * AL_TILE + 16 * w + t;
  const bool ok = i < T;
  const int64_t row = ((int64_t)b * T + (ok ? i : 0)) * E + h * DK;
  float fd[G::NS], fo[G::NS];
  al_frag<DK>(a.dout + row, g, ok, 1.f, fd);
  al_frag<DK>(a.out + row, g, ok, 1.f, fo);
  const float d = al_rowdot<DK>(fd, fo, t);    // (A = dO, B = O: as dP's A = dO, B = V)
  if (ok && g == 0) a.delta[(int64_t)bh * T + i] = d;
}

// al_acc_tile for two value sets against one tile (each LDS word read once):
// o1 += tile^T . v1, o2 += tile^T . v2, each in al_acc_tile's own order
template <int DK>
__device__ __forceinline__ void as_acc_tile2(const float* tile, const f32x4_t (&v1)[4],
                                             const f32x4_t (&v2)[4], int t, int g,
                                             f32x4_t (&o1)[AlGeo<DK>::M],
                                             f32x4_t (&o2)[AlGeo<DK>::M]) {
  using G = AlGeo<DK>;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int m = 0; m < G::M; ++m) {
        const bool ok = DK >= 16 || t < DK;    // columns past d_k: zero rows of A
        const float a = ok ? tile[(16 * n + 4 * g + r) * G::LD + 16 * m + (ok ? t : 0)] : 0.f;
        o1[m] = al_mfma(a, v1[n][r], o1[m]);
        o2[m] = al_mfma(a, v2[n][r], o2[m]);
      }
    }
  }
}

// One backward block: KV = false, the dQ role (own = 64 queries); KV = true,
// the dK/dV role (own = 64 keys). s1 / s2: the streamed tiles (K, V) or
// (Q/sqrt(dk), dO); rowa / rowb [64]: the streamed tile's lse and D (KV role),
// or its keys' validity in rowa (dQ role).
template <int DK, bool KV, bool CAUSAL>
__device__ __forceinline__ void attn_stream_bwd_block(const AttnArgs& a, int b, int h, int tile,
                                                      int rowkey, float* s1, float* s2,
                                                      float* rowa, float* rowb) {
  using G = AlGeo<DK>;
  const int T = a.T, E = a.H * DK, bh = b * a.H + h;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int y = tile * AL_TILE + 16 * w + t;           // this lane's own row (query or key)
  const bool yok = y < T;
  const float* base = a.qkv + (int64_t)b * T * 3 * E + h * DK;
  const float* dob = a.dout + (int64_t)b * T * E + h * DK;
  const float* lseb = a.lse + (int64_t)bh * T;
  const float* delb = a.delta + (int64_t)bh * T;
  const int64_t* idb = a.ids + (int64_t)b * T;
  const uint32_t step = a.step ? (uint32_t)a.step[0] : 0u;
  const uint32_t sd = (uint32_t)a.seed ^ (step * 0x632BE5ABu);
  const float kscale = 1.f / (1.f - a.rate), invT = 1.f / (float)T;
  const int yc = yok ? y : 0;

  float own1[G::NS], own2[G::NS];
  float ylse = 0.f, yD = 0.f;                  // dQ role: this query's lse and D
  bool yvalid = false;                         // KV role: this key's validity
  if constexpr (KV) {
    al_frag<DK>(base + (int64_t)yc * 3 * E + E, g, yok, 1.f, own1);        // K
    al_frag<DK>(base + (int64_t)yc * 3 * E + 2 * E, g, yok, 1.f, own2);    // V
    yvalid = yok && idb[yc] != a.pad_id;
  } else {
    al_frag<DK>(base + (int64_t)yc * 3 * E, g, yok, a.scale, own1);        // Q / sqrt(dk)
    al_frag<DK>(dob + (int64_t)yc * E, g, yok, 1.f, own2);                 // dO
    ylse = yok ? lseb[yc] : 0.f;
    yD = yok ? delb[yc] : 0.f;
  }
  f32x4_t g1[G::M], g2[G::M];                  // dQ, U = P.K (its correction) | dK, dV
  float esum = 0.f;                            // dQ role: this lane's share of the row sum of dS
#pragma unroll
  for (int m = 0; m < G::M; ++m) { g1[m] = {0.f, 0.f, 0.f, 0.f}; g2[m] = {0.f, 0.f, 0.f, 0.f}; }

  const float* src1 = KV ? base : base + E;                  // Q | K
  const float* src2 = KV ? dob : base + 2 * E;               // dO | V
  const int64_t st2 = KV ? E : 3 * E;
  const float mul1 = KV ? a.scale : 1.f;                     // (Q / sqrt(dk))
  // causal: keys 0 .. own tile for a query tile, queries own tile .. for a key tile
  const int xbeg = CAUSAL && KV ? tile * AL_TILE : 0;
  const int xend = CAUSAL && !KV ? min(T, (tile + 1) * AL_TILE) : T;
  // streamed rows x that pair with own row y: keys x <= y | queries x >= y
  const int xlo = CAUSAL && KV ? y : 0, xhi = CAUSAL && !KV ? min(T, y + 1) : T;
  // the row data of streamed row x0 + threadIdx.x (threads 0..63)
  float ra = 0.f, rb = 0.f;
  auto fetch_rows = [&](int x0) {
    const int x = x0 + (int)threadIdx.x;
    const bool ok = (int)threadIdx.x < AL_TILE && x < T;
    if constexpr (KV) {
      ra = ok ? lseb[x] : 0.f;
      rb = ok ? delb[x] : 0.f;
    } else {
      ra = ok && idb[x] != a.pad_id ? 1.f : 0.f;
    }
  };
  AlRegs<DK> r1, r2;
  al_fetch<DK>(src1, 3 * E, xbeg, T, r1);
  al_fetch<DK>(src2, st2, xbeg, T, r2);
  fetch_rows(xbeg);
  for (int x0 = xbeg; x0 < xend; x0 += AL_TILE) {    // ascending: a fixed summation order
    __syncthreads();
    al_put<DK>(r1, mul1, s1);
    al_put<DK>(r2, 1.f, s2);
    if (threadIdx.x < AL_TILE) {
      rowa[threadIdx.x] = ra;
      if constexpr (KV) rowb[threadIdx.x] = rb;
    }
    __syncthreads();
    if (x0 + AL_TILE < xend) {                 // the next tile's loads fly during this one
      al_fetch<DK>(src1, 3 * E, x0 + AL_TILE, T, r1);
      al_fetch<DK>(src2, st2, x0 + AL_TILE, T, r2);
      fetch_rows(x0 + AL_TILE);
    }
    f32x4_t sc[4], dp[4];
    al_dot_tile<DK>(s1, own1, t, g, sc);       // S  (query, key) in (x, y) or (y, x)
    al_dot_tile<DK>(s2, own2, t, g, dp);       // dP~ = dO . V^T
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int xl = 16 * n + 4 * g + r, x = x0 + xl;
        const int i = KV ? x : y, j = KV ? y : x;
        const bool inr = x < xhi && yok && (!CAUSAL || x >= xlo);
        const bool valid = KV ? yvalid : rowa[xl] != 0.f;
        const float lse = KV ? rowa[xl] : ylse, D = KV ? rowb[xl] : yD;
        // a masked key has P = 0, except in a row whose visible keys are all
        // PAD, which is uniform over them: every score is -1e9 and lse =
        // -1e9 + log n rounds to -1e9 in f32 (n <= 4096), so exp(s - lse)
        // would give 1, not 1 / n; such a row is recognised by its lse
        float p = valid ? __expf(sc[n][r] - lse)
                        : (lse < -5e8f ? (CAUSAL ? __frcp_rn((float)(i + 1)) : invT) : 0.f);
        p = inr ? p : 0.f;
        const float km = al_keep(sd, (uint32_t)(bh * rowkey + i), j, a.rate, kscale);
        const float ds = p * (dp[n][r] * km - D);
        sc[n][r] = valid ? ds : 0.f;                         // dS (masked_fill: no gradient)
        if constexpr (KV) {
          dp[n][r] = p * km;                                 // P~
        } else {
          esum += ds;                                        // (every visible key, masked or not)
          dp[n][r] = valid ? p : 0.f;                        // P of the keys that take a gradient
        }
      }
    if constexpr (KV) {
      al_acc_tile<DK>(s1, sc, t, g, g1);       // dK += dS^T.Q/sqrt(dk)
      al_acc_tile<DK>(s2, dp, t, g, g2);       // dV += P~^T.dO
    } else {
      as_acc_tile2<DK>(s1, sc, dp, t, g, g1, g2);            // dQ += dS.K, U += P.K
    }
  }
  if constexpr (!KV) {
    // The row sum of dS is 0 when D equals rowsum(P o dP~) of this loop's own P
    // and dP~. D = dO . O does not: it carries the forward's rounding of O and
    // its own chain's, an ulp of |dO| |O|, and in a nearly one-hot row, where
    // dP - D at the winning key is 1 - P of either, that error enters
    // dQ = sum_k dS_k k_k at full size against a row that cancels to 1e-3 of
    // |k| (at T = 1087, 17 tiles of roundings in O, dqkv missed 8 x the
    // reference's error: 10.6 x). e = sum_k dS_k, a sum of small terms, is
    // to first order rowsum(P o dP~) - D, what D lacks; dQ = sum_k P_k (dP~_k -
    // D - e) k_k = dQ(D) - e U. The reference forms D from the same dP~ and
    // has this cancellation built in. e = 0 and U = 0 keep the rows that are
    // exactly 0 (one valid key: dS = 0; no valid key: P = 0 here) exactly 0.
    const float e = al_sum4(esum);
#pragma unroll
    for (int m = 0; m < G::M; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) g1[m][r] = fmaf(-e, g2[m][r], g1[m][r]);
  }
  if (!yok) return;
  float* dst = a.dqkv + ((int64_t)b * T + y) * 3 * E + h * DK;
  if constexpr (KV) {
    al_store<DK>(dst + E, g1, g, 1.f);
    al_store<DK>(dst + 2 * E, g2, g, 1.f);
  } else {
    al_store<DK>(dst, g1, g, a.scale);
  }
}

// grid: (b, h) x [nt dQ tiles | nt dK/dV tiles] in one launch
template <int DK, bool CAUSAL>
__global__ __launch_bounds__(AL_THREADS) void attn_stream_bwd_kernel(AttnArgs a, int heavy,
                                                                     int rowkey) {
  using G = AlGeo<DK>;
  __shared__ __attribute__((aligned(16))) float s1[AL_TILE * G::LD];
  __shared__ __attribute__((aligned(16))) float s2[AL_TILE * G::LD];
  __shared__ float rowa[AL_TILE], rowb[AL_TILE];
  const int nt = (a.T + AL_TILE - 1) / AL_TILE;
  int bid = blockIdx.x;
  if constexpr (CAUSAL) bid = heavy ? al_causal_block(bid, gridDim.x) : bid;
  const int u = bid % (2 * nt), bh = bid / (2 * nt);
  const int b = bh / a.H, h = bh - b * a.H;
  // (causal: the last query tile and the first key tile stream most)
  if (u < nt)
    attn_stream_bwd_block<DK, false, CAUSAL>(a, b, h, CAUSAL && heavy ? nt - 1 - u : u, rowkey,
                                             s1, s2, rowa, rowb);
  else
    attn_stream_bwd_block<DK, true, CAUSAL>(a, b, h, u - nt, rowkey, s1, s2, rowa, rowb);
}

void check_stream(const AttnArgs& a, bool bwd) {
  if (a.T <= ATTN_SHORT_MAXT || a.T > ATTN_STREAM_MAXT)
    throw std::runtime_error("attention (streaming): 64 < T <= 4096");
  if (!a.lse || !a.out) throw std::runtime_error("attention (streaming): lse / out missing");
  if (bwd && (!a.dout || !a.dqkv || !a.delta))
    throw std::runtime_error("attention_stream_bwd: dout / dqkv / delta missing");
  const int64_t nt = (a.T + AL_TILE - 1) / AL_TILE;
  if ((int64_t)a.B * a.H * nt * 2 > 0x7FFFFFFFll ||
      (int64_t)a.B * a.H * ATTN_STREAM_MAXT > 0x7FFFFFFFll)
    throw std::runtime_error("attention (streaming): B * H too large");
}

}  // namespace

#define TDFO_ATTN_STREAM_LAUNCH(KERNEL, DK, GRID)                                          \
  if (a.causal)                                                                            \
    hipLaunchKernelGGL((KERNEL<DK, true>), dim3(GRID), dim3(AL_THREADS), 0, s, a, heavy,   \
                       rowkey);                                                            \
  else                                                                                     \
    hipLaunchKernelGGL((KERNEL<DK, false>), dim3(GRID), dim3(AL_THREADS), 0, s, a, 0,      \
                       rowkey);                                                            \
  break;
#define TDFO_ATTN_STREAM_DISPATCH(KERNEL, GRID)                                          \
  {                                                                                      \
    const int heavy = a.causal ? attn_causal_heavy_first() : 0;                          \
    const int rowkey = a.T > ATTN_LONG_MAXT ? ATTN_STREAM_MAXT : ATTN_LONG_MAXT;         \
    switch (a.dk) {                                                                      \
      case 4: TDFO_ATTN_STREAM_LAUNCH(KERNEL, 4, GRID)                                   \
      case 8: TDFO_ATTN_STREAM_LAUNCH(KERNEL, 8, GRID)                                   \
      case 16: TDFO_ATTN_STREAM_LAUNCH(KERNEL, 16, GRID)                                 \
      case 32: TDFO_ATTN_STREAM_LAUNCH(KERNEL, 32, GRID)                                 \
      case 64: TDFO_ATTN_STREAM_LAUNCH(KERNEL, 64, GRID)                                 \
      default: throw std::runtime_error("attention: d_k must be 4/8/16/32/64");          \
    }                                                                                    \
  }

void attention_stream_fwd(const AttnArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  check_stream(a, false);
  const int nt = (a.T + AL_TILE - 1) / AL_TILE;
  TDFO_ATTN_STREAM_DISPATCH(attn_stream_fwd_kernel, a.B * a.H * nt);
  TDFO_CHECK_HIP(hipGetLastError());
}

void attention_stream_bwd(const AttnArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  check_stream(a, true);
  const int nt = (a.T + AL_TILE - 1) / AL_TILE;
  const dim3 dgrid(a.B * a.H * nt), block(AL_THREADS);
  switch (a.dk) {                              // D of every query, before either role reads it
    case 4: hipLaunchKernelGGL(attn_stream_delta_kernel<4>, dgrid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL(attn_stream_delta_kernel<8>, dgrid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL(attn_stream_delta_kernel<16>, dgrid, block, 0, s, a); break;
    case 32: hipLaunchKernelGGL(attn_stream_delta_kernel<32>, dgrid, block, 0, s, a); break;
    case 64: hipLaunchKernelGGL(attn_stream_delta_kernel<64>, dgrid, block, 0, s, a); break;
    default: throw std::runtime_error("attention: d_k must be 4/8/16/32/64");
  }
  TDFO_CHECK_HIP(hipGetLastError());
  TDFO_ATTN_STREAM_DISPATCH(attn_stream_bwd_kernel, a.B * a.H * nt * 2);
  TDFO_CHECK_HIP(hipGetLastError());
}
#undef TDFO_ATTN_STREAM_DISPATCH
#undef TDFO_ATTN_STREAM_LAUNCH

}  // namespace tdfo

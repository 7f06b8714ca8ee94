// Full-catalogue top-K retrieval and full-ranking eval:
//   score[b, v] = sum_e Q[b, e] W[v, e] (+ bias[v]),  v in [v_lo, v_hi),
// the K best items of every query under the total order (score descending,
// id ascending) and, with a target, the number of eligible items other than
// the target scoring >= the target. No [B, V] tensor, no float atomics.
//
// Scores come from the exact-f32 MFMA (v_mfma_f32_16x16x4_f32): a k-ordered
// fmaf chain per (query, item) that depends on nothing but that query row and
// that item row, so a score has the same bits in every tile, split and launch
// (the target's score is taken from the same chain by topk_target_kernel).
// Lane (col = lane & 15, g = lane >> 4) holds float4 e = 16 c + 4 g .. + 3 of
// query / item row `col` as A / B operand; MFMA step (c, j) multiplies element
// j of both, so the chain runs over e in the order c, j, g.
//
// topk_scan_kernel: one block = 64 queries (4 A tiles kept in registers) x one
// of S ranges of V; 8 waves, each streams 16 item rows per iteration straight
// from global / L2 and reuses the B fragment for the 4 A tiles (4 independent
// accumulators). At E = 128 / 256 a block holds 32 queries (2 A tiles: E / 2
// registers per lane, half the candidate LDS) and an item row passes through
// a ring of two 64-element groups instead of waiting whole in registers; the
// chain's order over e is the same (c, j, g). A (score, id) pair is one 64-bit key whose integer order is
// the total order. Per query row LDS holds a threshold key (the current K-th
// best) and 256 candidate slots. A score is first compared with the
// threshold's score (one float compare); only where a lane of the wave passes
// is the key built and tested exactly, and keys above the threshold are
// appended (LDS atomic counter; order inside the buffer is free). A buffer that fills
// up is compacted by its wave: excluded ids dropped (O(X) per compaction, not
// per score), the K-th largest key selected, the K keys from it up kept, the
// threshold raised to it; keys that found no room are appended after that.
// The block ends by ranking each query's buffer and writing its sorted K keys
// to part[b][split][K] and its >= target count to cpart[split][b].
// topk_merge_kernel: one block per query merges the S sorted lists (rank of a
// key = sum over lists of a binary search; keys below min_s list_s[ceil(K/S)-1]
// cannot reach the top K and are skipped) and sums the counts in split order.
// Excluded items are not tested per score for the rank either: the scan counts
// every in-range item scoring >= the target (the target too, if in range), and
// topk_target_kernel counts the distinct excluded in-range ids other than the
// target scoring >= it; the merge subtracts both.
#include "tdfo_common.h"
#include "tdfo_kernels.h"

namespace tdfo {
namespace {

constexpr int TK_WAVES = 8;
// query tiles (of 16) a block keeps in registers: E / 4 * NT registers per lane
constexpr int tk_nt(int E) { return E <= 64 ? 4 : 2; }
constexpr int tk_qt(int E) { return 16 * tk_nt(E); }   // queries per block
constexpr int TK_GC = 4;                // wide E: 16-element chunks of an item row per load group
constexpr int TK_IT = 16 * TK_WAVES;    // items per block iteration
constexpr int TK_CAP = 256;             // candidate slots per query
constexpr int TK_MAXS = 64;
constexpr int TK_MERGE_T = 256;
static_assert(TK_CAP >= 128 + TK_IT, "K kept + one iteration's keys must fit");

int g_topk_splits = 0;

__device__ __forceinline__ uint64_t tk_key(float s, int id) {
  uint32_t u = __float_as_uint(s + 0.f);          // -0 -> +0: equal scores, equal bits
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ((uint64_t)u << 32) | (uint32_t)~(uint32_t)id;
}
__device__ __forceinline__ float tk_score(uint64_t k) {
  uint32_t u = (uint32_t)(k >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
  return __uint_as_float(u);
}
__device__ __forceinline__ int tk_id(uint64_t k) { return (int)~(uint32_t)k; }

__device__ __forceinline__ void tk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int E>
struct TkFrag { float4 v[E / 16]; };

template <int E>
__device__ __forceinline__ TkFrag<E> tk_load(const float* row, int g) {
  TkFrag<E> f;
#pragma unroll
  for (int c = 0; c < E / 16; ++c) f.v[c] = *(const float4*)(row + 16 * c + 4 * g);
  return f;
}

__device__ __forceinline__ f32x4_t tk_mfma(float a, float b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// D[row 4 g + r][col] = A row (4 g + r) . B row col, in register r
template <int E>
__device__ __forceinline__ f32x4_t tk_dot(const TkFrag<E>& a, const TkFrag<E>& b) {
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < E / 16; ++c) {
    acc = tk_mfma(a.v[c].x, b.v[c].x, acc);
    acc = tk_mfma(a.v[c].y, b.v[c].y, acc);
    acc = tk_mfma(a.v[c].z, b.v[c].z, acc);
    acc = tk_mfma(a.v[c].w, b.v[c].w, acc);
  }
  return acc;
}

struct TopkArgs {
  const float* Q; const float* W; const float* bias;
  const int64_t* excl; const int64_t* target;
  int B, V, X, K, v_lo, v_hi, S, span;
  uint64_t* part; int* cpart; float* tscore; int* excl_ge;
};

// One wave per 16 queries: tscore[b] = score(b, target[b]) (NaN for a target
// outside [0, V): nothing compares >= it) and excl_ge[b] = number of distinct
// ids x in exclude[b], v_lo <= x < v_hi, x != target[b], score(b, x) >= it.
// The wanted products are the diagonal of Q tile x gathered rows.
template <int E>
__global__ __launch_bounds__(64) void topk_target_kernel(TopkArgs a) {
  const int lane = threadIdx.x, col = lane & 15, g = lane >> 4;
  const int qc = blockIdx.x * 16 + col;
  const bool valid = qc < a.B;
  const int qr = valid ? qc : a.B - 1;
  const bool diag = g == (col >> 2);
  const int src = 16 * (col >> 2) + col, r = col & 3;
  const TkFrag<E> qa = tk_load<E>(a.Q + (int64_t)qr * E, g);
  const int64_t tg = valid ? a.target[qc] : -1;
  const bool tok = tg >= 0 && tg < a.V;
  float ts;
  {
    const int64_t row = tok ? tg : 0;
    const f32x4_t acc = tk_dot<E>(qa, tk_load<E>(a.W + row * E, g));
    float s = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    s += a.bias ? a.bias[row] : 0.f;
    ts = __shfl(tok ? s : __builtin_nanf(""), src, 64);
  }
  if (diag && valid) a.tscore[qc] = ts;
  int ge = 0;
  const int64_t* ex = a.excl + (int64_t)qr * a.X;
  for (int j = 0; j < a.X; ++j) {
    const int64_t x = valid ? ex[j] : -1;
    const bool xin = x >= a.v_lo && x < a.v_hi && x != tg;
    const int64_t row = xin ? x : 0;
    const f32x4_t acc = tk_dot<E>(qa, tk_load<E>(a.W + row * E, g));
    float s = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    s += a.bias ? a.bias[row] : 0.f;
    const int need = __shfl((int)(xin && s >= ts), src, 64);
    if (__ballot(need) == 0) continue;
    // first occurrence only: the 4 lanes of a column split the entries before j
    int dup = 0;
    if (need)
      for (int jj = g; jj < j; jj += 4) dup |= ex[jj] == x;
    dup |= __shfl_xor(dup, 16, 64);
    dup |= __shfl_xor(dup, 32, 64);
    if (diag && need && !dup) ++ge;
  }
  if (diag && valid) a.excl_ge[qc] = ge;
}

// Query row ql's candidates into registers (4 per lane), excluded ids zeroed.
__device__ __forceinline__ int tk_take(const TopkArgs& a, const uint64_t* bq, int n, int qg,
                                       int lane, uint64_t (&e)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = lane + 64 * i < n ? bq[lane + 64 * i] : 0;
  if (a.X > 0) {
    const int64_t* ex = a.excl + (int64_t)qg * a.X;
    for (int j = 0; j < a.X; ++j) {
      const int64_t x = ex[j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((int64_t)tk_id(e[i]) == x) e[i] = 0;
    }
  }
  int m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) m += __popcll(__ballot(e[i] != 0));
  return m;
}

// Wave-level compaction of a full candidate buffer: excluded ids dropped, the
// K-th largest key found by a bitwise binary search on ballot counts (keys are
// distinct), the K keys >= it kept in any order, the threshold raised to it
// (or, with no tie at the K-th score, to that score with id bits 0: a lower
// bound that admits the same keys).
__device__ __forceinline__ void tk_select(const TopkArgs& a, uint64_t* buf, uint64_t* thr,
                                          float* thrf, int* cnt, int ql, int qg, int lane) {
  uint64_t* bq = buf + ql * TK_CAP;
  const int n = cnt[ql] < TK_CAP ? cnt[ql] : TK_CAP;
  uint64_t e[4];
  const int m = tk_take(a, bq, n, qg, lane, e);
  // the K-th largest key: its score word first, the id word only among ties
  // of that score (32-bit compares; the id search is rare on real scores)
  uint64_t T = 0;
  if (m >= a.K) {
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { hi[i] = (uint32_t)(e[i] >> 32); lo[i] = (uint32_t)e[i]; }
    uint32_t T1 = 0, T2 = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t c = T1 | (1u << bit);
      int ge = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) ge += __popcll(__ballot(hi[i] >= c));
      if (ge >= a.K) T1 = c;
    }
    int gt = 0, ge = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gt += __popcll(__ballot(hi[i] > T1));
      ge += __popcll(__ballot(hi[i] >= T1));
    }
    if (ge > a.K) {
      const int need = a.K - gt;
      for (int bit = 31; bit >= 0; --bit) {
        const uint32_t c = T2 | (1u << bit);
        int n2 = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) n2 += __popcll(__ballot(hi[i] == T1 && lo[i] >= c));
        if (n2 >= need) T2 = c;
      }
    }
    T = ((uint64_t)T1 << 32) | T2;
  }
  tk_wave_sync();
  int base = 0;
  const uint64_t below = (1ull << lane) - 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool keep = e[i] != 0 && e[i] >= T;
    const uint64_t mask = __ballot(keep);
    if (keep) bq[base + __popcll(mask & below)] = e[i];
    base += __popcll(mask);
  }
  if (lane == 0) {
    cnt[ql] = base;
    if (m >= a.K) {
      thr[ql] = T;
      thrf[ql] = tk_score(T);
    }
  }
}

// The end of a block's scan: the (<= K) best of the buffer, sorted (every key
// ranked against the buffer), to part[qg][split][0..K), zeros after them.
__device__ __forceinline__ void tk_final(const TopkArgs& a, uint64_t* buf, int* cnt, int ql,
                                         int qg, int split, int lane) {
  uint64_t* bq = buf + ql * TK_CAP;
  const int n = cnt[ql] < TK_CAP ? cnt[ql] : TK_CAP;
  uint64_t e[4];
  const int m = tk_take(a, bq, n, qg, lane, e);
  tk_wave_sync();
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (lane + 64 * i < n) bq[lane + 64 * i] = e[i];
  tk_wave_sync();
  int rk[4] = {0, 0, 0, 0};
#pragma unroll 4
  for (int j = 0; j < n; ++j) {
    const uint64_t kj = bq[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) rk[i] += kj > e[i];
  }
  const int keep = m < a.K ? m : a.K;
  uint64_t* out = a.part + ((int64_t)qg * a.S + split) * a.K;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (e[i] != 0 && rk[i] < a.K) out[rk[i]] = e[i];
  for (int i = keep + lane; i < a.K; i += 64) out[i] = 0;
}

template <int E, bool HAS_T>
__global__ __launch_bounds__(64 * TK_WAVES) void topk_scan_kernel(TopkArgs a) {
  constexpr int TK_NT = tk_nt(E), TK_QT = tk_qt(E);
  constexpr bool WIDE = E > 64;
  extern __shared__ __attribute__((aligned(16))) char tk_smem[];
  uint64_t* buf = (uint64_t*)tk_smem;          // [TK_QT][TK_CAP]
  uint64_t* thr = buf + TK_QT * TK_CAP;        // [TK_QT]
  int* cnt = (int*)(thr + TK_QT);              // [TK_QT]
  int* rcnt = cnt + TK_QT;                     // [TK_QT]
  float* thrf = (float*)(rcnt + TK_QT);        // [TK_QT] score of thr: the cheap first test
  int* ovf = (int*)(thrf + TK_QT);             // [2] "a key found its buffer full", by iteration parity
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, col = lane & 15, g = lane >> 4;
  const int nqt = (a.B + TK_QT - 1) / TK_QT;
  // blocks of one V range on one XCD, next to each other: they share its L2
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int split = L / nqt, q0 = (L - split * nqt) * TK_QT;
  if (t < TK_QT) {
    thr[t] = 0; cnt[t] = 0; rcnt[t] = 0;
    thrf[t] = q0 + t < a.B ? -INFINITY : INFINITY;      // rows past B take nothing
  }
  if (t < 2) ovf[t] = 0;

  TkFrag<E> qa[TK_NT];
#pragma unroll
  for (int tt = 0; tt < TK_NT; ++tt) {
    const int q = q0 + 16 * tt + col;
    qa[tt] = tk_load<E>(a.Q + (int64_t)(q < a.B ? q : a.B - 1) * E, g);
  }
  float ts[TK_NT][4];
  int ahead[TK_NT][4];
#pragma unroll
  for (int tt = 0; tt < TK_NT; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 16 * tt + 4 * g + r;
      ahead[tt][r] = 0;
      ts[tt][r] = (HAS_T && q < a.B) ? a.tscore[q] : 0.f;
    }
  const int64_t vb64 = (int64_t)a.v_lo + (int64_t)split * a.span;
  const int vbeg = (int)(vb64 < a.v_hi ? vb64 : a.v_hi);
  const int vend = (int)(vb64 + a.span < a.v_hi ? vb64 + a.span : a.v_hi);
  __syncthreads();

  // item rows PF block iterations ahead, in registers (6 ahead measured no
  // faster than 1: profiles/retrieval.md; kept small for registers)
  constexpr int PF = E == 16 ? 2 : 1;
  TkFrag<WIDE ? 16 : E> wq[PF];
  float bq[PF];
  // wide E: an item row does not wait whole in registers. It comes in groups
  // of TK_GC chunks through a ring of two; the last group of a row is
  // multiplied while the first group of the wave's next row loads into wg[0]
  // (the number of groups is even), wrow = the row the ring is reading.
  constexpr int NG = E / 16 / TK_GC;
  static_assert(!WIDE || (NG >= 2 && NG % 2 == 0 && PF == 1), "ring of two groups");
  float4 wg[2][TK_GC];
  const float* wrow = a.W;
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    bq[u] = 0.f;
    const int v = vbeg + u * TK_IT + 16 * w + col;
    if (vbeg + u * TK_IT < vend) {
      const int vr = v < vend ? v : vend - 1;
      if constexpr (WIDE) {
        wrow = a.W + (int64_t)vr * E + 4 * g;
#pragma unroll
        for (int cc = 0; cc < TK_GC; ++cc) wg[0][cc] = *(const float4*)(wrow + 16 * cc);
      } else {
        wq[u] = tk_load<E>(a.W + (int64_t)vr * E, g);
      }
      bq[u] = v < vend ? (a.bias ? a.bias[vr] : 0.f) : __builtin_nanf("");
    }
  }
  int it = 0;
  for (int vb0 = vbeg; vb0 < vend; vb0 += PF * TK_IT)
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const int vb = vb0 + u * TK_IT;
    if (vb >= vend) break;
    const int v = vb + 16 * w + col;
    const float bv = bq[u];
    f32x4_t acc[TK_NT];
#pragma unroll
    for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if constexpr (WIDE) {
      const bool more = vb + TK_IT < vend;
      const int v2 = v + TK_IT;
      const int vr2 = v2 < vend ? v2 : vend - 1;     // (read only if more)
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        if (gi + 1 < NG) {
#pragma unroll
          for (int cc = 0; cc < TK_GC; ++cc)
            wg[(gi + 1) & 1][cc] = *(const float4*)(wrow + 16 * (TK_GC * (gi + 1) + cc));
        } else if (more) {
          wrow = a.W + (int64_t)vr2 * E + 4 * g;
#pragma unroll
          for (int cc = 0; cc < TK_GC; ++cc) wg[0][cc] = *(const float4*)(wrow + 16 * cc);
          bq[0] = v2 < vend ? (a.bias ? a.bias[vr2] : 0.f) : __builtin_nanf("");
        }
        // the loads stay a whole group (16 MFMA steps per tile) ahead of their use
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int cc = 0; cc < TK_GC; ++cc) {
          const int c = TK_GC * gi + cc;
          const float4 wv = wg[gi & 1][cc];
#pragma unroll
          for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = tk_mfma(qa[tt].v[c].x, wv.x, acc[tt]);
#pragma unroll
          for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = tk_mfma(qa[tt].v[c].y, wv.y, acc[tt]);
#pragma unroll
          for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = tk_mfma(qa[tt].v[c].z, wv.z, acc[tt]);
#pragma unroll
          for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = tk_mfma(qa[tt].v[c].w, wv.w, acc[tt]);
        }
      }
    } else {
      const TkFrag<E> wb = wq[u];
      if (vb + PF * TK_IT < vend) {
        const int v2 = v + PF * TK_IT;
        const int vr = v2 < vend ? v2 : vend - 1;
        wq[u] = tk_load<E>(a.W + (int64_t)vr * E, g);
        bq[u] = v2 < vend ? (a.bias ? a.bias[vr] : 0.f) : __builtin_nanf("");
      }
#pragma unroll
      for (int c = 0; c < E / 16; ++c) {
#pragma unroll
        for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = tk_mfma(qa[tt].v[c].x, wb.v[c].x, acc[tt]);
#pragma unroll
        for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = tk_mfma(qa[tt].v[c].y, wb.v[c].y, acc[tt]);
#pragma unroll
        for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = tk_mfma(qa[tt].v[c].z, wb.v[c].z, acc[tt]);
#pragma unroll
        for (int tt = 0; tt < TK_NT; ++tt) acc[tt] = tk_mfma(qa[tt].v[c].w, wb.v[c].w, acc[tt]);
      }
    }
    __syncthreads();                            // the previous iteration's compactions are done
    // A score first meets its row's threshold score (one compare; an item
    // past the range has a NaN bias and meets nothing). Where any lane of the
    // wave passes, the exact 64-bit key test and the append follow. A key that
    // finds its buffer full waits (pend) for the compaction below.
    float thf[4 * TK_NT];
#pragma unroll
    for (int i = 0; i < 4 * TK_NT; ++i) thf[i] = thrf[16 * (i >> 2) + 4 * g + (i & 3)];
    uint32_t pend = 0;
#pragma unroll
    for (int i = 0; i < 4 * TK_NT; ++i) {
      const int ql = 16 * (i >> 2) + 4 * g + (i & 3);
      const float s = acc[i >> 2][i & 3] + bv;
      if (HAS_T) ahead[i >> 2][i & 3] += s >= ts[i >> 2][i & 3];   // (the target too: the merge takes it off)
      const bool c = s >= thf[i];
      if (__ballot(c) != 0) {
        if (c) {
          const uint64_t key = tk_key(s, v);
          if (key > thr[ql]) {
            const int p = atomicAdd(&cnt[ql], 1);
            if (p < TK_CAP) buf[ql * TK_CAP + p] = key;
            else pend |= 1u << i;
          }
        }
      }
    }
    if (pend) ovf[it & 1] = 1;
    __syncthreads();
    if (ovf[it & 1]) {                          // (block-uniform)
      for (int ql = w; ql < TK_QT; ql += TK_WAVES)
        if (cnt[ql] >= TK_CAP) tk_select(a, buf, thr, thrf, cnt, ql, q0 + ql, lane);
      __syncthreads();
      // K kept + one iteration's keys fit: nothing waits twice
#pragma unroll
      for (int i = 0; i < 4 * TK_NT; ++i)
        if (pend & (1u << i)) {
          const int ql = 16 * (i >> 2) + 4 * g + (i & 3);
          const uint64_t key = tk_key(acc[i >> 2][i & 3] + bv, v);
          if (key > thr[ql]) {
            const int p = atomicAdd(&cnt[ql], 1);
            if (p < TK_CAP) buf[ql * TK_CAP + p] = key;
          }
        }
    }
    // the other parity's flag: read by every wave before this iteration's
    // barriers, written next after the next iteration's first one
    if (t == 0) ovf[(it + 1) & 1] = 0;
    ++it;
  }
  __syncthreads();
  for (int ql = w; ql < TK_QT; ql += TK_WAVES)
    if (q0 + ql < a.B) tk_final(a, buf, cnt, ql, q0 + ql, split, lane);
  if (HAS_T) {
#pragma unroll
    for (int tt = 0; tt < TK_NT; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int c = ahead[tt][r];
        c += __shfl_xor(c, 1, 64);
        c += __shfl_xor(c, 2, 64);
        c += __shfl_xor(c, 4, 64);
        c += __shfl_xor(c, 8, 64);
        if (col == 0 && c) atomicAdd(&rcnt[16 * tt + 4 * g + r], c);
      }
    __syncthreads();
    if (t < TK_QT && q0 + t < a.B) a.cpart[(int64_t)split * a.B + q0 + t] = rcnt[t];
  }
}

__global__ __launch_bounds__(TK_MERGE_T) void topk_merge_kernel(
    const uint64_t* __restrict__ part, const int* __restrict__ cpart,
    const int* __restrict__ excl_ge, const int64_t* __restrict__ target,
    const float* __restrict__ tscore, int v_lo, int v_hi, int B, int S, int K,
    int64_t* __restrict__ ids, float* __restrict__ scores, int64_t* __restrict__ rank) {
  extern __shared__ __attribute__((aligned(16))) char tk_smem[];
  const int n = S * K;
  uint64_t* keys = (uint64_t*)tk_smem;            // [S][K]
  unsigned long long& floor_key = *(unsigned long long*)(keys + n);
  int* live = (int*)(keys + n + 1);               // [n]
  int& nlive = live[n];
  const int t = threadIdx.x, q = blockIdx.x;
  const uint64_t* pq = part + (int64_t)q * n;
  if (t == 0) { nlive = 0; floor_key = ~0ull; }
  for (int i = t; i < n; i += TK_MERGE_T) keys[i] = pq[i];
  for (int i = t; i < K; i += TK_MERGE_T) {
    ids[(int64_t)q * K + i] = -1;
    scores[(int64_t)q * K + i] = -INFINITY;
  }
  __syncthreads();
  // >= K keys are >= min_s keys[s][c - 1], c = ceil(K / S): smaller ones are out
  const int c = (K + S - 1) / S;
  if (t < S) atomicMin(&floor_key, (unsigned long long)keys[t * K + c - 1]);
  __syncthreads();
  const uint64_t fl = floor_key;
  for (int i = t; i < n; i += TK_MERGE_T)
    if (keys[i] != 0 && keys[i] >= fl) live[atomicAdd(&nlive, 1)] = i;
  __syncthreads();
  const int nl = nlive;
  for (int u = t; u < nl; u += TK_MERGE_T) {
    const uint64_t key = keys[live[u]];
    int r = 0;
    for (int s = 0; s < S && r < K; ++s) {
      const uint64_t* ls = keys + s * K;          // descending, zeros last
      int lo = 0, hi = K;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ls[mid] > key) lo = mid + 1; else hi = mid;
      }
      r += lo;
    }
    if (r < K) {
      ids[(int64_t)q * K + r] = tk_id(key);
      scores[(int64_t)q * K + r] = tk_score(key);
    }
  }
  if (rank != nullptr && t == 0) {
    int64_t cnum = 0;
    for (int s = 0; s < S; ++s) cnum += cpart[(int64_t)s * B + q];
    // the scan counted every in-range item scoring >= the target: the target
    // itself among them when it is in range (and its score is no NaN)
    const int64_t tq = target[q];
    const float tsq = tscore[q];
    const int self = tq >= v_lo && tq < v_hi && tsq == tsq;
    rank[q] = cnum - excl_ge[q] - self;
  }
}

}  // namespace

int topk_splits(int n) {
  const int old = g_topk_splits;
  if (n >= 0) g_topk_splits = n;
  return old;
}

bool topk_width_ok(int E) { return E == 16 || E == 32 || E == 64 || E == 128 || E == 256; }

TopkPlan topk_plan(int B, int E, int v_lo, int v_hi) {
  const int64_t tiles = ((int64_t)v_hi - v_lo + TK_IT - 1) / TK_IT;
  const int qt = tk_qt(E);
  const int nqt = (B + qt - 1) / qt;
  int64_t S = g_topk_splits > 0 ? g_topk_splits : (256 + nqt - 1) / (nqt < 1 ? 1 : nqt);
  if (S > TK_MAXS) S = TK_MAXS;
  if (S > tiles) S = tiles;
  if (S < 1) S = 1;
  const int64_t per = tiles > 0 ? (tiles + S - 1) / S : 1;
  TopkPlan p;
  p.span = (int)(per * TK_IT);
  p.S = tiles > 0 ? (int)((tiles + per - 1) / per) : 1;
  return p;
}

void topk_scores(const float* Q, const float* W, const float* bias, const int64_t* exclude,
                 const int64_t* target, int B, int V, int E, int X, int K, int v_lo, int v_hi,
                 const TopkPlan& plan, uint64_t* part, int* cpart, float* tscore, int* excl_ge,
                 int64_t* ids, float* scores, int64_t* rank, hipStream_t s) {
  if (B <= 0) return;
  if (K < 1 || K > 128) throw std::runtime_error("topk_scores: 1 <= K <= 128");
  if (V < 1 || v_lo < 0 || v_lo > v_hi || v_hi > V)
    throw std::runtime_error("topk_scores: 0 <= v_lo <= v_hi <= V, V >= 1");
  if (plan.S < 1 || plan.S > TK_MAXS || plan.span < TK_IT || plan.span % TK_IT != 0 ||
      (int64_t)plan.S * plan.span < (int64_t)v_hi - v_lo)
    throw std::runtime_error("topk_scores: bad split plan");
  TopkArgs a{Q, W, bias, X > 0 ? exclude : nullptr, target, B, V, X > 0 ? X : 0, K, v_lo, v_hi,
             plan.S, plan.span, part, cpart, tscore, excl_ge};
  if (!topk_width_ok(E)) throw std::runtime_error(TDFO_TOPK_WIDTHS_MSG);
  const int qt = tk_qt(E), nqt = (B + qt - 1) / qt;
  const size_t sm = (size_t)qt * TK_CAP * 8 + qt * (8 + 4 + 4 + 4) + 16;
  const size_t msm = (size_t)plan.S * K * (8 + 4) + 16;
  const bool has_t = target != nullptr;
#define TDFO_TK(EE)                                                                          \
  {                                                                                          \
    static bool attr = false;                                                                \
    if (!attr) {                                                                             \
      TDFO_CHECK_HIP(hipFuncSetAttribute((const void*)topk_scan_kernel<EE, false>,           \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm)); \
      TDFO_CHECK_HIP(hipFuncSetAttribute((const void*)topk_scan_kernel<EE, true>,            \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm)); \
      attr = true;                                                                           \
    }                                                                                        \
    if (has_t) {                                                                             \
      hipLaunchKernelGGL(topk_target_kernel<EE>, dim3((B + 15) / 16), dim3(64), 0, s, a);    \
      hipLaunchKernelGGL((topk_scan_kernel<EE, true>), dim3(nqt * plan.S),                   \
                         dim3(64 * TK_WAVES), sm, s, a);                                     \
    } else {                                                                                 \
      hipLaunchKernelGGL((topk_scan_kernel<EE, false>), dim3(nqt * plan.S),                  \
                         dim3(64 * TK_WAVES), sm, s, a);                                     \
    }                                                                                        \
  }
  switch (E) {
    case 16: TDFO_TK(16); break;
    case 32: TDFO_TK(32); break;
    case 64: TDFO_TK(64); break;
    case 128: TDFO_TK(128); break;
    case 256: TDFO_TK(256); break;
    default: throw std::runtime_error(TDFO_TOPK_WIDTHS_MSG);
  }
#undef TDFO_TK
  TDFO_CHECK_HIP(hipGetLastError());
  {
    static bool attr = false;
    if (!attr) {
      TDFO_CHECK_HIP(hipFuncSetAttribute((const void*)topk_merge_kernel,
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         TK_MAXS * 128 * (8 + 4) + 16));
      attr = true;
    }
  }
  hipLaunchKernelGGL(topk_merge_kernel, dim3(B), dim3(TK_MERGE_T), msm, s, part, cpart, excl_ge,
                     target, tscore, v_lo, v_hi, B, plan.S, K, ids, scores,
                     has_t ? rank : nullptr);
  TDFO_CHECK_HIP(hipGetLastError());
}

}  // namespace tdfo

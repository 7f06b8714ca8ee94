// Fused output projection + label-smoothed cross-entropy for hidden widths 32
// and 64 (Bert4Rec at the published hidden size 64; linear_xent.hip and its
// MFMA kernels are built around E = 16). Same contract, same maths, no
// [tokens, V] logits:
//   compact : valid tokens (label != ignore) -> idx[], n_valid (device)
//   pass1   : grid (vocab split s, 64-token chunk), one wave, lane = token;
//             W rows are wave-uniform (scalar loads). Online softmax over the
//             split: part[token][s] = (m, sum, O = sum_v e^{z_v - m} W_v);
//             chunk 0 also emits sum_v W_v, sum_v b_v of the split
//   merge   : one wave per valid token, lane = hidden dim: the splits are
//             combined in order (deterministic) -> lse, loss,
//             dH = scale * (E_p[W] - (1-eps) W_y - eps/V sum_v W_v)
//   wgrad   : one thread per vocab row, tokens wave-uniform:
//             dz = scale * (e^{z - lse} - eps/V - (1-eps)[v == y]),
//             dW_v = sum_n dz H_n, db_v = sum_n dz (no atomics)
//   loss    : mean over the valid tokens in a fixed tree (+ fp64 running sum)
// With a fused optimizer step the flat optimizer's kernel runs on W and bias
// right after wgrad, as linear_xent.hip's VALU path does.
#include "tdfo_common.h"
#include "tdfo_kernels.h"

#include <algorithm>

namespace tdfo {
namespace {

template <int E>
__global__ __launch_bounds__(1024) void xw_compact_kernel(const int64_t* __restrict__ labels,
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
#pragma unroll
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

template <int E>
__global__ __launch_bounds__(64) void xw_pass1_kernel(const float* __restrict__ H,
                                                      const float* __restrict__ W,
                                                      const float* __restrict__ bias, int64_t V,
                                                      int64_t VS, int S,
                                                      const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ count,
                                                      float* __restrict__ part,
                                                      float* __restrict__ wpart) {
  constexpr int XP = E + 4;             // partial record: m, sum, O[E], pad
  const int s = blockIdx.x, chunk = blockIdx.y, t = threadIdx.x;
  const int nv = *count;
  const int64_t v0 = (int64_t)s * VS, v1 = min(V, v0 + VS);
  if (chunk == 0) {                     // column sums of [W | b] over this split
    for (int c = t; c <= E; c += 64) {
      float a = 0.f;
      if (c < E)
        for (int64_t r = v0; r < v1; ++r) a += W[r * E + c];
      else
        for (int64_t r = v0; r < v1; ++r) a += bias[r];
      wpart[(int64_t)s * (E + 1) + c] = a;
    }
  }
  if (chunk * 64 >= nv) return;
  const int j = chunk * 64 + t;
  const bool valid = j < nv;
  float h[E];
  const float* hr = H + (int64_t)idx[valid ? j : 0] * E;
#pragma unroll
  for (int k = 0; k < E; k += 4) {
    const float4 q = *(const float4*)(hr + k);
    h[k] = q.x; h[k + 1] = q.y; h[k + 2] = q.z; h[k + 3] = q.w;
  }
  float m = -INFINITY, sum = 0.f, acc[E];
#pragma unroll
  for (int k = 0; k < E; ++k) acc[k] = 0.f;
  for (int64_t r = v0; r < v1; ++r) {
    const float* wr = W + r * E;        // uniform -> scalar loads
    float z = bias[r];
#pragma unroll
    for (int k = 0; k < E; ++k) z = fmaf(wr[k], h[k], z);
    if (z > m) {
      const float c = __expf(m - z);
      sum *= c;
#pragma unroll
      for (int k = 0; k < E; ++k) acc[k] *= c;
      m = z;
    }
    const float e = __expf(z - m);
    sum += e;
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = fmaf(e, wr[k], acc[k]);
  }
  if (valid) {
    float* p = part + ((int64_t)j * S + s) * XP;
    p[0] = m;
    p[1] = sum;
#pragma unroll
    for (int k = 0; k < E; k += 4)
      *(float4*)(p + 4 + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
  }
}

// one wave per valid token; lane k owns hidden dims k, k + 64, ... (< E)
template <int E>
__global__ __launch_bounds__(64) void xw_merge_kernel(const float* __restrict__ H,
                                                      const float* __restrict__ W,
                                                      const float* __restrict__ bias,
                                                      const int64_t* __restrict__ labels,
                                                      int64_t V, int S, float eps,
                                                      const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ count,
                                                      const float* __restrict__ part,
                                                      const float* __restrict__ wpart,
                                                      float* __restrict__ lse_out,
                                                      float* __restrict__ dH,
                                                      float* __restrict__ lossv) {
  constexpr int XP = E + 4;
  const int lane = threadIdx.x, j = blockIdx.x;
  const int nv = *count;
  if (j >= nv) return;
  const float scale = 1.f / (float)max(1, nv);
  const float* p0 = part + (int64_t)j * S * XP;
  float mx = -INFINITY;
  for (int s = lane; s < S; s += 64) mx = fmaxf(mx, p0[(int64_t)s * XP]);
  mx = wave_max(mx);
  const bool on = lane < E;             // (E = 32: the upper half-wave idles)
  const int k = on ? lane : 0;
  float sum = 0.f, acc = 0.f, ws = 0.f, wsb = 0.f;
  for (int s = 0; s < S; ++s) {         // split order: deterministic
    const float* p = p0 + (int64_t)s * XP;
    const float c = __expf(p[0] - mx);  // (an empty split cannot occur: every split holds a row)
    sum += c * p[1];
    acc += c * p[4 + k];
    ws += wpart[(int64_t)s * (E + 1) + k];
    wsb += wpart[(int64_t)s * (E + 1) + E];
  }
  const int n = idx[j];
  int64_t y = labels[n];
  if (y < 0 || y >= V) y = 0;           // host validates; never read out of bounds
  const float hk = on ? H[(int64_t)n * E + k] : 0.f;
  const float wy = W[y * E + k];
  const float zy = bias[y] + wave_sum(on ? wy * hk : 0.f);
  const float zmean = (wsb + wave_sum(on ? ws * hk : 0.f)) / (float)V;
  const float lse = mx + __logf(sum);
  if (lane == 0) {
    lse_out[j] = lse;
    lossv[n] = lse - (1.f - eps) * zy - eps * zmean;
  }
  if (on)
    dH[(int64_t)n * E + k] = scale * (acc / sum - (1.f - eps) * wy - eps * ws / (float)V);
}

template <int E>
__global__ __launch_bounds__(256) void xw_wgrad_kernel(const float* __restrict__ H,
                                                       const float* __restrict__ W,
                                                       const float* __restrict__ bias,
                                                       const int64_t* __restrict__ labels,
                                                       int64_t V, float eps,
                                                       const int32_t* __restrict__ idx,
                                                       const int32_t* __restrict__ count,
                                                       const float* __restrict__ lse,
                                                       float* __restrict__ dW,
                                                       float* __restrict__ db) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = v < V;
  const int64_t vr = valid ? v : V - 1;
  const int nv = *count;
  const float scale = 1.f / (float)max(1, nv);
  const float off = eps / (float)V, hit = 1.f - eps;
  float w[E], g[E], gb = 0.f;
#pragma unroll
  for (int k = 0; k < E; k += 4) {
    const float4 q = *(const float4*)(W + vr * E + k);
    w[k] = q.x; w[k + 1] = q.y; w[k + 2] = q.z; w[k + 3] = q.w;
  }
  const float b = bias[vr];
#pragma unroll
  for (int k = 0; k < E; ++k) g[k] = 0.f;
  for (int j = 0; j < nv; ++j) {
    const int n = idx[j];
    const float* hr = H + (int64_t)n * E;      // uniform -> scalar loads
    const float l = lse[j];
    const int64_t y = labels[n];
    float z = b;
#pragma unroll
    for (int k = 0; k < E; ++k) z = fmaf(w[k], hr[k], z);
    float dz = __expf(z - l) - off;
    if (y == v) dz -= hit;
    dz *= scale;
    gb += dz;
#pragma unroll
    for (int k = 0; k < E; ++k) g[k] = fmaf(dz, hr[k], g[k]);
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < E; k += 4)
      *(float4*)(dW + v * E + k) = make_float4(g[k], g[k + 1], g[k + 2], g[k + 3]);
    db[v] = gb;
  }
}

// mean loss over the valid tokens, fixed reduction tree (as linear_xent.hip)
__global__ __launch_bounds__(1024) void xw_loss_kernel(const float* __restrict__ lossv, int N,
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

// ~8 waves per SIMD in pass1 (one wave per (split, 64-token chunk)); the
// number of valid tokens is device-side, so size for the capacity N
void xw_splits(int N, int64_t V, int64_t* VS, int* S) {
  const int chunks = std::max(1, (N + 63) / 64);
  const int64_t want = std::min<int64_t>(8192, std::max<int64_t>(64, 16384 / chunks));
  const int64_t vs = std::max<int64_t>(64, (V + want - 1) / want);
  *VS = vs;
  *S = (int)((V + vs - 1) / vs);
}

template <int E>
void xw_run(const LinearXentArgs& a, hipStream_t s) {
  constexpr int XP = E + 4;
  int64_t VS;
  int S;
  xw_splits(a.N, a.V, &VS, &S);
  char* ws = (char*)a.workspace;
  int32_t* idx = (int32_t*)ws;
  int32_t* count = idx + a.N;
  float* lse = (float*)(count + 16);
  float* part = lse + a.N;
  part = (float*)(((uintptr_t)part + 15) & ~(uintptr_t)15);
  float* wpart = part + (int64_t)a.N * S * XP;
  hipLaunchKernelGGL(xw_compact_kernel<E>, dim3(1), dim3(1024), 0, s, a.labels, a.N, a.ignore,
                     idx, count, a.dH, a.lossv);
  const int chunks = (a.N + 63) / 64;
  hipLaunchKernelGGL(xw_pass1_kernel<E>, dim3(S, chunks), dim3(64), 0, s, a.H, a.W, a.bias, a.V,
                     VS, S, idx, count, part, wpart);
  hipLaunchKernelGGL(xw_merge_kernel<E>, dim3(a.N), dim3(64), 0, s, a.H, a.W, a.bias, a.labels,
                     a.V, S, a.eps, idx, count, part, wpart, lse, a.dH, a.lossv);
  if (a.dW) {
    hipLaunchKernelGGL(xw_wgrad_kernel<E>, dim3((unsigned)((a.V + 255) / 256)), dim3(256), 0, s,
                       a.H, a.W, a.bias, a.labels, a.V, a.eps, idx, count, lse, a.dW, a.db);
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
    hipLaunchKernelGGL(xw_loss_kernel, dim3(1), dim3(1024), 0, s, a.lossv, a.N, count, a.loss,
                       a.loss_acc);
  TDFO_CHECK_HIP(hipGetLastError());
}

}  // namespace

size_t linear_xent_wide_workspace(int N, int64_t V, int E) {
  int64_t VS;
  int S;
  xw_splits(N, V, &VS, &S);
  // idx[N] + count (16 ints) + lse[N] + part[N][S][E + 4] + wpart[S][E + 1]
  return (size_t)(2 * N + 16) * 4 + 16 + (size_t)N * S * (E + 4) * 4 + (size_t)S * (E + 1) * 4 + 512;
}

void linear_xent_wide(const LinearXentArgs& a, int E, hipStream_t s) {
  if (a.N <= 0) return;
  if (a.V <= 0 || a.V >= (int64_t(1) << 31))
    throw std::runtime_error("linear_xent: vocab must be in [1, 2^31)");
  if (E == 32) xw_run<32>(a, s);
  else if (E == 64) xw_run<64>(a, s);
  else throw std::runtime_error("linear_xent: hidden width must be 16, 32 or 64");
}

}  // namespace tdfo

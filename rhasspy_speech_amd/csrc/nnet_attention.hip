// RestrictedAttentionComponent: time-restricted self-attention in exact FP32 on the VALU.  What a workgroup takes, what it stages
// and why the order of one element's sum is fixed: attention_plan.h.
#include <hip/hip_runtime.h>

#include "attention_plan.h"
#include "kernels.h"

namespace rs {

namespace {
constexpr int kThreads = 64 * kAttnWaves;
constexpr int kLoadsInFlight = 8;

__global__ __launch_bounds__(kThreads) void AttentionKernel(AttentionDev d, int rows) {
  extern __shared__ float lds[];
  const AttentionLaunchPlan &p = d.plan;
  const int tid = threadIdx.x;
  const int K = d.key_dim, V = d.value_dim, C = d.context, KV = K + V;
  const int in_per_head = 2 * K + V + C, out_per_head = V + (d.output_context ? C : 0);
  const int i0 = blockIdx.x * p.frames;
  const int n = min(p.frames, rows - i0);
  const int h0 = blockIdx.y * p.heads_per_block;
  const int nh = min(p.heads_per_block, d.heads - h0);
  const int reach = (C - 1) * d.stride;
  int *prow = reinterpret_cast<int *>(lds);              // frames: the physical row of every frame of the tile
  float *kv = lds + p.frames;                            // cap_rows x pitch: [key | value] of the run's rows, head after head
  float *q = kv + (size_t)p.cap_rows * p.pitch;          // frames x heads_per_block x q_pitch: [query key | query context]
  float *bb = q + (size_t)p.frames * p.heads_per_block * p.q_pitch;   // frames x heads_per_block x C: b, then c
  for (int j = tid; j < n; j += kThreads) prow[j] = d.row_map ? d.row_map[i0 + j] : i0 + j;
  __syncthreads();
  const float *src = d.src + d.col0 + (size_t)h0 * in_per_head;
  int j0 = 0;
  while (j0 < n) {
    // ---- the run: frames j0 .. j1-1, whose context rows lie inside cap_rows consecutive physical rows starting at lo - left stride
    // (the same walk in every thread; one frame always fits)
    int lo = prow[j0], hi = lo, j1 = j0 + 1;
    while (j1 < n) {
      const int r = prow[j1], nlo = min(lo, r), nhi = max(hi, r);
      if (nhi - nlo + reach + 1 > p.cap_rows) break;
      lo = nlo; hi = nhi; j1++;
    }
    const int nrun = j1 - j0, span = hi - lo + reach + 1;
    const long base = (long)lo + d.row_off - (long)d.left * d.stride;      // physical row of staged row 0
    // ---- stage: consecutive threads take consecutive floats of a row's [key | value] columns, head after head; eight loads in
    // flight per thread before the first LDS write
    const int rowlen = nh * KV, total = span * rowlen;
    for (int e0 = tid; e0 < total; e0 += kThreads * kLoadsInFlight) {
      float v[kLoadsInFlight];
      int at[kLoadsInFlight];
#pragma unroll
      for (int u = 0; u < kLoadsInFlight; u++) {
        const int e = e0 + u * kThreads;
        at[u] = -1;
        if (e < total) {
          const int r = e / rowlen, c = e - r * rowlen, hh = c / KV;
          v[u] = src[(base + r) * d.ld + (size_t)hh * in_per_head + (c - hh * KV)];
          at[u] = r * p.pitch + c;
        }
      }
#pragma unroll
      for (int u = 0; u < kLoadsInFlight; u++)
        if (at[u] >= 0) kv[at[u]] = v[u];
    }
    const int qlen = K + C, qtotal = nrun * nh * qlen;
    for (int e0 = tid; e0 < qtotal; e0 += kThreads * kLoadsInFlight) {
      float v[kLoadsInFlight];
      int at[kLoadsInFlight];
#pragma unroll
      for (int u = 0; u < kLoadsInFlight; u++) {
        const int e = e0 + u * kThreads;
        at[u] = -1;
        if (e < qtotal) {
          const int jh = e / qlen, c = e - jh * qlen, j = jh / nh, hh = jh - j * nh;
          v[u] = src[((long)prow[j0 + j] + d.row_off) * d.ld + (size_t)hh * in_per_head + KV + c];
          at[u] = jh * p.q_pitch + c;
        }
      }
#pragma unroll
      for (int u = 0; u < kLoadsInFlight; u++)
        if (at[u] >= 0) q[at[u]] = v[u];
    }
    __syncthreads();
    // ---- b[o] = key_scale <query key, key of row t + (o - left) stride> + query context[o]
    for (int t = tid; t < nrun * nh * C; t += kThreads) {
      const int jh = t / C, o = t - jh * C;
      const int j = jh / nh, hh = jh - j * nh;
      const float *qk = q + (size_t)jh * p.q_pitch;
      const float *key = kv + (size_t)(prow[j0 + j] - lo + o * d.stride) * p.pitch + hh * KV;
      float acc = 0.f;
#pragma unroll 8
      for (int k = 0; k < K; k++) acc = fmaf(qk[k], key[k], acc);
      bb[t] = __fadd_rn(__fmul_rn(d.key_scale, acc), qk[K + o]);
    }
    __syncthreads();
    // ---- c = softmax(b), the row maximum subtracted (SoftMaxPerRow)
    for (int jh = tid; jh < nrun * nh; jh += kThreads) {
      float *b = bb + (size_t)jh * C;
      float mx = b[0];
      for (int o = 1; o < C; o++) mx = fmaxf(mx, b[o]);
      float sum = 0.f;
      for (int o = 0; o < C; o++) { const float e = expf(b[o] - mx); b[o] = e; sum += e; }
      const float inv = 1.0f / sum;
      for (int o = 0; o < C; o++) b[o] = __fmul_rn(b[o], inv);
    }
    __syncthreads();
    // ---- out = [sum_o c[o] value of row t + (o - left) stride | c]
    for (int t = tid; t < nrun * nh * out_per_head; t += kThreads) {
      const int jh = t / out_per_head, col = t - jh * out_per_head;
      const int j = jh / nh, hh = jh - j * nh;
      const float *c = bb + (size_t)jh * C;
      float v;
      if (col < V) {
        const float *val = kv + (size_t)(prow[j0 + j] - lo) * p.pitch + hh * KV + K + col;
        v = 0.f;
#pragma unroll 4
        for (int o = 0; o < C; o++) v = fmaf(c[o], val[(size_t)o * d.stride * p.pitch], v);
      } else {
        v = c[col - V];
      }
      const int ocol = (h0 + hh) * out_per_head + col;
      d.out[(size_t)prow[j0 + j] * d.ldo + ocol] = v;
    }
    __syncthreads();      // (the next run stages over what this one read)
    j0 = j1;
  }
}
}  // namespace

void LaunchAttention(const AttentionDev &d, int rows, hipStream_t s) {
  if (rows <= 0) return;
  const AttentionLaunchPlan &p = d.plan;
  if (p.frames < 1 || p.heads_per_block < 1 || p.lds_bytes > kAttnMaxLdsBytes) Fail("attention kernel: no plan for this layer");
  hipLaunchKernelGGL(AttentionKernel, dim3((unsigned)AttentionGridX(p, rows), (unsigned)p.head_groups), dim3(kThreads), (size_t)p.lds_bytes, s, d, rows);
}

}  // namespace rs

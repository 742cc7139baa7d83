// The serial part of a recurrent block (nnet3's fast-lstmp-layer / fast-lstm-layer) on the exact-FP32 matrix cores.  What a
// workgroup owns, what it keeps in LDS and why a row's result does not depend on its place: lstm_plan.h.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lstm_plan.h"

namespace rs {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ScalarSigmoid / ScalarTanh as the reference writes them (cudamatrix/cu-math.cc:422-442), on the full-precision expf
__device__ __forceinline__ float LstmSigmoid(float a) {
  if (a > 0.f) return 1.f / (1.f + expf(-a));
  const float x = expf(a);
  return x / (x + 1.f);
}
__device__ __forceinline__ float LstmTanh(float a) {
  if (a > 0.f) {
    const float inv_expa = expf(-a);
    return -1.f + 2.f / (1.f + inv_expa * inv_expa);
  }
  const float expa = expf(a);
  return 1.f - 2.f / (1.f + expa * expa);
}

// per chain of the workgroup
struct LstmChain {
  int row0;        // physical row of the chain's first step; step n is row0 + n * delay
  int count;       // steps
  int ring_off;    // streams: offset of the chain's parked state row in LstmDev::ring
  int cont;        // its first step continues from the parked row (else from zeros)
  int save_step;   // the step whose state row is parked for the next advance, -1: none
};

__global__ __launch_bounds__(64 * kLstmWaves) void LstmKernel(LstmDev d) {
  extern __shared__ float lds[];
  __shared__ LstmChain chains[kLstmChains];
  __shared__ int n_steps_s;
  const LstmLaunchPlan &p = d.plan;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell, state_w = d.cell + d.rec_dim;
  const bool proj = d.rp != nullptr;
  float *const sr_tile[2] = {lds, lds + kLstmChains * p.ld_r};
  float *const m_tile = lds + 2 * kLstmChains * p.ld_r;      // (with a projection only)

  if (tid < kLstmChains) {
    const int per_utt = LstmChainsPerUtt(d.delay, d.stride), step = d.stride > 1 ? d.stride : 1;
    const int chain = blockIdx.x * kLstmChains + tid, u = chain / per_utt, c = chain - u * per_utt;
    LstmChain ch = {0, 0, 0, 0, -1};
    const int T = u < d.n_utts ? d.num_frames[u] : 0;
    if (T > 0) {
      const int t0 = d.t0 ? d.t0[u] : 0;
      ch.cont = d.slot != nullptr && t0 > 0;
      const int t_start = ch.cont ? -d.lext_cont : -d.lext, t_end = T + d.rext;
      int m = (c * step - t_start) % d.delay;      // the first t >= t_start of the chain's class, t = c * step mod delay
      if (m < 0) m += d.delay;
      const int t_first = t_start + m;
      if (t_first < t_end) ch.count = (t_end - 1 - t_first) / d.delay + 1;
      ch.row0 = d.row_base[u] + d.L + t_first;
      if (d.slot) {
        int rr = (t0 + t_first) % d.delay;
        if (rr < 0) rr += d.delay;
        ch.ring_off = (d.slot[u] * d.delay + rr) * state_w;
        const int re = T - d.lext_cont;            // where the next advance re-enters: it reads the rows [re - delay, re)
        if (re - 1 >= t_first) ch.save_step = (re - 1 - t_first) / d.delay;
      }
    }
    chains[tid] = ch;
  }
  for (int e = tid; e < kLstmChains * (2 * p.ld_r + (proj ? p.ld_m : 0)); e += 64 * kLstmWaves) lds[e] = 0.f;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < kLstmChains; i++) n = max(n, chains[i].count);
    n_steps_s = n;
  }
  // s_r of the rows before the chains' first: what an earlier advance parked, else the zeros above
  for (int e = tid; e < kLstmChains * d.rec_dim; e += 64 * kLstmWaves) {
    const int i = e / d.rec_dim, k = e - i * d.rec_dim;
    if (chains[i].count > 0 && chains[i].cont) sr_tile[0][i * p.ld_r + k] = d.ring[chains[i].ring_off + C + k];
  }
  __syncthreads();
  const int n_steps = n_steps_s;

  for (int n = 0; n < n_steps; n++) {
    const float *sr_cur = sr_tile[n & 1];
    float *sr_next = sr_tile[(n + 1) & 1];
    // ---- gates = pre[t] + W_r s_r[t - d], then the nonlinearity: a wave item is the four gates of 16 cells for the 16 chains
    for (int item = wave; item < p.cell_tiles; item += kLstmWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const LstmChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count && cell < C;
        const float *prow = d.pre + (long)(ch.row0 + n * d.delay) * d.ld_pre + cell;
#pragma unroll
        for (int g = 0; g < 4; g++) acc[g][r] = live ? prow[g * C] : 0.f;
      }
      // (a lane's four gate weights of a k are one 16-byte load; the loads of four k-steps -- k_r is a multiple of 16 -- are issued
      // before their MFMAs, which run in k order all the same)
      const float *wp = d.wr_t + (size_t)lk * p.n_gates + 4 * cell;
      for (int k0 = 0; k0 < p.k_r; k0 += 16) {
        float a[4];
        float4 w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = sr_cur[lm * p.ld_r + k0 + 4 * u + lk];
          w[u] = *reinterpret_cast<const float4 *>(wp + (size_t)(k0 + 4 * u) * p.n_gates);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].x, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].y, acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].z, acc[2], 0, 0, 0);
          acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].w, acc[3], 0, 0, 0);
        }
      }
      // (accumulator register r of lane l: chain 4 (l >> 4) + r, cell 16 item + (l & 15))
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const LstmChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float c_t = 0.f, m_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * d.delay;
          float c_prev = 0.f;
          if (n > 0) c_prev = d.st[(row - d.delay) * d.ld_st + cell];      // (this lane's own store of the step before)
          else if (ch.cont) c_prev = d.ring[ch.ring_off + cell];
          // CpuComputeLstmNonlinearity (cu-math.cc:477-481) with the three dropout scales at 1
          const float i_t = LstmSigmoid(acc[0][r] + d.params[cell] * c_prev);
          const float f_t = LstmSigmoid(acc[1][r] + d.params[C + cell] * c_prev);
          c_t = f_t * c_prev + i_t * LstmTanh(acc[2][r]);
          const float o_t = LstmSigmoid(acc[3][r] + d.params[2 * C + cell] * c_t);
          m_t = o_t * LstmTanh(c_t);
          d.cm[row * d.ld_cm + cell] = c_t;
          d.cm[row * d.ld_cm + C + cell] = m_t;
          const float s_c = __fmul_rn(c_t, d.scale);
          d.st[row * d.ld_st + cell] = s_c;
          if (n == ch.save_step) d.ring[ch.ring_off + cell] = s_c;
          if (!proj) {
            const float s_r = __fmul_rn(m_t, d.scale);
            d.st[row * d.ld_st + C + cell] = s_r;
            if (n == ch.save_step) d.ring[ch.ring_off + C + cell] = s_r;
          }
        }
        if (proj) { if (cell < p.k_m) m_tile[i * p.ld_m + cell] = m_t; }
        else if (cell < p.k_r) sr_next[i * p.ld_r + cell] = live ? __fmul_rn(m_t, d.scale) : 0.f;
      }
    }
    __syncthreads();
    // ---- rp = W_rp m + b, and its first columns, scaled, as the state's recurrent part
    if (proj) {
      for (int item = wave; item < p.out_tiles; item += kLstmWaves) {
        const int col = 16 * item + lm;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *wp = d.wrp_t + (size_t)lk * p.n_out + col;
        for (int k0 = 0; k0 < p.k_m; k0 += 16) {      // (k_m is a multiple of 16: four k-steps' operands first, then their MFMAs in k order)
          float a[4], w[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            a[u] = m_tile[lm * p.ld_m + k0 + 4 * u + lk];
            w[u] = wp[(size_t)(k0 + 4 * u) * p.n_out];
          }
#pragma unroll
          for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int i = 4 * lk + r;
          const LstmChain &ch = chains[i];
          const bool live = n < ch.count && col < d.out_dim;
          float s_r = 0.f;
          if (live) {
            const long row = ch.row0 + n * d.delay;
            const float v = __fadd_rn(acc[r], d.b_rp[col]);
            d.rp[row * d.ld_rp + col] = v;
            if (col < d.rec) {
              s_r = __fmul_rn(v, d.scale);
              d.st[row * d.ld_st + C + col] = s_r;
              if (n == ch.save_step) d.ring[ch.ring_off + C + col] = s_r;
            }
          }
          if (col < d.rec) sr_next[i * p.ld_r + col] = s_r;
        }
      }
      __syncthreads();
    }
  }
}
}  // namespace

void LaunchLstm(const LstmDev &d, hipStream_t s) {
  const int grid = LstmGridX(d.n_utts, d.delay, d.stride);
  if (grid <= 0) return;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&LstmKernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLstmMaxLdsBytes);
  if (attr != hipSuccess) Fail(std::string("recurrent block kernel: cannot reserve its LDS: ") + hipGetErrorString(attr));
  hipLaunchKernelGGL(LstmKernel, dim3((unsigned)grid), dim3(64 * kLstmWaves), (size_t)d.plan.lds_bytes, s, d);
}

}  // namespace rs

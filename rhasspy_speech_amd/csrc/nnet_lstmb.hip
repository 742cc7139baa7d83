// The serial part of an LSTM block behind a bottleneck (nnet3's lstmb-layer: two LinearComponents and a ScaleAndOffsetComponent in
// front of the LstmNonlinearityComponent) on the exact-FP32 matrix cores.  What a workgroup owns, the two phases of a step, what it
// keeps in LDS and why a row's result does not depend on its place: lstmb_plan.h.  The chains, their rows and the parked state are
// LstmKernel's (nnet_lstm.hip).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lstmb_plan.h"

namespace rs {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ScalarSigmoid / ScalarTanh as the reference writes them (cudamatrix/cu-math.cc:422-442), on the full-precision expf
__device__ __forceinline__ float LstmbSigmoid(float a) {
  if (a > 0.f) return 1.f / (1.f + expf(-a));
  const float x = expf(a);
  return x / (x + 1.f);
}
__device__ __forceinline__ float LstmbTanh(float a) {
  if (a > 0.f) {
    const float inv_expa = expf(-a);
    return -1.f + 2.f / (1.f + inv_expa * inv_expa);
  }
  const float expa = expf(a);
  return 1.f - 2.f / (1.f + expa * expa);
}

// per chain of the workgroup
struct LstmbChain {
  int row0;        // physical row of the chain's first step; step n is row0 + n * delay
  int count;       // steps
  int ring_off;    // streams: offset of the chain's parked state row in LstmbDev::ring
  int cont;        // its first step continues from the parked row (else from zeros)
  int save_step;   // the step whose state row is parked for the next advance, -1: none
};

__global__ __launch_bounds__(64 * kLstmbWaves) void LstmbKernel(LstmbDev d) {
  extern __shared__ float lds[];
  __shared__ LstmbChain chains[kLstmbChains];
  __shared__ int n_steps_s;
  const LstmbLaunchPlan &p = d.plan;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell, B = d.bottleneck, state_w = 2 * d.cell;
  float *const sm_tile = lds;
  float *const b_tile = lds + kLstmbChains * p.ld_m;

  if (tid < kLstmbChains) {
    const int per_utt = LstmChainsPerUtt(d.delay, d.stride), step = d.stride > 1 ? d.stride : 1;
    const int chain = blockIdx.x * kLstmbChains + tid, u = chain / per_utt, c = chain - u * per_utt;
    LstmbChain ch = {0, 0, 0, 0, -1};
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
  for (int e = tid; e < kLstmbChains * (p.ld_m + p.ld_b); e += 64 * kLstmbWaves) lds[e] = 0.f;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < kLstmbChains; i++) n = max(n, chains[i].count);
    n_steps_s = n;
  }
  // sm of the rows before the chains' first: what an earlier advance parked, else the zeros above
  for (int e = tid; e < kLstmbChains * C; e += 64 * kLstmbWaves) {
    const int i = e / C, k = e - i * C;
    if (chains[i].count > 0 && chains[i].cont) sm_tile[i * p.ld_m + k] = d.ring[chains[i].ring_off + C + k];
  }
  __syncthreads();
  const int n_steps = n_steps_s;

  for (int n = 0; n < n_steps; n++) {
    // ---- A: b = pre_b[t] + W_a,m sm[t - d].  A wave item is 16 columns of b for the 16 chains; a wave takes two items at a time
    // (two independent accumulators over the same sm operands), each element's sum in k order all the same
    for (int item = wave; item < p.b_tiles; item += 2 * kLstmbWaves) {
      const bool two = item + kLstmbWaves < p.b_tiles;
      const int col0 = 16 * item + lm, col1 = two ? col0 + 16 * kLstmbWaves : col0;
      f32x4 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const LstmbChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count;
        const float *prow = d.pre + (long)(ch.row0 + n * d.delay) * d.ld_pre;
        acc0[r] = live && col0 < B ? prow[col0] : 0.f;
        acc1[r] = live && two && col1 < B ? prow[col1] : 0.f;
      }
      const float *wp0 = d.wam_t + (size_t)lk * p.n_b + col0, *wp1 = d.wam_t + (size_t)lk * p.n_b + col1;
      for (int k0 = 0; k0 < p.k_m; k0 += 16) {      // (k_m is a multiple of 16: four k-steps' operands first, then their MFMAs in k order)
        float a[4], w0[4], w1[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = sm_tile[lm * p.ld_m + k0 + 4 * u + lk];
          w0[u] = wp0[(size_t)(k0 + 4 * u) * p.n_b];
          w1[u] = wp1[(size_t)(k0 + 4 * u) * p.n_b];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w0[u], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w1[u], acc1, 0, 0, 0);
        }
      }
      // (accumulator register r of lane l: chain 4 (l >> 4) + r, column 16 item + (l & 15); the columns from B up to the tile's end
      // have zero weights and no pre: zeros)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const bool live = n < chains[i].count;
        b_tile[i * p.ld_b + col0] = live ? acc0[r] : 0.f;
        if (two) b_tile[i * p.ld_b + col1] = live ? acc1[r] : 0.f;
      }
    }
    __syncthreads();
    // ---- B: g = W_b b, scale and offset, then the nonlinearity: a wave item is the four gates of 16 cells for the 16 chains
    for (int item = wave; item < p.cell_tiles; item += kLstmbWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      // (a lane's four gate weights of a k are one 16-byte load)
      const float *wp = d.wb_t + (size_t)lk * p.n_gates + 4 * cell;
      for (int k0 = 0; k0 < p.k_b; k0 += 16) {
        float a[4];
        float4 w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = b_tile[lm * p.ld_b + k0 + 4 * u + lk];
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
      float so_s[4] = {0.f, 0.f, 0.f, 0.f}, so_o[4] = {0.f, 0.f, 0.f, 0.f}, peep[3] = {0.f, 0.f, 0.f};
      if (cell < C) {
#pragma unroll
        for (int g = 0; g < 4; g++) { so_s[g] = d.so_scale[g * C + cell]; so_o[g] = d.so_offset[g * C + cell]; }
#pragma unroll
        for (int g = 0; g < 3; g++) peep[g] = d.params[g * C + cell];
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const LstmbChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float s_m = 0.f;
        if (live) {
          const long row = ch.row0 + n * d.delay;
          float c_prev = 0.f;
          if (n > 0) c_prev = d.st[(row - d.delay) * d.ld_st + cell];      // (this lane's own store of the step before)
          else if (ch.cont) c_prev = d.ring[ch.ring_off + cell];
          // ScaleAndOffsetComponent::PropagateInternal: MulColsVec, then AddVecToRows
          float g[4];
#pragma unroll
          for (int q = 0; q < 4; q++) g[q] = __fadd_rn(__fmul_rn(acc[q][r], so_s[q]), so_o[q]);
          // CpuComputeLstmNonlinearity (cu-math.cc:477-481), no dropout mask
          const float i_t = LstmbSigmoid(g[0] + peep[0] * c_prev);
          const float f_t = LstmbSigmoid(g[1] + peep[1] * c_prev);
          const float c_t = f_t * c_prev + i_t * LstmbTanh(g[2]);
          const float o_t = LstmbSigmoid(g[3] + peep[2] * c_t);
          const float m_t = o_t * LstmbTanh(c_t);
          d.cm[row * d.ld_cm + cell] = c_t;
          d.cm[row * d.ld_cm + C + cell] = m_t;
          // BackpropTruncationComponent's scale, then the descriptor's Scale() on the recurrent input: two roundings
          const float s_c = __fmul_rn(c_t, d.scale);
          s_m = __fmul_rn(__fmul_rn(m_t, d.scale), d.self_scale);
          d.st[row * d.ld_st + cell] = s_c;
          d.st[row * d.ld_st + C + cell] = s_m;
          if (n == ch.save_step) {
            d.ring[ch.ring_off + cell] = s_c;
            d.ring[ch.ring_off + C + cell] = s_m;
          }
        }
        sm_tile[i * p.ld_m + cell] = s_m;      // (cell < k_m = 16 cell_tiles; the cells from C up stay zero)
      }
    }
    __syncthreads();
  }
}
}  // namespace

void LaunchLstmb(const LstmbDev &d, hipStream_t s) {
  const int grid = LstmGridX(d.n_utts, d.delay, d.stride);
  if (grid <= 0) return;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&LstmbKernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLstmbMaxLdsBytes);
  if (attr != hipSuccess) Fail(std::string("recurrent block kernel: cannot reserve its LDS: ") + hipGetErrorString(attr));
  hipLaunchKernelGGL(LstmbKernel, dim3((unsigned)grid), dim3(64 * kLstmbWaves), (size_t)d.plan.lds_bytes, s, d);
}

}  // namespace rs

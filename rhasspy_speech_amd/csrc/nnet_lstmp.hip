// The serial part of an LSTM block in its composed form (nnet3's lstmp-layer / lstmp-batchnorm-layer / lstm-layer: four affines,
// three per-element-scale peepholes, Sigmoid / Tanh nodes, three ElementwiseProductComponents, two truncation components) on the
// exact-FP32 matrix cores.  The chains, the tiles, the LDS layout and the weight images are those of nnet_lstm.hip (lstm_plan.h);
// that kernel is left as it is, and its set-up is restated here.  What differs is the arithmetic behind the recurrent product: the
// reference evaluates one component after the other, so every product and every sum below is a rounding of its own (__fmul_rn /
// __fadd_rn: nothing is contracted), the cell is scaled BEFORE the output gate's peephole and before Tanh, and the activations are
// the SigmoidComponent's / TanhComponent's on the CPU.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lstm_plan.h"

namespace rs {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

// SigmoidComponent / TanhComponent on the CPU: VectorBase::Sigmoid / Tanh (matrix/kaldi-vector.cc:899-951), on the full-precision expf
__device__ __forceinline__ float LstmpSigmoid(float x) {
  if (x > 0.f) return 1.f / (1.f + expf(-x));
  const float ex = expf(x);
  return ex / (ex + 1.f);
}
__device__ __forceinline__ float LstmpTanh(float x) {
  if (x > 0.f) {
    const float inv_expx = expf(-x);
    return -1.f + 2.f / (1.f + inv_expx * inv_expx);
  }
  const float expx = expf(x);
  return 1.f - 2.f / (1.f + expx * expx);
}

// per chain of the workgroup
struct LstmpChain {
  int row0;        // physical row of the chain's first step; step n is row0 + n * delay
  int count;       // steps
  int ring_off;    // streams: offset of the chain's parked state row [sc | sr] in LstmDev::ring
  int cont;        // its first step continues from the parked row (else from zeros)
  int save_step;   // the step whose state row is parked for the next advance, -1: none
};

__global__ __launch_bounds__(64 * kLstmWaves) void LstmpKernel(LstmDev d) {
  extern __shared__ float lds[];
  __shared__ LstmpChain chains[kLstmChains];
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
    LstmpChain ch = {0, 0, 0, 0, -1};
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
  // sr of the rows before the chains' first: what an earlier advance parked, else the zeros above
  for (int e = tid; e < kLstmChains * d.rec_dim; e += 64 * kLstmWaves) {
    const int i = e / d.rec_dim, k = e - i * d.rec_dim;
    if (chains[i].count > 0 && chains[i].cont) sr_tile[0][i * p.ld_r + k] = d.ring[chains[i].ring_off + C + k];
  }
  __syncthreads();
  const int n_steps = n_steps_s;

  for (int n = 0; n < n_steps; n++) {
    const float *sr_cur = sr_tile[n & 1];
    float *sr_next = sr_tile[(n + 1) & 1];
    // ---- the four affines' rows, pre[t] + W_r sr[t - d], then the gates: a wave item is the four gates of 16 cells for the 16 chains
    for (int item = wave; item < p.cell_tiles; item += kLstmWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const LstmpChain &ch = chains[4 * lk + r];
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
        const LstmpChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float m_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * d.delay;
          float c_prev = 0.f;      // sc[t - d]
          if (n > 0) c_prev = d.st[(row - d.delay) * d.ld_st + cell];      // (this lane's own store of the step before)
          else if (ch.cont) c_prev = d.ring[ch.ring_off + cell];
          // i2_t / f2_t (PerElementScale), the descriptors' Sum(i1_t, i2_t) / Sum(f1_t, f2_t), the components i, f and g
          const float i_t = LstmpSigmoid(__fadd_rn(acc[0][r], __fmul_rn(d.params[cell], c_prev)));
          const float f_t = LstmpSigmoid(__fadd_rn(acc[1][r], __fmul_rn(d.params[C + cell], c_prev)));
          const float g_t = LstmpTanh(acc[2][r]);
          // c1_t, c2_t (ElementwiseProduct), Sum(c1_t, c2_t), the truncation component c: the cell the rest of the row reads is scaled
          const float sum = __fadd_rn(__fmul_rn(f_t, c_prev), __fmul_rn(i_t, g_t));
          const float sc = __fmul_rn(sum, d.scale);
          // o2_t on the current cell, Sum(o1_t, o2_t), o; h_t; m_t
          const float o_t = LstmpSigmoid(__fadd_rn(acc[3][r], __fmul_rn(d.params[2 * C + cell], sc)));
          m_t = __fmul_rn(o_t, LstmpTanh(sc));
          d.cm[row * d.ld_cm + cell] = sc;
          d.cm[row * d.ld_cm + C + cell] = m_t;
          d.st[row * d.ld_st + cell] = sc;
          if (n == ch.save_step) d.ring[ch.ring_off + cell] = sc;
          if (!proj) {
            const float s_r = __fmul_rn(m_t, d.scale_r);
            d.st[row * d.ld_st + C + cell] = s_r;
            if (n == ch.save_step) d.ring[ch.ring_off + C + cell] = s_r;
          }
        }
        if (proj) { if (cell < p.k_m) m_tile[i * p.ld_m + cell] = m_t; }
        else if (cell < p.k_r) sr_next[i * p.ld_r + cell] = live ? __fmul_rn(m_t, d.scale_r) : 0.f;
      }
    }
    __syncthreads();      // (m of every cell is in LDS before a wave reads a row of it; without a projection: sr of the next step)
    // ---- rp = W_rp m + b, and its first columns through the truncation component r as the state's recurrent part
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
          const LstmpChain &ch = chains[i];
          const bool live = n < ch.count && col < d.out_dim;
          float s_r = 0.f;
          if (live) {
            const long row = ch.row0 + n * d.delay;
            const float v = __fadd_rn(acc[r], d.b_rp[col]);
            d.rp[row * d.ld_rp + col] = v;
            if (col < d.rec) {
              s_r = __fmul_rn(v, d.scale_r);
              d.st[row * d.ld_st + C + col] = s_r;
              if (n == ch.save_step) d.ring[ch.ring_off + C + col] = s_r;
            }
          }
          if (col < d.rec) sr_next[i * p.ld_r + col] = s_r;
        }
      }
      __syncthreads();      // (sr of the next step is complete, and nobody reads this step's m any more)
    }
  }
}
}  // namespace

void LaunchLstmp(const LstmDev &d, hipStream_t s) {
  const int grid = LstmGridX(d.n_utts, d.delay, d.stride);
  if (grid <= 0) return;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&LstmpKernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLstmMaxLdsBytes);
  if (attr != hipSuccess) Fail(std::string("composed recurrent block kernel: cannot reserve its LDS: ") + hipGetErrorString(attr));
  hipLaunchKernelGGL(LstmpKernel, dim3((unsigned)grid), dim3(64 * kLstmWaves), (size_t)d.plan.lds_bytes, s, d);
}

}  // namespace rs

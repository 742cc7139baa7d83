// The serial part of a recurrent block (nnet3's fast-lstmp-layer / fast-lstm-layer) on the exact-FP32 matrix cores.  What a
// workgroup owns, what it keeps in LDS and why a row's result does not depend on its place: lstm_plan.h.  The chains, the k-loop and
// the projection phase are the ones every recurrent kernel shares (recurrent_dev.h); here is the gate phase with the nonlinearity.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lstm_plan.h"
#include "recurrent_dev.h"

namespace rs {

namespace {
__global__ __launch_bounds__(64 * kRecWaves) void LstmKernel(LstmDev d) {
  extern __shared__ float lds[];
  __shared__ RecChain chains[kRecChains];
  const LstmLaunchPlan &p = d.plan;
  const RecWalk &w = d.walk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell;
  const bool proj = d.rp != nullptr;
  float *const sr_tile[2] = {lds, lds + kRecChains * p.ld_r};
  float *const m_tile = lds + 2 * kRecChains * p.ld_r;      // (with a projection only)

  const int n_steps = RecPrologue(w, chains, lds, kRecChains * (2 * p.ld_r + (proj ? p.ld_m : 0)), sr_tile[0], p.ld_r, d.rec_dim, C);

  for (int n = 0; n < n_steps; n++) {
    const float *sr_cur = sr_tile[n & 1];
    float *sr_next = sr_tile[(n + 1) & 1];
    // ---- gates = pre[t] + W_r s_r[t - d], then the nonlinearity: a wave item is the four gates of 16 cells for the 16 chains
    for (int item = wave; item < p.cell_tiles; item += kRecWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const RecChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count && cell < C;
        const float *prow = d.pre + (long)(ch.row0 + n * w.delay) * d.ld_pre + cell;
#pragma unroll
        for (int g = 0; g < 4; g++) acc[g][r] = live ? prow[g * C] : 0.f;
      }
      // (a lane's four gate weights of a k are one 16-byte load)
      RecMfma<4>(acc, sr_cur, lm * p.ld_r + lk, d.wr_t + (size_t)lk * p.n_gates + 4 * cell, p.n_gates, p.k_r);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const RecChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float c_t = 0.f, m_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * w.delay;
          float c_prev = 0.f;
          if (n > 0) c_prev = d.st[(row - w.delay) * d.ld_st + cell];      // (this lane's own store of the step before)
          else if (ch.cont) c_prev = w.ring[ch.ring_off + cell];
          // CpuComputeLstmNonlinearity (cu-math.cc:477-481) with the three dropout scales at 1
          const float i_t = RefSigmoid(acc[0][r] + d.params[cell] * c_prev);
          const float f_t = RefSigmoid(acc[1][r] + d.params[C + cell] * c_prev);
          c_t = f_t * c_prev + i_t * RefTanh(acc[2][r]);
          const float o_t = RefSigmoid(acc[3][r] + d.params[2 * C + cell] * c_t);
          m_t = o_t * RefTanh(c_t);
          d.cm[row * d.ld_cm + cell] = c_t;
          d.cm[row * d.ld_cm + C + cell] = m_t;
          const float s_c = __fmul_rn(c_t, d.scale);
          d.st[row * d.ld_st + cell] = s_c;
          if (n == ch.save_step) w.ring[ch.ring_off + cell] = s_c;
          if (!proj) {
            const float s_r = __fmul_rn(m_t, d.scale);
            d.st[row * d.ld_st + C + cell] = s_r;
            if (n == ch.save_step) w.ring[ch.ring_off + C + cell] = s_r;
          }
        }
        if (proj) { if (cell < p.k_m) m_tile[i * p.ld_m + cell] = m_t; }
        else if (cell < p.k_r) sr_next[i * p.ld_r + cell] = live ? __fmul_rn(m_t, d.scale) : 0.f;
      }
    }
    __syncthreads();
    // ---- rp = W_rp m + b, and its first columns, scaled, as the state's recurrent part
    if (proj) {
      RecProject(chains, n, w.delay, m_tile, p.ld_m, p.k_m, d.wrp_t, p.n_out, p.out_tiles, d.b_rp, d.rp, d.ld_rp, d.out_dim, d.rec, d.scale, false,
                 d.st, d.ld_st, C, w.ring, C, sr_next, p.ld_r);
      __syncthreads();
    }
  }
}
}  // namespace

void LaunchLstm(const LstmDev &d, hipStream_t s) { RecLaunch<LstmDev, LstmKernel>(d, s); }

}  // namespace rs

// The serial part of an LSTM block in its composed form (nnet3's lstmp-layer / lstmp-batchnorm-layer / lstm-layer: four affines,
// three per-element-scale peepholes, Sigmoid / Tanh nodes, three ElementwiseProductComponents, two truncation components) on the
// exact-FP32 matrix cores.  The tiles, the LDS layout and the weight images are those of nnet_lstm.hip (lstm_plan.h); the chains, the
// k-loop and the projection phase are the ones every recurrent kernel shares (recurrent_dev.h).  What differs is the arithmetic
// behind the recurrent product: the reference evaluates one component after the other, so every product and every sum below is a
// rounding of its own (__fmul_rn / __fadd_rn: nothing is contracted), the cell is scaled BEFORE the output gate's peephole and
// before Tanh, and the activations are the SigmoidComponent's / TanhComponent's on the CPU.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lstm_plan.h"
#include "recurrent_dev.h"

namespace rs {

namespace {
__global__ __launch_bounds__(64 * kRecWaves) void LstmpKernel(LstmDev d) {
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
    // ---- the four affines' rows, pre[t] + W_r sr[t - d], then the gates: a wave item is the four gates of 16 cells for the 16 chains
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
        float m_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * w.delay;
          float c_prev = 0.f;      // sc[t - d]
          if (n > 0) c_prev = d.st[(row - w.delay) * d.ld_st + cell];      // (this lane's own store of the step before)
          else if (ch.cont) c_prev = w.ring[ch.ring_off + cell];
          // i2_t / f2_t (PerElementScale), the descriptors' Sum(i1_t, i2_t) / Sum(f1_t, f2_t), the components i, f and g
          const float i_t = RefSigmoid(__fadd_rn(acc[0][r], __fmul_rn(d.params[cell], c_prev)));
          const float f_t = RefSigmoid(__fadd_rn(acc[1][r], __fmul_rn(d.params[C + cell], c_prev)));
          const float g_t = RefTanh(acc[2][r]);
          // c1_t, c2_t (ElementwiseProduct), Sum(c1_t, c2_t), the truncation component c: the cell the rest of the row reads is scaled
          const float sum = __fadd_rn(__fmul_rn(f_t, c_prev), __fmul_rn(i_t, g_t));
          const float sc = __fmul_rn(sum, d.scale);
          // o2_t on the current cell, Sum(o1_t, o2_t), o; h_t; m_t
          const float o_t = RefSigmoid(__fadd_rn(acc[3][r], __fmul_rn(d.params[2 * C + cell], sc)));
          m_t = __fmul_rn(o_t, RefTanh(sc));
          d.cm[row * d.ld_cm + cell] = sc;
          d.cm[row * d.ld_cm + C + cell] = m_t;
          d.st[row * d.ld_st + cell] = sc;
          if (n == ch.save_step) w.ring[ch.ring_off + cell] = sc;
          if (!proj) {
            const float s_r = __fmul_rn(m_t, d.scale_r);
            d.st[row * d.ld_st + C + cell] = s_r;
            if (n == ch.save_step) w.ring[ch.ring_off + C + cell] = s_r;
          }
        }
        if (proj) { if (cell < p.k_m) m_tile[i * p.ld_m + cell] = m_t; }
        else if (cell < p.k_r) sr_next[i * p.ld_r + cell] = live ? __fmul_rn(m_t, d.scale_r) : 0.f;
      }
    }
    __syncthreads();      // (m of every cell is in LDS before a wave reads a row of it; without a projection: sr of the next step)
    // ---- rp = W_rp m + b, and its first columns through the truncation component r as the state's recurrent part
    if (proj) {
      RecProject(chains, n, w.delay, m_tile, p.ld_m, p.k_m, d.wrp_t, p.n_out, p.out_tiles, d.b_rp, d.rp, d.ld_rp, d.out_dim, d.rec, d.scale_r, false,
                 d.st, d.ld_st, C, w.ring, C, sr_next, p.ld_r);
      __syncthreads();      // (sr of the next step is complete, and nobody reads this step's m any more)
    }
  }
}
}  // namespace

void LaunchLstmp(const LstmDev &d, hipStream_t s) { RecLaunch<LstmDev, LstmpKernel>(d, s, "composed recurrent block kernel"); }

}  // namespace rs

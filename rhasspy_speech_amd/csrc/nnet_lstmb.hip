// The serial part of an LSTM block behind a bottleneck (nnet3's lstmb-layer: two LinearComponents and a ScaleAndOffsetComponent in
// front of the LstmNonlinearityComponent) on the exact-FP32 matrix cores.  What a workgroup owns, the two phases of a step, what it
// keeps in LDS and why a row's result does not depend on its place: lstmb_plan.h.  The chains and the k-loops are the ones every
// recurrent kernel shares (recurrent_dev.h); here are the two phases with the nonlinearity.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lstmb_plan.h"
#include "recurrent_dev.h"

namespace rs {

namespace {
__global__ __launch_bounds__(64 * kRecWaves) void LstmbKernel(LstmbDev d) {
  extern __shared__ float lds[];
  __shared__ RecChain chains[kRecChains];
  const LstmbLaunchPlan &p = d.plan;
  const RecWalk &w = d.walk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell, B = d.bottleneck;
  float *const sm_tile = lds;
  float *const b_tile = lds + kRecChains * p.ld_m;

  const int n_steps = RecPrologue(w, chains, lds, kRecChains * (p.ld_m + p.ld_b), sm_tile, p.ld_m, C, C);

  for (int n = 0; n < n_steps; n++) {
    // ---- A: b = pre_b[t] + W_a,m sm[t - d].  A wave item is 16 columns of b for the 16 chains; a wave takes two items at a time
    // (two independent accumulators over the same sm operands), each element's sum in k order all the same
    for (int item = wave; item < p.b_tiles; item += 2 * kRecWaves) {
      const bool two = item + kRecWaves < p.b_tiles;
      const int col0 = 16 * item + lm, col1 = two ? col0 + 16 * kRecWaves : col0;
      f32x4 acc[2];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const RecChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count;
        const float *prow = d.pre + (long)(ch.row0 + n * w.delay) * d.ld_pre;
        acc[0][r] = live && col0 < B ? prow[col0] : 0.f;
        acc[1][r] = live && two && col1 < B ? prow[col1] : 0.f;
      }
      const float *const wp[2] = {d.wam_t + (size_t)lk * p.n_b + col0, d.wam_t + (size_t)lk * p.n_b + col1};
      RecMfmaItems<2, 1>(acc, sm_tile, lm * p.ld_m + lk, wp, p.n_b, p.k_m);
      // (the columns from B up to the tile's end have zero weights and no pre: zeros)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const bool live = n < chains[i].count;
        b_tile[i * p.ld_b + col0] = live ? acc[0][r] : 0.f;
        if (two) b_tile[i * p.ld_b + col1] = live ? acc[1][r] : 0.f;
      }
    }
    __syncthreads();
    // ---- B: g = W_b b, scale and offset, then the nonlinearity: a wave item is the four gates of 16 cells for the 16 chains
    for (int item = wave; item < p.cell_tiles; item += kRecWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      // (a lane's four gate weights of a k are one 16-byte load)
      RecMfma<4>(acc, b_tile, lm * p.ld_b + lk, d.wb_t + (size_t)lk * p.n_gates + 4 * cell, p.n_gates, p.k_b);
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
        const RecChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float s_m = 0.f;
        if (live) {
          const long row = ch.row0 + n * w.delay;
          float c_prev = 0.f;
          if (n > 0) c_prev = d.st[(row - w.delay) * d.ld_st + cell];      // (this lane's own store of the step before)
          else if (ch.cont) c_prev = w.ring[ch.ring_off + cell];
          // ScaleAndOffsetComponent::PropagateInternal: MulColsVec, then AddVecToRows
          float g[4];
#pragma unroll
          for (int q = 0; q < 4; q++) g[q] = __fadd_rn(__fmul_rn(acc[q][r], so_s[q]), so_o[q]);
          // CpuComputeLstmNonlinearity (cu-math.cc:477-481), no dropout mask
          const float i_t = RefSigmoid(g[0] + peep[0] * c_prev);
          const float f_t = RefSigmoid(g[1] + peep[1] * c_prev);
          const float c_t = f_t * c_prev + i_t * RefTanh(g[2]);
          const float o_t = RefSigmoid(g[3] + peep[2] * c_t);
          const float m_t = o_t * RefTanh(c_t);
          d.cm[row * d.ld_cm + cell] = c_t;
          d.cm[row * d.ld_cm + C + cell] = m_t;
          // BackpropTruncationComponent's scale, then the descriptor's Scale() on the recurrent input: two roundings
          const float s_c = __fmul_rn(c_t, d.scale);
          s_m = __fmul_rn(__fmul_rn(m_t, d.scale), d.self_scale);
          d.st[row * d.ld_st + cell] = s_c;
          d.st[row * d.ld_st + C + cell] = s_m;
          if (n == ch.save_step) {
            w.ring[ch.ring_off + cell] = s_c;
            w.ring[ch.ring_off + C + cell] = s_m;
          }
        }
        sm_tile[i * p.ld_m + cell] = s_m;      // (cell < k_m = 16 cell_tiles; the cells from C up stay zero)
      }
    }
    __syncthreads();
  }
}
}  // namespace

void LaunchLstmb(const LstmbDev &d, hipStream_t s) { RecLaunch<LstmbDev, LstmbKernel>(d, s); }

}  // namespace rs

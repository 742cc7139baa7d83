// The serial part of a recurrent block of the output-gate projected GRU (nnet3's fast-opgru-layer / fast-norm-opgru-layer) on the
// exact-FP32 matrix cores.  What a workgroup owns, what it keeps in LDS and why a row's result does not depend on its place:
// gru_plan.h.  The chains, the k-loop and the projection and normalisation phases are the ones every recurrent kernel shares
// (recurrent_dev.h); here is the gate phase with the cell's roundings.
#include <hip/hip_runtime.h>

#include "gru_plan.h"
#include "kernels.h"
#include "recurrent_dev.h"

namespace rs {

namespace {
__global__ __launch_bounds__(64 * kRecWaves) void GruKernel(GruDev d) {
  extern __shared__ float lds[];
  __shared__ RecChain chains[kRecChains];
  const GruLaunchPlan &p = d.plan;
  const RecWalk &w = d.walk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell, R = d.rec;
  float *const s_tile[2] = {lds, lds + kRecChains * p.ld_s};
  float *const co_tile = lds + 2 * kRecChains * p.ld_s;

  const int n_steps = RecPrologue(w, chains, lds, kRecChains * (2 * p.ld_s + p.ld_c), s_tile[0], p.ld_s, R, C);

  for (int n = 0; n < n_steps; n++) {
    const float *s_cur = s_tile[n & 1];
    float *s_next = s_tile[(n + 1) & 1];
    // ---- z, o = Sigmoid(pre[t] + W_zo,s s[t - d]), then h and c: a wave item is the two gates of 16 cells for the 16 chains
    for (int item = wave; item < p.cell_tiles; item += kRecWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[2];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const RecChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count && cell < C;
        const float *prow = d.pre + (long)(ch.row0 + n * w.delay) * d.ld_pre + cell;
        acc[0][r] = live ? prow[0] : 0.f;
        acc[1][r] = live ? prow[C] : 0.f;
      }
      // (a lane's two gate weights of a k are one 8-byte load)
      RecMfma<2>(acc, s_cur, lm * p.ld_s + lk, d.ws_t + (size_t)lk * p.n_gates + 2 * cell, p.n_gates, p.k_s);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const RecChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float co = 0.f;
        if (live) {
          const long row = ch.row0 + n * w.delay;
          float c_prev = 0.f;
          if (n > 0) c_prev = d.hc[(row - w.delay) * d.ld_hc + C + cell];      // (this lane's own store of the step before)
          else if (ch.cont) c_prev = w.ring[ch.ring_off + cell];
          const float z_t = RefSigmoid(acc[0][r]), o_t = RefSigmoid(acc[1][r]);
          // OutputGruNonlinearityComponent::Propagate (nnet-combined-component.cc:1969-1982), one rounding per operation of its
          // MulColsVec, AddMat, CopyFromMat and two AddMatMatElements
          const float h_t = RefTanh(__fadd_rn(__fmul_rn(c_prev, d.w_h[cell]), d.pre[row * d.ld_pre + 2 * C + cell]));
          float c_t = __fadd_rn(h_t, __fmul_rn(-z_t, h_t));
          c_t = __fadd_rn(c_t, __fmul_rn(z_t, c_prev));
          d.hc[row * d.ld_hc + cell] = h_t;
          d.hc[row * d.ld_hc + C + cell] = c_t;
          if (n == ch.save_step) w.ring[ch.ring_off + cell] = c_t;
          co = __fmul_rn(c_t, o_t);
        }
        if (cell < p.k_c) co_tile[i * p.ld_c + cell] = co;
      }
    }
    __syncthreads();
    // ---- y = W_y (c . o) + b, and its first columns as the recurrent state: scaled here, or left for the normalisation below
    RecProject(chains, n, w.delay, co_tile, p.ld_c, p.k_c, d.wy_t, p.n_out, p.out_tiles, d.b_y, d.y, d.ld_y, d.out_dim, R, d.scale, d.norm != 0,
               d.st, d.ld_st, 0, w.ring, C, s_next, p.ld_s);
    __syncthreads();
    // ---- norm variant
    if (d.norm) {
      RecNormalize(chains, n, w.delay, s_next, p.ld_s, R, d.norm_alpha, d.scale, d.st, d.ld_st, w.ring, C);
      __syncthreads();
    }
  }
}
}  // namespace

void LaunchGru(const GruDev &d, hipStream_t s) { RecLaunch<GruDev, GruKernel>(d, s); }

}  // namespace rs

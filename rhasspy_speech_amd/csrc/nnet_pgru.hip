// The serial part of a recurrent block around a GruNonlinearityComponent (nnet3's fast-pgru-layer / fast-norm-pgru-layer /
// fast-gru-layer) on the exact-FP32 matrix cores.  What a workgroup owns, the phases of a step, what it keeps in LDS and why a
// row's result does not depend on its place: pgru_plan.h.  The chains, the k-loops and the projection and normalisation phases are
// the ones every recurrent kernel shares (recurrent_dev.h); here are the two gate phases with the cell's roundings.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pgru_plan.h"
#include "recurrent_dev.h"

namespace rs {

namespace {
__global__ __launch_bounds__(64 * kRecWaves) void PgruKernel(PgruDev d) {
  extern __shared__ float lds[];
  __shared__ RecChain chains[kRecChains];
  const PgruLaunchPlan &p = d.plan;
  const RecWalk &w = d.walk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell, R = d.rec;
  const bool proj = d.proj != 0;
  float *const s_tile[2] = {lds, lds + kRecChains * p.ld_s};
  float *const sr_tile = lds + 2 * kRecChains * p.ld_s;
  float *const c_tile = lds + 3 * kRecChains * p.ld_s;           // (with a projection only)

  // (s starts behind c in a parked row, or is all of it)
  const int n_steps = RecPrologue(w, chains, lds, kRecChains * (3 * p.ld_s + p.ld_c), s_tile[0], p.ld_s, R, proj ? C : 0);

  for (int n = 0; n < n_steps; n++) {
    const float *s_cur = s_tile[n & 1];
    float *s_next = s_tile[(n + 1) & 1];
    // ---- phase 1: r = Sigmoid(pre_r[t] + W_r,s s[t - d]) and sdotr = r . s[t - d]: a wave item is 16 columns of r for the 16 chains
    for (int item = wave; item < p.rec_tiles; item += kRecWaves) {
      const int col = 16 * item + lm;
      f32x4 acc[1];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const RecChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count && col < R;
        acc[0][r] = live ? d.pre[(long)(ch.row0 + n * w.delay) * d.ld_pre + C + col] : 0.f;
      }
      RecMfma<1>(acc, s_cur, lm * p.ld_s + lk, d.wr_t + (size_t)lk * p.n_r + col, p.n_r, p.k_s);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const bool live = n < chains[i].count && col < R;
        // AddMatMatElements(1.0, r_t, s_t1, 0.0): one rounding
        sr_tile[i * p.ld_s + col] = live ? __fmul_rn(RefSigmoid(acc[0][r]), s_cur[i * p.ld_s + col]) : 0.f;
      }
    }
    __syncthreads();
    // ---- phase 2: z = Sigmoid(pre_z[t] + W_z,s s[t - d]), h = Tanh(pre_h[t] + W_h sdotr), then c: a wave item is 16 cells
    for (int item = wave; item < p.cell_tiles; item += kRecWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[2];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const RecChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count && cell < C;
        const float *prow = d.pre + (long)(ch.row0 + n * w.delay) * d.ld_pre + cell;
        acc[0][r] = live ? prow[0] : 0.f;
        acc[1][r] = live ? prow[C + R] : 0.f;
      }
      // (a lane's z and h weights of a k are one 8-byte load; z runs over the s rows, h over the sdotr rows)
      // (the k-loop of recurrent_dev.h over two tiles: four k-steps' operands first, then their MFMAs in k order)
      const float *wp = d.wzh_t + (size_t)lk * p.n_zh + 2 * cell;
      for (int k0 = 0; k0 < p.k_s; k0 += 16) {
        float a[4], ar[4];
        float2 wzh[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = s_cur[lm * p.ld_s + k0 + 4 * u + lk];
          ar[u] = sr_tile[lm * p.ld_s + k0 + 4 * u + lk];
          wzh[u] = *reinterpret_cast<const float2 *>(wp + (size_t)(k0 + 4 * u) * p.n_zh);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], wzh[u].x, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[u], wzh[u].y, acc[1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const RecChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float c_t = 0.f, s_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * w.delay;
          float c_prev;
          if (!proj) c_prev = s_cur[i * p.ld_s + cell];      // (c[t - d] and s[t - d] are one variable)
          else if (n > 0) c_prev = d.hc[(row - w.delay) * d.ld_hc + C + cell];      // (this lane's own store of the step before)
          else c_prev = ch.cont ? w.ring[ch.ring_off + cell] : 0.f;
          const float z_t = RefSigmoid(acc[0][r]);
          // GruNonlinearityComponent::Propagate (nnet-combined-component.cc:1473-1480): Tanh, CopyFromMat and two AddMatMatElements,
          // one rounding per operation
          const float h_t = RefTanh(acc[1][r]);
          c_t = __fadd_rn(h_t, __fmul_rn(-z_t, h_t));
          c_t = __fadd_rn(c_t, __fmul_rn(z_t, c_prev));
          d.hc[row * d.ld_hc + cell] = h_t;
          d.hc[row * d.ld_hc + C + cell] = c_t;
          if (proj) {
            if (n == ch.save_step) w.ring[ch.ring_off + cell] = c_t;
          } else {
            s_t = __fmul_rn(c_t, d.scale);
            d.st[row * d.ld_st + cell] = s_t;
            if (n == ch.save_step) w.ring[ch.ring_off + cell] = s_t;
          }
        }
        if (proj) c_tile[i * p.ld_c + cell] = c_t;      // (cell < k_c = 16 cell_tiles)
        else s_next[i * p.ld_s + cell] = s_t;           // (k_s = k_c without a projection)
      }
    }
    __syncthreads();
    if (!proj) continue;
    // ---- phase 3: y = W_y c + b, and its first columns as the recurrent state: scaled here, or left for the normalisation below
    RecProject(chains, n, w.delay, c_tile, p.ld_c, p.k_c, d.wy_t, p.n_out, p.out_tiles, d.b_y, d.y, d.ld_y, d.out_dim, R, d.scale, d.norm != 0,
               d.st, d.ld_st, 0, w.ring, C, s_next, p.ld_s);
    __syncthreads();
    // ---- phase 4, norm variant
    if (d.norm) {
      RecNormalize(chains, n, w.delay, s_next, p.ld_s, R, d.norm_alpha, d.scale, d.st, d.ld_st, w.ring, C);
      __syncthreads();
    }
  }
}
}  // namespace

void LaunchPgru(const PgruDev &d, hipStream_t s) { RecLaunch<PgruDev, PgruKernel>(d, s); }

}  // namespace rs

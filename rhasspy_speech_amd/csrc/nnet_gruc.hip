// The serial part of a GRU block in its composed form -- the cell spelled out as Sigmoid / Tanh / ElementwiseProduct / NoOp nodes, as
// nnet3's gru-layer / pgru-layer / norm-pgru-layer (PgrucKernel) and opgru-layer / norm-opgru-layer (GrucKernel) emit it -- on the
// exact-FP32 matrix cores.  The descriptors, plans, weight images and LDS layouts are the fast blocks' (pgru_plan.h, gru_plan.h); the
// chains, the k-loops and the projection and normalisation phases are the ones every recurrent kernel shares (recurrent_dev.h), the
// phases and barriers those of nnet_pgru.hip and nnet_gru.hip.  What differs is the cell: y = fl(fl(h . fl(1 - z)) + fl(y[t - d] . z)),
// the roundings of the descriptor Sum(Scale(-1, z_t), Const(1)), of the two ElementwiseProductComponents y1 and y2, and of the
// Sum(y1_t, y2_t) in front of the NoOpComponent.
#include <hip/hip_runtime.h>

#include "gru_plan.h"
#include "kernels.h"
#include "pgru_plan.h"
#include "recurrent_dev.h"

namespace rs {

namespace {
// y_t of the composed cell, one rounding per reference operation: the descriptor's AddMat(-1, z_t) onto the Const(1) rows, the
// MulElements of y1 and of y2 (ElementwiseProductComponent::Propagate), the AddMat of Sum(y1_t, y2_t); the NoOpComponent copies
__device__ __forceinline__ float GrucCell(float h_t, float z_t, float y_prev) {
  const float one_minus_z = __fadd_rn(1.f, -z_t);
  return __fadd_rn(__fmul_rn(h_t, one_minus_z), __fmul_rn(y_prev, z_t));
}

// ---- the reset-gate family: gru-layer (no projection), pgru-layer, norm-pgru-layer
__global__ __launch_bounds__(64 * kRecWaves) void PgrucKernel(PgruDev d) {
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

  // (s starts behind y in a parked row, or is all of it)
  const int n_steps = RecPrologue(w, chains, lds, kRecChains * (3 * p.ld_s + p.ld_c), s_tile[0], p.ld_s, R, proj ? C : 0);

  for (int n = 0; n < n_steps; n++) {
    const float *s_cur = s_tile[n & 1];
    float *s_next = s_tile[(n + 1) & 1];
    // ---- phase 1: r = Sigmoid(pre_r[t] + W_r,s s[t - d]) and h1 = r . s[t - d]: a wave item is 16 columns of r for the 16 chains
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
        // the ElementwiseProductComponent h1: one rounding
        sr_tile[i * p.ld_s + col] = live ? __fmul_rn(RefSigmoid(acc[0][r]), s_cur[i * p.ld_s + col]) : 0.f;
      }
    }
    __syncthreads();
    // ---- phase 2: z = Sigmoid(pre_z[t] + W_z,s s[t - d]), h = Tanh(pre_h[t] + W_h h1), then y: a wave item is 16 cells
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
      // (a lane's z and h weights of a k are one 8-byte load; z runs over the s rows, h over the h1 rows)
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
        float y_t = 0.f, s_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * w.delay;
          float y_prev;
          if (!proj) y_prev = s_cur[i * p.ld_s + cell];      // (gru-layer: y2_t reads the scaled s[t - d])
          else if (n > 0) y_prev = d.hc[(row - w.delay) * d.ld_hc + C + cell];      // (this lane's own store of the step before, unscaled)
          else y_prev = ch.cont ? w.ring[ch.ring_off + cell] : 0.f;
          const float z_t = RefSigmoid(acc[0][r]);
          const float h_t = RefTanh(acc[1][r]);
          y_t = GrucCell(h_t, z_t, y_prev);
          d.hc[row * d.ld_hc + cell] = h_t;
          d.hc[row * d.ld_hc + C + cell] = y_t;
          if (proj) {
            if (n == ch.save_step) w.ring[ch.ring_off + cell] = y_t;
          } else {
            s_t = __fmul_rn(y_t, d.scale);
            d.st[row * d.ld_st + cell] = s_t;
            if (n == ch.save_step) w.ring[ch.ring_off + cell] = s_t;
          }
        }
        if (proj) c_tile[i * p.ld_c + cell] = y_t;      // (cell < k_c = 16 cell_tiles)
        else s_next[i * p.ld_s + cell] = s_t;           // (k_s = k_c without a projection)
      }
    }
    __syncthreads();
    if (!proj) continue;
    // ---- phase 3: sn = W_s.ys y + b, and its first columns as the recurrent state: scaled here, or left for the normalisation below
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

// ---- the output-gate family: opgru-layer, norm-opgru-layer
__global__ __launch_bounds__(64 * kRecWaves) void GrucKernel(GruDev d) {
  extern __shared__ float lds[];
  __shared__ RecChain chains[kRecChains];
  const GruLaunchPlan &p = d.plan;
  const RecWalk &w = d.walk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell, R = d.rec;
  float *const s_tile[2] = {lds, lds + kRecChains * p.ld_s};
  float *const yo_tile = lds + 2 * kRecChains * p.ld_s;

  const int n_steps = RecPrologue(w, chains, lds, kRecChains * (2 * p.ld_s + p.ld_c), s_tile[0], p.ld_s, R, C);

  for (int n = 0; n < n_steps; n++) {
    const float *s_cur = s_tile[n & 1];
    float *s_next = s_tile[(n + 1) & 1];
    // ---- z, o = Sigmoid(pre[t] + W_zo,s s[t - d]), then h and y: a wave item is the two gates of 16 cells for the 16 chains
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
        float yo = 0.f;
        if (live) {
          const long row = ch.row0 + n * w.delay;
          float y_prev = 0.f;
          if (n > 0) y_prev = d.hc[(row - w.delay) * d.ld_hc + C + cell];      // (this lane's own store of the step before)
          else if (ch.cont) y_prev = w.ring[ch.ring_off + cell];
          const float z_t = RefSigmoid(acc[0][r]), o_t = RefSigmoid(acc[1][r]);
          // h_t = Tanh(Sum(h_t_pre, h_t_pre2)): the per-element scale's MulColsVec, then the descriptor's AddMat
          const float h_t = RefTanh(__fadd_rn(d.pre[row * d.ld_pre + 2 * C + cell], __fmul_rn(y_prev, d.w_h[cell])));
          const float y_t = GrucCell(h_t, z_t, y_prev);
          d.hc[row * d.ld_hc + cell] = h_t;
          d.hc[row * d.ld_hc + C + cell] = y_t;
          if (n == ch.save_step) w.ring[ch.ring_off + cell] = y_t;
          yo = __fmul_rn(o_t, y_t);      // the ElementwiseProductComponent o1
        }
        if (cell < p.k_c) yo_tile[i * p.ld_c + cell] = yo;
      }
    }
    __syncthreads();
    // ---- sn = W_s.ys (o . y) + b, and its first columns as the recurrent state: scaled here, or left for the normalisation below
    RecProject(chains, n, w.delay, yo_tile, p.ld_c, p.k_c, d.wy_t, p.n_out, p.out_tiles, d.b_y, d.y, d.ld_y, d.out_dim, R, d.scale, d.norm != 0,
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

void LaunchPgruc(const PgruDev &d, hipStream_t s) { RecLaunch<PgruDev, PgrucKernel>(d, s); }
void LaunchGruc(const GruDev &d, hipStream_t s) { RecLaunch<GruDev, GrucKernel>(d, s); }

}  // namespace rs

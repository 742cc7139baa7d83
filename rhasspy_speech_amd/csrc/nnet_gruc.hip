// The serial part of a GRU block in its composed form -- the cell spelled out as Sigmoid / Tanh / ElementwiseProduct / NoOp nodes, as
// nnet3's gru-layer / pgru-layer / norm-pgru-layer (PgrucKernel) and opgru-layer / norm-opgru-layer (GrucKernel) emit it -- on the
// exact-FP32 matrix cores.  The descriptors, plans, weight images and LDS layouts are the fast blocks' (pgru_plan.h, gru_plan.h); the
// chain set-up, the phases and the barriers are those of nnet_pgru.hip and nnet_gru.hip, restated here: those kernels are left as they
// are.  What differs is the cell: y = fl(fl(h . fl(1 - z)) + fl(y[t - d] . z)), the roundings of the descriptor Sum(Scale(-1, z_t),
// Const(1)), of the two ElementwiseProductComponents y1 and y2, and of the Sum(y1_t, y2_t) in front of the NoOpComponent.
#include <hip/hip_runtime.h>

#include "gru_plan.h"
#include "kernels.h"
#include "pgru_plan.h"

namespace rs {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

// SigmoidComponent / TanhComponent on the CPU: VectorBase::Sigmoid / Tanh (matrix/kaldi-vector.cc:899-951), on the full-precision expf
__device__ __forceinline__ float GrucSigmoid(float x) {
  if (x > 0.f) return 1.f / (1.f + expf(-x));
  const float ex = expf(x);
  return ex / (ex + 1.f);
}
__device__ __forceinline__ float GrucTanh(float x) {
  if (x > 0.f) {
    const float inv_expx = expf(-x);
    return -1.f + 2.f / (1.f + inv_expx * inv_expx);
  }
  const float expx = expf(x);
  return 1.f - 2.f / (1.f + expx * expx);
}
// y_t of the composed cell, one rounding per reference operation: the descriptor's AddMat(-1, z_t) onto the Const(1) rows, the
// MulElements of y1 and of y2 (ElementwiseProductComponent::Propagate), the AddMat of Sum(y1_t, y2_t); the NoOpComponent copies
__device__ __forceinline__ float GrucCell(float h_t, float z_t, float y_prev) {
  const float one_minus_z = __fadd_rn(1.f, -z_t);
  return __fadd_rn(__fmul_rn(h_t, one_minus_z), __fmul_rn(y_prev, z_t));
}

// per chain of the workgroup
struct GrucChain {
  int row0;        // physical row of the chain's first step; step n is row0 + n * delay
  int count;       // steps
  int ring_off;    // streams: offset of the chain's parked state row ([y | s], or [s]) in the descriptor's ring
  int cont;        // its first step continues from the parked row (else from zeros)
  int save_step;   // the step whose state row is parked for the next advance, -1: none
};

// (the chain of thread `tid` of the workgroup: both descriptors carry the same geometry fields)
template <typename Dev> __device__ __forceinline__ GrucChain GrucSetUp(const Dev &d, int tid, int chains, int per_utt, int state_w) {
  const int step = d.stride > 1 ? d.stride : 1;
  const int chain = blockIdx.x * chains + tid, u = chain / per_utt, c = chain - u * per_utt;
  GrucChain ch = {0, 0, 0, 0, -1};
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
  return ch;
}

// ---- the reset-gate family: gru-layer (no projection), pgru-layer, norm-pgru-layer
__global__ __launch_bounds__(64 * kPgruWaves) void PgrucKernel(PgruDev d) {
  extern __shared__ float lds[];
  __shared__ GrucChain chains[kPgruChains];
  __shared__ int n_steps_s;
  const PgruLaunchPlan &p = d.plan;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell, R = d.rec;
  const bool proj = d.proj != 0;
  const int state_w = proj ? C + R : C, s_off = proj ? C : 0;      // a parked row, and where its s starts
  float *const s_tile[2] = {lds, lds + kPgruChains * p.ld_s};
  float *const sr_tile = lds + 2 * kPgruChains * p.ld_s;
  float *const c_tile = lds + 3 * kPgruChains * p.ld_s;           // (with a projection only)

  if (tid < kPgruChains) chains[tid] = GrucSetUp(d, tid, kPgruChains, PgruChainsPerUtt(d.delay, d.stride), state_w);
  for (int e = tid; e < kPgruChains * (3 * p.ld_s + p.ld_c); e += 64 * kPgruWaves) lds[e] = 0.f;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < kPgruChains; i++) n = max(n, chains[i].count);
    n_steps_s = n;
  }
  // s of the rows before the chains' first: what an earlier advance parked, else the zeros above
  for (int e = tid; e < kPgruChains * R; e += 64 * kPgruWaves) {
    const int i = e / R, k = e - i * R;
    if (chains[i].count > 0 && chains[i].cont) s_tile[0][i * p.ld_s + k] = d.ring[chains[i].ring_off + s_off + k];
  }
  __syncthreads();
  const int n_steps = n_steps_s;

  for (int n = 0; n < n_steps; n++) {
    const float *s_cur = s_tile[n & 1];
    float *s_next = s_tile[(n + 1) & 1];
    // ---- phase 1: r = Sigmoid(pre_r[t] + W_r,s s[t - d]) and h1 = r . s[t - d]: a wave item is 16 columns of r for the 16 chains
    for (int item = wave; item < p.rec_tiles; item += kPgruWaves) {
      const int col = 16 * item + lm;
      f32x4 acc;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const GrucChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count && col < R;
        acc[r] = live ? d.pre[(long)(ch.row0 + n * d.delay) * d.ld_pre + C + col] : 0.f;
      }
      const float *wp = d.wr_t + (size_t)lk * p.n_r + col;
      for (int k0 = 0; k0 < p.k_s; k0 += 16) {      // (k_s is a multiple of 16: four k-steps' operands first, then their MFMAs in k order)
        float a[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = s_cur[lm * p.ld_s + k0 + 4 * u + lk];
          w[u] = wp[(size_t)(k0 + 4 * u) * p.n_r];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u], acc, 0, 0, 0);
      }
      // (accumulator register r of lane l: chain 4 (l >> 4) + r, column 16 item + (l & 15))
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const bool live = n < chains[i].count && col < R;
        // the ElementwiseProductComponent h1: one rounding
        sr_tile[i * p.ld_s + col] = live ? __fmul_rn(GrucSigmoid(acc[r]), s_cur[i * p.ld_s + col]) : 0.f;
      }
    }
    __syncthreads();
    // ---- phase 2: z = Sigmoid(pre_z[t] + W_z,s s[t - d]), h = Tanh(pre_h[t] + W_h h1), then y: a wave item is 16 cells
    for (int item = wave; item < p.cell_tiles; item += kPgruWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[2];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const GrucChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count && cell < C;
        const float *prow = d.pre + (long)(ch.row0 + n * d.delay) * d.ld_pre + cell;
        acc[0][r] = live ? prow[0] : 0.f;
        acc[1][r] = live ? prow[C + R] : 0.f;
      }
      // (a lane's z and h weights of a k are one 8-byte load; z runs over the s rows, h over the h1 rows)
      const float *wp = d.wzh_t + (size_t)lk * p.n_zh + 2 * cell;
      for (int k0 = 0; k0 < p.k_s; k0 += 16) {
        float a[4], ar[4];
        float2 w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = s_cur[lm * p.ld_s + k0 + 4 * u + lk];
          ar[u] = sr_tile[lm * p.ld_s + k0 + 4 * u + lk];
          w[u] = *reinterpret_cast<const float2 *>(wp + (size_t)(k0 + 4 * u) * p.n_zh);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].x, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[u], w[u].y, acc[1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const GrucChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float y_t = 0.f, s_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * d.delay;
          float y_prev;
          if (!proj) y_prev = s_cur[i * p.ld_s + cell];      // (gru-layer: y2_t reads the scaled s[t - d])
          else if (n > 0) y_prev = d.hc[(row - d.delay) * d.ld_hc + C + cell];      // (this lane's own store of the step before, unscaled)
          else y_prev = ch.cont ? d.ring[ch.ring_off + cell] : 0.f;
          const float z_t = GrucSigmoid(acc[0][r]);
          const float h_t = GrucTanh(acc[1][r]);
          y_t = GrucCell(h_t, z_t, y_prev);
          d.hc[row * d.ld_hc + cell] = h_t;
          d.hc[row * d.ld_hc + C + cell] = y_t;
          if (proj) {
            if (n == ch.save_step) d.ring[ch.ring_off + cell] = y_t;
          } else {
            s_t = __fmul_rn(y_t, d.scale);
            d.st[row * d.ld_st + cell] = s_t;
            if (n == ch.save_step) d.ring[ch.ring_off + cell] = s_t;
          }
        }
        if (proj) c_tile[i * p.ld_c + cell] = y_t;      // (cell < k_c = 16 cell_tiles)
        else s_next[i * p.ld_s + cell] = s_t;           // (k_s = k_c without a projection)
      }
    }
    __syncthreads();
    if (!proj) continue;
    // ---- phase 3: sn = W_s.ys y + b, and its first columns as the recurrent state: scaled here, or left for the normalisation below
    for (int item = wave; item < p.out_tiles; item += kPgruWaves) {
      const int col = 16 * item + lm;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float *wp = d.wy_t + (size_t)lk * p.n_out + col;
      for (int k0 = 0; k0 < p.k_c; k0 += 16) {
        float a[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = c_tile[lm * p.ld_c + k0 + 4 * u + lk];
          w[u] = wp[(size_t)(k0 + 4 * u) * p.n_out];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const GrucChain &ch = chains[i];
        const bool live = n < ch.count && col < d.out_dim;
        float s_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * d.delay;
          const float v = __fadd_rn(acc[r], d.b_y[col]);
          d.y[row * d.ld_y + col] = v;
          if (col < R) {
            if (d.norm) {
              s_t = v;
            } else {
              s_t = __fmul_rn(v, d.scale);
              d.st[row * d.ld_st + col] = s_t;
              if (n == ch.save_step) d.ring[ch.ring_off + C + col] = s_t;
            }
          }
        }
        if (col < R) s_next[i * p.ld_s + col] = s_t;
      }
    }
    __syncthreads();
    // ---- phase 4, norm variant: NormalizePerRow (cu-math.cc:302-310) over each chain's rec columns, then the scale.  A wave takes
    // two chains; a lane sums its k = lane, lane + 64, ... in that order, the 64 partial sums meet in a fixed tree.
    if (d.norm) {
      for (int i = wave; i < kPgruChains; i += kPgruWaves) {
        const GrucChain &ch = chains[i];
        if (n >= ch.count) continue;      // (the whole wave: its row of the tile holds zeros)
        float *srow = s_next + i * p.ld_s;
        float ss = 0.f;
        for (int k = lane; k < R; k += 64) ss = __fadd_rn(ss, __fmul_rn(srow[k], srow[k]));
        for (int o = 32; o > 0; o >>= 1) ss = __fadd_rn(ss, __shfl_xor(ss, o, 64));
        float nrm = __fmul_rn(ss, d.norm_alpha);
        nrm = fmaxf(nrm, 1.3552527156068805425e-20f);      // kSquaredNormFloor, 2^-66
        nrm = powf(nrm, -0.5f);
        const long row = ch.row0 + n * d.delay;
        for (int k = lane; k < R; k += 64) {
          const float s_t = __fmul_rn(__fmul_rn(srow[k], nrm), d.scale);
          srow[k] = s_t;
          d.st[row * d.ld_st + k] = s_t;
          if (n == ch.save_step) d.ring[ch.ring_off + C + k] = s_t;
        }
      }
      __syncthreads();
    }
  }
}

// ---- the output-gate family: opgru-layer, norm-opgru-layer
__global__ __launch_bounds__(64 * kGruWaves) void GrucKernel(GruDev d) {
  extern __shared__ float lds[];
  __shared__ GrucChain chains[kGruChains];
  __shared__ int n_steps_s;
  const GruLaunchPlan &p = d.plan;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  const int C = d.cell, R = d.rec, state_w = d.cell + d.rec;
  float *const s_tile[2] = {lds, lds + kGruChains * p.ld_s};
  float *const yo_tile = lds + 2 * kGruChains * p.ld_s;

  if (tid < kGruChains) chains[tid] = GrucSetUp(d, tid, kGruChains, GruChainsPerUtt(d.delay, d.stride), state_w);
  for (int e = tid; e < kGruChains * (2 * p.ld_s + p.ld_c); e += 64 * kGruWaves) lds[e] = 0.f;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < kGruChains; i++) n = max(n, chains[i].count);
    n_steps_s = n;
  }
  // s of the rows before the chains' first: what an earlier advance parked, else the zeros above
  for (int e = tid; e < kGruChains * R; e += 64 * kGruWaves) {
    const int i = e / R, k = e - i * R;
    if (chains[i].count > 0 && chains[i].cont) s_tile[0][i * p.ld_s + k] = d.ring[chains[i].ring_off + C + k];
  }
  __syncthreads();
  const int n_steps = n_steps_s;

  for (int n = 0; n < n_steps; n++) {
    const float *s_cur = s_tile[n & 1];
    float *s_next = s_tile[(n + 1) & 1];
    // ---- z, o = Sigmoid(pre[t] + W_zo,s s[t - d]), then h and y: a wave item is the two gates of 16 cells for the 16 chains
    for (int item = wave; item < p.cell_tiles; item += kGruWaves) {
      const int cell = 16 * item + lm;
      f32x4 acc[2];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const GrucChain &ch = chains[4 * lk + r];
        const bool live = n < ch.count && cell < C;
        const float *prow = d.pre + (long)(ch.row0 + n * d.delay) * d.ld_pre + cell;
        acc[0][r] = live ? prow[0] : 0.f;
        acc[1][r] = live ? prow[C] : 0.f;
      }
      // (a lane's two gate weights of a k are one 8-byte load; the loads of four k-steps -- k_s is a multiple of 16 -- are issued
      // before their MFMAs, which run in k order all the same)
      const float *wp = d.ws_t + (size_t)lk * p.n_gates + 2 * cell;
      for (int k0 = 0; k0 < p.k_s; k0 += 16) {
        float a[4];
        float2 w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = s_cur[lm * p.ld_s + k0 + 4 * u + lk];
          w[u] = *reinterpret_cast<const float2 *>(wp + (size_t)(k0 + 4 * u) * p.n_gates);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].x, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u].y, acc[1], 0, 0, 0);
        }
      }
      // (accumulator register r of lane l: chain 4 (l >> 4) + r, cell 16 item + (l & 15))
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const GrucChain &ch = chains[i];
        const bool live = n < ch.count && cell < C;
        float yo = 0.f;
        if (live) {
          const long row = ch.row0 + n * d.delay;
          float y_prev = 0.f;
          if (n > 0) y_prev = d.hc[(row - d.delay) * d.ld_hc + C + cell];      // (this lane's own store of the step before)
          else if (ch.cont) y_prev = d.ring[ch.ring_off + cell];
          const float z_t = GrucSigmoid(acc[0][r]), o_t = GrucSigmoid(acc[1][r]);
          // h_t = Tanh(Sum(h_t_pre, h_t_pre2)): the per-element scale's MulColsVec, then the descriptor's AddMat
          const float h_t = GrucTanh(__fadd_rn(d.pre[row * d.ld_pre + 2 * C + cell], __fmul_rn(y_prev, d.w_h[cell])));
          const float y_t = GrucCell(h_t, z_t, y_prev);
          d.hc[row * d.ld_hc + cell] = h_t;
          d.hc[row * d.ld_hc + C + cell] = y_t;
          if (n == ch.save_step) d.ring[ch.ring_off + cell] = y_t;
          yo = __fmul_rn(o_t, y_t);      // the ElementwiseProductComponent o1
        }
        if (cell < p.k_c) yo_tile[i * p.ld_c + cell] = yo;
      }
    }
    __syncthreads();
    // ---- sn = W_s.ys (o . y) + b, and its first columns as the recurrent state: scaled here, or left for the normalisation below
    for (int item = wave; item < p.out_tiles; item += kGruWaves) {
      const int col = 16 * item + lm;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float *wp = d.wy_t + (size_t)lk * p.n_out + col;
      for (int k0 = 0; k0 < p.k_c; k0 += 16) {      // (k_c is a multiple of 16: four k-steps' operands first, then their MFMAs in k order)
        float a[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          a[u] = yo_tile[lm * p.ld_c + k0 + 4 * u + lk];
          w[u] = wp[(size_t)(k0 + 4 * u) * p.n_out];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i = 4 * lk + r;
        const GrucChain &ch = chains[i];
        const bool live = n < ch.count && col < d.out_dim;
        float s_t = 0.f;
        if (live) {
          const long row = ch.row0 + n * d.delay;
          const float v = __fadd_rn(acc[r], d.b_y[col]);
          d.y[row * d.ld_y + col] = v;
          if (col < R) {
            if (d.norm) {
              s_t = v;
            } else {
              s_t = __fmul_rn(v, d.scale);
              d.st[row * d.ld_st + col] = s_t;
              if (n == ch.save_step) d.ring[ch.ring_off + C + col] = s_t;
            }
          }
        }
        if (col < R) s_next[i * p.ld_s + col] = s_t;
      }
    }
    __syncthreads();
    // ---- norm variant: NormalizePerRow (cu-math.cc:302-310) over each chain's rec columns, then the scale.  A wave takes two
    // chains; a lane sums its k = lane, lane + 64, ... in that order, the 64 partial sums meet in a fixed tree.
    if (d.norm) {
      for (int i = wave; i < kGruChains; i += kGruWaves) {
        const GrucChain &ch = chains[i];
        if (n >= ch.count) continue;      // (the whole wave: its row of the tile holds zeros)
        float *srow = s_next + i * p.ld_s;
        float ss = 0.f;
        for (int k = lane; k < R; k += 64) ss = __fadd_rn(ss, __fmul_rn(srow[k], srow[k]));
        for (int o = 32; o > 0; o >>= 1) ss = __fadd_rn(ss, __shfl_xor(ss, o, 64));
        float nrm = __fmul_rn(ss, d.norm_alpha);
        nrm = fmaxf(nrm, 1.3552527156068805425e-20f);      // kSquaredNormFloor, 2^-66
        nrm = powf(nrm, -0.5f);
        const long row = ch.row0 + n * d.delay;
        for (int k = lane; k < R; k += 64) {
          const float s_t = __fmul_rn(__fmul_rn(srow[k], nrm), d.scale);
          srow[k] = s_t;
          d.st[row * d.ld_st + k] = s_t;
          if (n == ch.save_step) d.ring[ch.ring_off + C + k] = s_t;
        }
      }
      __syncthreads();
    }
  }
}
}  // namespace

void LaunchPgruc(const PgruDev &d, hipStream_t s) {
  const int grid = PgruGridX(d.n_utts, d.delay, d.stride);
  if (grid <= 0) return;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&PgrucKernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPgruMaxLdsBytes);
  if (attr != hipSuccess) Fail(std::string("recurrent block kernel: cannot reserve its LDS: ") + hipGetErrorString(attr));
  hipLaunchKernelGGL(PgrucKernel, dim3((unsigned)grid), dim3(64 * kPgruWaves), (size_t)d.plan.lds_bytes, s, d);
}

void LaunchGruc(const GruDev &d, hipStream_t s) {
  const int grid = GruGridX(d.n_utts, d.delay, d.stride);
  if (grid <= 0) return;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&GrucKernel), hipFuncAttributeMaxDynamicSharedMemorySize, kGruMaxLdsBytes);
  if (attr != hipSuccess) Fail(std::string("recurrent block kernel: cannot reserve its LDS: ") + hipGetErrorString(attr));
  hipLaunchKernelGGL(GrucKernel, dim3((unsigned)grid), dim3(64 * kGruWaves), (size_t)d.plan.lds_bytes, s, d);
}

}  // namespace rs

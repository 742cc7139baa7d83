// What the recurrent block kernels share on the device (nnet_lstm.hip, nnet_lstmp.hip, nnet_lstmb.hip, nnet_gru.hip, nnet_pgru.hip,
// nnet_gruc.hip): the activations as the reference rounds them, the set-up of a workgroup's chains (recurrent_walk.h), the k-loop on
// v_mfma_f32_16x16x4_f32, the output-projection and normalisation phases of a step, and the launch.  Everything is inlined into
// the one kernel of a family; what a family's file keeps is its gate phase and its cell's roundings.
//
// Lane l of a wave holds, in register r of an accumulator, chain 4 (l >> 4) + r and column 16 item + (l & 15) of the wave's item.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "kernels.h"
#include "recurrent_walk.h"

namespace rs {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Sigmoid and Tanh as the reference writes them, on the full-precision expf: ScalarSigmoid / ScalarTanh of the fused nonlinearities
// (cudamatrix/cu-math.cc:422-442) and VectorBase::Sigmoid / Tanh of the SigmoidComponent / TanhComponent on the CPU
// (matrix/kaldi-vector.cc:899-951) are the same expressions
__device__ __forceinline__ float RefSigmoid(float x) {
  if (x > 0.f) return 1.f / (1.f + expf(-x));
  const float ex = expf(x);
  return ex / (ex + 1.f);
}
__device__ __forceinline__ float RefTanh(float x) {
  if (x > 0.f) {
    const float inv_expx = expf(-x);
    return -1.f + 2.f / (1.f + inv_expx * inv_expx);
  }
  const float expx = expf(x);
  return 1.f - 2.f / (1.f + expx * expx);
}

// The start of every kernel: the workgroup's chains, `lds_floats` floats of LDS zeroed, and the recurrent part of the state rows
// before the chains' first -- what an earlier advance parked at `row_off` of a parked row, `width` floats, else the zeros -- in
// `tile` (row pitch `pitch`).  Returns the steps of the workgroup's longest chain.
__device__ __forceinline__ int RecPrologue(const RecWalk &w, RecChain (&chains)[kRecChains], float *lds, int lds_floats, float *tile, int pitch,
                                           int width, int row_off) {
  __shared__ int n_steps_s;
  const int tid = threadIdx.x;
  if (tid < kRecChains) chains[tid] = RecChainSetUp(w, blockIdx.x * kRecChains + tid);
  for (int e = tid; e < lds_floats; e += 64 * kRecWaves) lds[e] = 0.f;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < kRecChains; i++) n = max(n, chains[i].count);
    n_steps_s = n;
  }
  for (int e = tid; e < kRecChains * width; e += 64 * kRecWaves) {
    const int i = e / width, k = e - i * width;
    if (chains[i].count > 0 && chains[i].cont) tile[i * pitch + k] = w.ring[chains[i].ring_off + row_off + k];
  }
  __syncthreads();
  return n_steps_s;
}

// a lane's N adjacent weights of one k: one 4-, 8- or 16-byte load
template <int N> struct RecWeights { float v[N]; };
template <int N> __device__ __forceinline__ RecWeights<N> RecLoadWeights(const float *p);
template <> __device__ __forceinline__ RecWeights<1> RecLoadWeights<1>(const float *p) { return {{p[0]}}; }
template <> __device__ __forceinline__ RecWeights<2> RecLoadWeights<2>(const float *p) {
  const float2 t = *reinterpret_cast<const float2 *>(p);
  return {{t.x, t.y}};
}
template <> __device__ __forceinline__ RecWeights<4> RecLoadWeights<4>(const float *p) {
  const float4 t = *reinterpret_cast<const float4 *>(p);
  return {{t.x, t.y, t.z, t.w}};
}

// The k-loop of every product: acc[j * N + g] += A . W over k = 0 .. k_ext - 1 (a multiple of 16), for the NP weight pointers wp[j]
// (the lane's first row, lk, and first column of a transposed weight of row pitch w_pitch) with N adjacent columns each, all over
// one LDS tile; a_off is the lane's place in its row of it, lm * pitch + lk.  The operands of four k-steps are loaded first, then
// their MFMAs run in k order: an element's sum is over k in the weight's column order, four per MFMA.
// (The loop is written over indices, as the kernels had it.  How the compiler schedules its loads depends on the register
// pressure around it: phase 2 of PgruKernel / PgrucKernel, one tile per accumulator, keeps a loop of its own, because through
// this template its loads came out one wait apiece.)
template <int NP, int N>
__device__ __forceinline__ void RecMfmaItems(f32x4 (&acc)[NP * N], const float *tile, int a_off, const float *const (&wp)[NP], int w_pitch, int k_ext) {
  for (int k0 = 0; k0 < k_ext; k0 += 16) {
    float a[4];
    RecWeights<N> w[NP][4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      a[u] = tile[a_off + k0 + 4 * u];
#pragma unroll
      for (int j = 0; j < NP; j++) w[j][u] = RecLoadWeights<N>(wp[j] + (size_t)(k0 + 4 * u) * w_pitch);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
#pragma unroll
      for (int j = 0; j < NP; j++) {
#pragma unroll
        for (int g = 0; g < N; g++) acc[j * N + g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[j][u].v[g], acc[j * N + g], 0, 0, 0);
      }
    }
  }
}
// (the usual case: one wave item, N accumulators over one weight pointer)
template <int N> __device__ __forceinline__ void RecMfma(f32x4 (&acc)[N], const float *tile, int a_off, const float *wp, int w_pitch, int k_ext) {
  const float *const wps[1] = {wp};
  RecMfmaItems<1, N>(acc, tile, a_off, wps, w_pitch, k_ext);
}

// The output projection of a step: out = W . tile + bias for the 16 chains, a wave item is 16 columns; the first `rec` columns are
// the state's recurrent part: scaled into the state buffer (from column st_col0), the next step's tile and, at the chain's
// save step, the ring (from ring_col0 of a parked row) -- or, `unscaled`, left as they are in the next step's tile for RecNormalize.
__device__ __forceinline__ void RecProject(const RecChain (&chains)[kRecChains], int n, int delay, const float *tile, int ld_tile, int k_ext,
                                           const float *w_t, int n_out, int out_tiles, const float *bias, float *out, int ld_out, int out_dim,
                                           int rec, float scale, bool unscaled, float *st, int ld_st, int st_col0, float *ring, int ring_col0,
                                           float *s_next, int ld_s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lm = lane & 15, lk = lane >> 4;
  for (int item = wave; item < out_tiles; item += kRecWaves) {
    const int col = 16 * item + lm;
    f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    RecMfma<1>(acc, tile, lm * ld_tile + lk, w_t + (size_t)lk * n_out + col, n_out, k_ext);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = 4 * lk + r;
      const RecChain &ch = chains[i];
      const bool live = n < ch.count && col < out_dim;
      float s_t = 0.f;
      if (live) {
        const long row = ch.row0 + n * delay;
        const float v = __fadd_rn(acc[0][r], bias[col]);
        out[row * ld_out + col] = v;
        if (col < rec) {
          if (unscaled) {
            s_t = v;
          } else {
            s_t = __fmul_rn(v, scale);
            st[row * ld_st + st_col0 + col] = s_t;
            if (n == ch.save_step) ring[ch.ring_off + ring_col0 + col] = s_t;
          }
        }
      }
      if (col < rec) s_next[i * ld_s + col] = s_t;
    }
  }
}

// The norm variants' last phase: NormalizePerRow (cu-math.cc:302-310) over each chain's rec columns of the next step's tile, then
// the scale.  A wave takes two chains; a lane sums its k = lane, lane + 64, ... in that order, the 64 partial sums meet in a fixed tree.
__device__ __forceinline__ void RecNormalize(const RecChain (&chains)[kRecChains], int n, int delay, float *s_next, int ld_s, int rec, float norm_alpha,
                                             float scale, float *st, int ld_st, float *ring, int ring_col0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < kRecChains; i += kRecWaves) {
    const RecChain &ch = chains[i];
    if (n >= ch.count) continue;      // (the whole wave: its row of the tile holds zeros)
    float *srow = s_next + i * ld_s;
    float ss = 0.f;
    for (int k = lane; k < rec; k += 64) ss = __fadd_rn(ss, __fmul_rn(srow[k], srow[k]));
    for (int o = 32; o > 0; o >>= 1) ss = __fadd_rn(ss, __shfl_xor(ss, o, 64));
    float nrm = __fmul_rn(ss, norm_alpha);
    nrm = fmaxf(nrm, 1.3552527156068805425e-20f);      // kSquaredNormFloor, 2^-66
    nrm = powf(nrm, -0.5f);
    const long row = ch.row0 + n * delay;
    for (int k = lane; k < rec; k += 64) {
      const float s_t = __fmul_rn(__fmul_rn(srow[k], nrm), scale);
      srow[k] = s_t;
      st[row * ld_st + k] = s_t;
      if (n == ch.save_step) ring[ch.ring_off + ring_col0 + k] = s_t;
    }
  }
}

// One workgroup per kRecChains chains of the call; the kernel's LDS cap is raised once per process and kernel.
template <typename Dev, void (*Kernel)(Dev), int kLdsCap = kRecMaxLdsBytes>
void RecLaunch(const Dev &d, hipStream_t s, const char *what = "recurrent block kernel") {
  const int grid = RecGridX(d.walk.n_utts, d.walk.delay, d.walk.stride);
  if (grid <= 0) return;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap);
  if (attr != hipSuccess) Fail(std::string(what) + ": cannot reserve its LDS: " + hipGetErrorString(attr));
  hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(64 * kRecWaves), (size_t)d.plan.lds_bytes, s, d);
}

}  // namespace rs

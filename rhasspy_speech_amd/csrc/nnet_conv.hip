// TimeHeightConvolutionComponent as an implicit GEMM on the exact-FP32 matrix cores, and the column gather of a PermuteComponent.
// What a workgroup takes, what it stages and why the order of one element's sum is fixed: conv_plan.h.
#include <hip/hip_runtime.h>

#include "conv_plan.h"
#include "kernels.h"
#include "nnet_common.h"

namespace rs {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int MPW, int NACC>
__global__ __launch_bounds__(64 * kConvWaves) void ConvKernel(ConvDev d, int rows) {
  extern __shared__ float lds[];
  const ConvLaunchPlan &p = d.plan;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * p.rows_per_block;
  const int nrows = min(p.rows_per_block, rows - i0);
  // ---- stage: per (frame of the tile, distinct time offset) the input row, hp heights of fs floats; what lies outside the
  // input's heights, the filler float of a height and the frames past the end of the list are zero
  const int n_slots = p.rows_per_block * d.n_t;
  for (int s = 0; s < n_slots; s++) {
    const int j = s / d.n_t, ti = s - j * d.n_t;
    const bool live = j < nrows;
    const float *srow = d.src;
    if (live) {
      const long prow = d.row_map ? d.row_map[i0 + j] : i0 + j;
      srow = d.src + (prow + d.row_off[ti]) * d.ld + d.col0;
    }
    float *dst = lds + s * p.slot;
    for (int e = tid; e < p.slot; e += 64 * kConvWaves) {
      const int hpi = e / p.fs, f = e - hpi * p.fs, h = hpi - p.pad_lo;
      float v = 0.f;
      if (live && f < d.filters_in && h >= 0 && h < d.height_in) v = srow[h * d.filters_in + f];
      dst[e] = v;
    }
  }
  __syncthreads();
  // ---- multiply: the workgroup's (group of MPW pixel tiles, chunk of NACC filter tiles) pairs, dealt round to the waves; k in
  // W's column order, four per MFMA
  const int lm = lane & 15, lk = lane >> 4;
  const int total_pix = nrows * d.height_out;
  const int m_groups = (p.m_tiles + MPW - 1) / MPW;
  for (int item = wave; item < m_groups * p.n_chunks; item += kConvWaves) {
    const int mg = item % m_groups, n0 = (item / m_groups) * NACC * 16;
    int base[MPW];
#pragma unroll
    for (int i = 0; i < MPW; i++) {
      const int pix = (mg * MPW + i) * 16 + lm;
      const int j = pix / d.height_out, h = pix - j * d.height_out;
      base[i] = pix < total_pix ? j * d.n_t * p.slot + h * d.height_sub * p.fs : 0;
    }
    f32x4 acc[MPW][NACC];
#pragma unroll
    for (int i = 0; i < MPW; i++)
#pragma unroll
      for (int n = 0; n < NACC; n++) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *wp = d.wt + (size_t)lk * p.n_pad + n0 + lm;
    const int *kp = d.koff + lk;
    for (int k0 = 0; k0 < p.k_pad; k0 += 4) {
      const int ko = kp[k0];
      const bool kin = k0 + lk < p.k;
      float a[MPW], b[NACC];
#pragma unroll
      for (int i = 0; i < MPW; i++) { const float x = lds[base[i] + ko]; a[i] = kin ? x : 0.f; }
#pragma unroll
      for (int n = 0; n < NACC; n++) b[n] = wp[(size_t)k0 * p.n_pad + n * 16];
#pragma unroll
      for (int i = 0; i < MPW; i++)
#pragma unroll
        for (int n = 0; n < NACC; n++) acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[n], acc[i][n], 0, 0, 0);
    }
    // ---- epilogue: bias, the fused stages, FP32 store (accumulator register r of lane l: pixel 4 (l >> 4) + r, filter l & 15)
#pragma unroll
    for (int i = 0; i < MPW; i++) {
      const int tile = mg * MPW + i;
      if (tile >= p.m_tiles) continue;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int pix = tile * 16 + lk * 4 + r;
        if (pix >= total_pix) continue;
        const int j = pix / d.height_out, h = pix - j * d.height_out;
        const long prow = d.row_map ? d.row_map[i0 + j] : i0 + j;
        float *orow = d.out + prow * d.ldo;
#pragma unroll
        for (int n = 0; n < NACC; n++) {
          const int f = n0 + n * 16 + lm;
          if (f >= d.filters_out) continue;
          const int col = h * d.filters_out + f;
          float v = __fadd_rn(acc[i][n][r], d.bias[f]);
          for (int st = 0; st < d.nstages; st++) v = ApplyStage(d.stages[st], v, col);
          orow[col] = v;
        }
      }
    }
  }
}

template <int MPW, int NACC>
void RunConv(const ConvDev &d, int rows, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&ConvKernel<MPW, NACC>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, kConvMaxLdsBytes);
  if (attr != hipSuccess) Fail(std::string("convolution kernel: cannot reserve its LDS: ") + hipGetErrorString(attr));
  hipLaunchKernelGGL((ConvKernel<MPW, NACC>), dim3((unsigned)ConvGridX(d.plan, rows)), dim3(64 * kConvWaves),
                     (size_t)d.plan.lds_bytes, s, d, rows);
}

__global__ void GatherKernel(GatherDev d, int rows) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)rows * d.dim) return;
  int row = (int)(idx / d.dim);
  const int col = (int)(idx % d.dim);
  if (d.row_map) row = d.row_map[row];
  const GatherDev::Part &pt = d.parts[d.part[col]];
  d.out[(size_t)row * d.ldo + col] = pt.src[((long)row + pt.row_off) * pt.ld + pt.col0 + d.col[col]];
}
}  // namespace

void LaunchConv(const ConvDev &d, int rows, hipStream_t s) {
  if (rows <= 0) return;
  const ConvLaunchPlan &p = d.plan;
  const int key = p.mpw * 10 + p.nacc;
  switch (key) {
    case 11: return RunConv<1, 1>(d, rows, s);
    case 12: return RunConv<1, 2>(d, rows, s);
    case 14: return RunConv<1, 4>(d, rows, s);
    case 21: return RunConv<2, 1>(d, rows, s);
    case 22: return RunConv<2, 2>(d, rows, s);
    case 24: return RunConv<2, 4>(d, rows, s);
  }
  Fail("convolution kernel: no instantiation conv16x16x4<m" + std::to_string(p.mpw) + ",n" + std::to_string(p.nacc) + ">");
}

void LaunchGather(const GatherDev &d, int rows, hipStream_t s) {
  const size_t total = (size_t)rows * d.dim;
  if (total == 0) return;
  hipLaunchKernelGGL(GatherKernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d, rows);
}

}  // namespace rs

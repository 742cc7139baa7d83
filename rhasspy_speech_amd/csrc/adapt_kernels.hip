// Speaker adaptation state of ended streams (kernels.h: AdaptWork), one workgroup per stream:
//   online2/online-ivector-feature.cc:386-396   OnlineIvectorFeature::GetAdaptationState
//   feat/online-feature.cc:467-487              OnlineCmvn::GetState: the statistics the utterance started with + (1, x, x^2) per raw frame
//   online2/online-ivector-feature.cc:109-127   LimitFrames
//   ivector/ivector-extractor.cc:671-693        OnlineIvectorEstimationStats::Scale (both max_count branches)
// Everything in double.  The sums run over the stream's raw MFCC rows in ascending frame order, one thread per dimension, so the
// result does not depend on how many streams a call lists.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rs {

namespace {
constexpr int kAdTC = 16;       // frames per chunk
constexpr int kAdPer = 8;       // elements of a chunk per thread: kAdTC * 128 dimensions = 256 * kAdPer

// Frames in chunks staged through LDS, the next chunk's loads in flight (in registers) while thread d walks the current one: a
// thread that read its dimension row by row from memory would wait out one trip per frame, thousands of them in a row.
__global__ __launch_bounds__(256) void AdaptGetKernel(AdaptWork w) {
  __shared__ float xs[kAdTC * 128];
  const int u = blockIdx.x, tid = threadIdx.x, D = w.dim, C1 = D + 1, T = w.frames[u], ld = w.ld;
  const size_t base = (size_t)w.row0[u];
  const float *__restrict__ in = w.raw;
  const int Di = w.has_iv ? w.ivec_dim : 0, usz = Di * (Di + 1) / 2, n_iv = w.has_iv ? Di + usz + 1 : 0;
  const double *car = w.carried + (size_t)u * 4 * C1;
  double *o = w.out + (size_t)u * w.out_stride;
  double *o_iv = o + n_iv, *o_nn = o_iv + (w.has_iv ? 2 * C1 : 0);
  // ---- speaker CMVN statistics: iVector branch (limited below) and nnet-input branch (never limited)
  const int dd = tid < D ? tid : 0;
  double s1i = car[dd], s2i = car[C1 + dd], cnt_i = car[D];
  double s1n = car[2 * C1 + dd], s2n = car[3 * C1 + dd], cnt_n = car[2 * C1 + D];
  float nx[kAdPer];
  const int i_first = tid / D, d_first = tid - i_first * D, i_step = 256 / D, d_step = 256 - i_step * D;      // element tid + 256 q = (frame, dimension), by steps
  auto fetch = [&](int t0) {
    const int n = T - t0 < kAdTC ? T - t0 : kAdTC;
    int i = i_first, d = d_first;
#pragma unroll
    for (int q = 0; q < kAdPer; q++) {
      const int ti = t0 + (i < n ? i : 0);      // (no load under a condition: an element past the chunk's end re-reads its first frame)
      nx[q] = in[(base + ti) * ld + d];
      i += i_step; d += d_step;
      if (d >= D) { d -= D; i++; }
    }
  };
  if (T > 0) fetch(0);
  for (int t0 = 0; t0 < T; t0 += kAdTC) {
    const int n = T - t0 < kAdTC ? T - t0 : kAdTC;
#pragma unroll
    for (int q = 0; q < kAdPer; q++) {
      const int idx = tid + 256 * q;
      if (idx < n * D) xs[idx] = nx[q];
    }
    __syncthreads();
    if (t0 + kAdTC < T) fetch(t0 + kAdTC);
    if (tid < D) {
      if (n == kAdTC) {
        float xv[kAdTC];
#pragma unroll
        for (int i = 0; i < kAdTC; i++) xv[i] = xs[i * D + tid];
#pragma unroll
        for (int i = 0; i < kAdTC; i++) { const double x = (double)xv[i]; s1i += x; s2i += x * x; }
        if (w.has_nn) {
#pragma unroll
          for (int i = 0; i < kAdTC; i++) { const double x = (double)xv[i]; s1n += x; s2n += x * x; }
        }
      } else {
        for (int i = 0; i < n; i++) {
          const double x = (double)xs[i * D + tid];
          s1i += x; s2i += x * x;
          s1n += x; s2n += x * x;
        }
      }
    }
    for (int i = 0; i < n; i++) { cnt_i += 1.0; cnt_n += 1.0; }
    __syncthreads();
  }
  if (w.has_iv) {
    // LimitFrames on the iVector branch's block: the whole 2 x (D + 1) matrix is scaled
    double sc = 1.0;
    if (cnt_i > w.max_remembered) sc = w.max_remembered / cnt_i;
    if (tid < D) { o_iv[tid] = sc != 1.0 ? s1i * sc : s1i; o_iv[C1 + tid] = sc != 1.0 ? s2i * sc : s2i; }
    if (tid == 0) { o_iv[D] = sc != 1.0 ? cnt_i * sc : cnt_i; o_iv[C1 + D] = sc != 1.0 ? car[C1 + D] * sc : car[C1 + D]; }
  }
  if (w.has_nn) {
    if (tid < D) { o_nn[tid] = s1n; o_nn[C1 + tid] = s2n; }
    if (tid == 0) { o_nn[D] = cnt_n; o_nn[C1 + D] = car[3 * C1 + D]; }
  }
  // ---- the estimator's statistics as they stand, limited
  if (w.has_iv) {
    const int slot = w.slot[u];
    const double *lin = w.lin + (size_t)slot * Di, *quad = w.quad + (size_t)slot * usz;
    const double nf = w.numf[slot], target = w.max_remembered_scaled;
    const bool apply = nf > target;
    double sc = 1.0, fix = 0.0, nf_new = nf;
    if (apply) {
      sc = target / nf;
      nf_new = nf * sc;
      if (w.max_count == 0.0) {
        fix = 1.0 - sc;
      } else {
        // the prior term was scaled with the statistics: bring it to the scale the new count asks for
        const double old_prior_scale = sc * fmax(nf, w.max_count) / w.max_count, new_prior_scale = fmax(nf_new, w.max_count) / w.max_count;
        fix = new_prior_scale - old_prior_scale;
      }
    }
    for (int k = tid; k < usz; k += 256) o[Di + k] = apply ? quad[k] * sc : quad[k];
    for (int i = tid; i < Di; i += 256) o[i] = apply ? lin[i] * sc : lin[i];
    if (tid == 0) o[Di + usz] = nf_new;
    __syncthreads();
    if (apply) {
      for (int r = tid; r < Di; r += 256) o[Di + (size_t)r * (r + 1) / 2 + r] += fix;
      if (tid == 0) o[0] += w.prior_offset * fix;
    }
  }
}
}  // namespace

void LaunchAdaptGet(const AdaptWork &w, hipStream_t s) {
  if (w.n_streams == 0) return;
  hipLaunchKernelGGL(AdaptGetKernel, dim3(w.n_streams), dim3(256), 0, s, w);
}

}  // namespace rs

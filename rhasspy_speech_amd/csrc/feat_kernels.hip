// Feature front-end kernels for gfx950: batched MFCC / log-mel filterbank and sliding-window CMVN (the iVector estimator lives in
// ivector_kernels.hip).  One 64-lane wavefront per frame for the per-frame kernels (CDNA4 wave64; never 32).
//
// Reference behaviour being reproduced (kaldi/src):
//   feat/feature-window.cc:90-224 (dither, DC removal, pre-emphasis, window, zero padding)
//   matrix/srfft.cc:356-432 + feat/feature-functions.cc:29-51 (real FFT -> 257-bin power spectrum)
//   feat/mel-computations.cc:226-251, feat/feature-mfcc.cc:28-80 (mel, log, DCT, lifter)
//   feat/feature-fbank.cc:72-123 (the filterbank row: optional sqrt, mel, floor + log, energy column)
//   feat/online-feature.cc:337-452 + transform/cmvn.cc:64-91 (OnlineCmvn)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "kernels.h"
#include "env.h"

namespace rs {

#define RS_WAVE 64

__device__ __forceinline__ float WaveSum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, RS_WAVE);
  return v;
}
// sum of a double over the wave: row rotations inside the rows of 16 lanes, then the four row results through SGPRs
__device__ __forceinline__ double WaveSumF64(double v) {
#define RS_DPP_D(CTRL)                                                                                                  \
  v += __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true),                       \
                        __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true));
  RS_DPP_D(0x121) RS_DPP_D(0x122) RS_DPP_D(0x124) RS_DPP_D(0x128)
#undef RS_DPP_D
  auto rl = [&](int l) { return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l)); };
  return (rl(0) + rl(16)) + (rl(32) + rl(48));
}
__device__ __forceinline__ float WaveMax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, RS_WAVE));
  return v;
}

// ------------------------------------------------------------------------------------------ MFCC
// One wave per frame; the rows of an utterance's halo (copies of its first / last frame) are written by the waves of those
// two frames.
//
// The real FFT is the reference's own algorithm (matrix/srfft.cc: in-place single-precision split radix + a
// post-processing pass whose twiddle comes from a float recurrence), restated as levels of independent butterfly
// tasks (srfft_plan.h) executed lane-parallel with the same float operations on the same operands, so the power
// spectrum matches the reference to the bit instead of to its own ~1e-3 rounding noise.  This file is compiled with
// -ffp-contract=off for that reason.
__device__ __forceinline__ void SrfftRunTask(const int4 tk, const float *__restrict__ tw, float *xr, float *xi, const float *tw_inline = nullptr) {
  const int kind = tk.x & 0xff, lg = tk.x >> 8, off = tk.y;
  if (kind == 0) {
    // srfft.cc:278-333 for one n: the four points it touches are private to this task
    const int m = 1 << lg, m2 = m >> 1, m4 = m >> 2, n = tk.z;
    const int e0 = off + n, e1 = e0 + m4, e2 = e0 + m2, e3 = e2 + m4;
    const float ar = xr[e0], ai = xi[e0], br = xr[e1], bi = xi[e1], cr = xr[e2], ci = xi[e2], dr = xr[e3], di = xi[e3];
    // step 1 on (e0, e2) and (e1, e3)
    xr[e0] = ar + cr; xi[e0] = ai + ci;
    xr[e1] = br + dr; xi[e1] = bi + di;
    const float p_r = ar - cr, p_i = ai - ci, q_r = br - dr, q_i = bi - di;
    // step 2 on the pair (e2, e3)
    float r1 = p_r + q_i, i2 = p_i + q_r, i1 = p_i - q_r, r2 = p_r - q_i;
    // steps 3 & 4
    if (tk.w == -2) {
      const float sqhalf = 0.70710678118654752440f;
      const float t1 = sqhalf * (r1 + i1);
      i1 = sqhalf * (i1 - r1);
      r1 = t1;
      const float t2 = sqhalf * (i2 - r2);
      i2 = -sqhalf * (r2 + i2);
      r2 = t2;
    } else if (tk.w >= 0) {
      const float *w = tw_inline ? tw_inline : tw + (size_t)tk.w * 6;
      const float cn = w[0], spcn = w[1], smcn = w[2], c3n = w[3], spc3n = w[4], smc3n = w[5];
      float t2 = cn * (r1 + i1);
      float t1 = spcn * r1 + t2;
      r1 = smcn * i1 + t2;
      i1 = t1;
      t2 = c3n * (r2 + i2);
      t1 = spc3n * r2 + t2;
      r2 = smc3n * i2 + t2;
      i2 = t1;
    }
    xr[e2] = r1; xi[e2] = i1;
    xr[e3] = r2; xi[e3] = i2;
  } else if (kind == 1) {
    // srfft.cc:227-264: the whole length-4 transform
    float r0 = xr[off], r1 = xr[off + 1], r2 = xr[off + 2], r3 = xr[off + 3];
    float i0 = xi[off], i1 = xi[off + 1], i2 = xi[off + 2], i3 = xi[off + 3];
    float t;
    t = r0 + r2; r2 = r0 - r2; r0 = t;
    t = i0 + i2; i2 = i0 - i2; i0 = t;
    t = r1 + r3; r3 = r1 - r3; r1 = t;
    t = i1 + i3; i3 = i1 - i3; i1 = t;
    t = r0 + r1; r1 = r0 - r1; r0 = t;
    t = i0 + i1; i1 = i0 - i1; i0 = t;
    const float t1 = r2 + i3, t2 = i2 + r3;
    i2 = i2 - r3;
    r3 = r2 - i3;
    r2 = t1;
    i3 = t2;
    xr[off] = r0; xr[off + 1] = r1; xr[off + 2] = r2; xr[off + 3] = r3;
    xi[off] = i0; xi[off + 1] = i1; xi[off + 2] = i2; xi[off + 3] = i3;
  } else {
    // srfft.cc:265-274: length 2
    const float r0 = xr[off], r1 = xr[off + 1], i0 = xi[off], i1 = xi[off + 1];
    xr[off] = r0 + r1; xr[off + 1] = r0 - r1;
    xi[off] = i0 + i1; xi[off + 1] = i0 - i1;
  }
}

// The same task from a 48-byte record of the padded, pre-addressed plan (MfccDev::fft_recs: 64 records per level, one per lane):
//   {byte offsets of the task's (up to) four points inside xr / xi; kind (3 = no task for this lane) | twiddle class << 8 (0 factors
//    below, 1 none, 2 the sqrt(1/2) case), the six twiddle factors; -}
// The offsets are those of the SWIZZLED layout (MfccDev::fft_swz): point i of the transform lives at index i ^ g(i >> 5).  In the
// plain layout the small blocks of the in-place split radix -- points 8 k + n, 16 k + n, ... -- put a half wave's 32 reads on 8 or
// 4 of the 32 LDS banks: the kernel's LDS pipe was busy 83 % of the time and half of that was bank conflicts (SQ_LDS_IDX_ACTIVE /
// SQ_LDS_BANK_CONFLICT, profiles/micro/pmc_lds.sh); the swizzle (found by exhaustive search over the linear ones against this plan's
// access patterns, profiles/micro/fft_swizzle.py) halves the passes of the levels and of the post-processing gather (636 -> 308
// per frame; 208 would be conflict-free).  Same float operations on the same operands.
__device__ __forceinline__ void SrfftRunRec(const float4 r0, const float4 r1, const float4 r2, float *xr, int xi_off) {
  const int meta = __float_as_int(r1.x), kind = meta & 0xff, twc = meta >> 8;
  char *xb = reinterpret_cast<char *>(xr);
  float *q0 = reinterpret_cast<float *>(xb + __float_as_int(r0.x)), *q1 = reinterpret_cast<float *>(xb + __float_as_int(r0.y));
  float *q2 = reinterpret_cast<float *>(xb + __float_as_int(r0.z)), *q3 = reinterpret_cast<float *>(xb + __float_as_int(r0.w));
  if (kind == 0) {
    const float ar = q0[0], ai = q0[xi_off], br = q1[0], bi = q1[xi_off], cr = q2[0], ci = q2[xi_off], dr = q3[0], di = q3[xi_off];
    q0[0] = ar + cr; q0[xi_off] = ai + ci;
    q1[0] = br + dr; q1[xi_off] = bi + di;
    const float p_r = ar - cr, p_i = ai - ci, q_r = br - dr, q_i = bi - di;
    float r1v = p_r + q_i, i2 = p_i + q_r, i1 = p_i - q_r, r2v = p_r - q_i;
    if (twc == 2) {
      const float sqhalf = 0.70710678118654752440f;
      const float t1 = sqhalf * (r1v + i1);
      i1 = sqhalf * (i1 - r1v);
      r1v = t1;
      const float t2 = sqhalf * (i2 - r2v);
      i2 = -sqhalf * (r2v + i2);
      r2v = t2;
    } else if (twc == 0) {
      const float cn = r1.y, spcn = r1.z, smcn = r1.w, c3n = r2.x, spc3n = r2.y, smc3n = r2.z;
      float t2 = cn * (r1v + i1);
      float t1 = spcn * r1v + t2;
      r1v = smcn * i1 + t2;
      i1 = t1;
      t2 = c3n * (r2v + i2);
      t1 = spc3n * r2v + t2;
      r2v = smc3n * i2 + t2;
      i2 = t1;
    }
    q2[0] = r1v; q2[xi_off] = i1;
    q3[0] = r2v; q3[xi_off] = i2;
  } else if (kind == 1) {
    float a0 = q0[0], a1 = q1[0], a2 = q2[0], a3 = q3[0];
    float i0 = q0[xi_off], i1 = q1[xi_off], i2 = q2[xi_off], i3 = q3[xi_off];
    float t;
    t = a0 + a2; a2 = a0 - a2; a0 = t;
    t = i0 + i2; i2 = i0 - i2; i0 = t;
    t = a1 + a3; a3 = a1 - a3; a1 = t;
    t = i1 + i3; i3 = i1 - i3; i1 = t;
    t = a0 + a1; a1 = a0 - a1; a0 = t;
    t = i0 + i1; i1 = i0 - i1; i0 = t;
    const float t1 = a2 + i3, t2 = i2 + a3;
    i2 = i2 - a3;
    a3 = a2 - i3;
    a2 = t1;
    i3 = t2;
    q0[0] = a0; q1[0] = a1; q2[0] = a2; q3[0] = a3;
    q0[xi_off] = i0; q1[xi_off] = i1; q2[xi_off] = i2; q3[xi_off] = i3;
  } else if (kind == 2) {
    const float a0 = q0[0], a1 = q1[0], i0 = q0[xi_off], i1 = q1[xi_off];
    q0[0] = a0 + a1; q1[0] = a0 - a1;
    q0[xi_off] = i0 + i1; q1[xi_off] = i0 - i1;
  }
}

// The waves of a workgroup work on different frames, each in its own slices of the LDS arrays: a wave only has to order
// its own LDS traffic (its earlier writes land before its later reads), no wave ever waits for another one.
__device__ __forceinline__ void WaveLdsSync() {
  __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// (the kernel: feature_frame_kernel.inc -- MfccKernel, and FbankKernel for log-mel filterbank models)
#define RS_FEAT_FBANK 0
#include "feature_frame_kernel.inc"
#undef RS_FEAT_FBANK
#define RS_FEAT_FBANK 1
#include "feature_frame_kernel.inc"
#undef RS_FEAT_FBANK

// (f: the filterbank kernel's own options; only read when FBANK)
template <bool FBANK, int NFFT, int WPB, bool TAB = false>
static void LaunchMfccT(const MfccDev &m, const FbankDev *f, const BatchGeom &g, const int16_t *pcm, float *feats, int ld, bool exclusive,
                        const int *out_rows, hipStream_t s) {
  const int blocks = (g.total_rows + WPB - 1) / WPB;
  if (!blocks) return;
  const size_t need = sizeof(float) * WPB * (3 * (NFFT / 2) + 1 + (FBANK ? 0 : 64)) + (TAB ? (size_t)m.fft_num_levels * 64 * 48 : 0);
  const size_t smem = exclusive ? std::max<size_t>(need, 159 * 1024) : need;
  static size_t attr = 0;
  const void *fn = FBANK ? reinterpret_cast<const void *>(&FbankKernel<NFFT, WPB, TAB>) : reinterpret_cast<const void *>(&MfccKernel<NFFT, WPB, TAB>);
  if (smem > attr) {
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    attr = smem;
  }
  if (FBANK) hipLaunchKernelGGL((FbankKernel<NFFT, WPB, TAB>), dim3(blocks), dim3(64 * WPB), smem, s, m, *f, g, pcm, feats, ld, out_rows);
  else hipLaunchKernelGGL((MfccKernel<NFFT, WPB, TAB>), dim3(blocks), dim3(64 * WPB), smem, s, m, g, pcm, feats, ld, out_rows);
}

template <bool FBANK>
static void LaunchFeatureKernel(const MfccDev &m, const FbankDev *f, const BatchGeom &g, const int16_t *pcm, float *feats, int ld, hipStream_t s,
                                bool exclusive, const int *out_rows) {
  if (m.padded == 512) {
    // Launches of one to about twelve device fills of 16-frame workgroups (8 k to 96 k rows: 64 to 256 utterances of 3 s) take them,
    // with the FFT plan in LDS.  Alone the launch is 4 % slower than with four frames per workgroup (167 against 161 us for the
    // headline batch: coarser tail), but beside other calls' layer GEMMs -- four calls in flight -- the pipelined step is shorter:
    // 0.59 against 0.73 ms for 64 utterances, 1.14 / 1.16 for 128, 1.52-1.56 / 1.63-1.69 for 256 (four boxes); 1.51 / 1.44 for 192 is
    // the exception inside the range, and above it the 4-wave form wins (384: 2.69 / 2.63, 512: 3.56 / 3.36, the mixed workload's
    // 512-utterance calls 6.8 / 6.5-6.6): profiles/micro/mfcc_shape_{ab,utts,conc,mixed}.sh.  Most of the effect is the workgroup size
    // (the 16-wave form without the tables shows it too) -- how this kernel's workgroups share CUs with the GEMMs' -- the rest a third
    // fewer vector memory requests.  An empirical launcher rule, not a model.  Small launches (a stream round, one utterance) keep the
    // 4-wave form.
    static const int shape_env = [] { const char *e = TuneEnv("RS_MFCC_SHAPE"); return e ? std::atoi(e) : -1; }();
    const bool tab_ok = m.fft_recs != nullptr && m.fft_num_levels * 64 * 48 <= 32 * 1024;
    const int shape = shape_env >= 0 ? shape_env : ((g.total_rows >= 16 * 512 && g.total_rows <= 96 * 1024) ? 16 : 0);
    // (the filterbank kernel takes the same shapes: its front end, where the shapes differ, is the same code)
    if (exclusive) LaunchMfccT<FBANK, 512, 16>(m, f, g, pcm, feats, ld, true, out_rows, s);
    else if (shape == 16 && tab_ok) LaunchMfccT<FBANK, 512, 16, true>(m, f, g, pcm, feats, ld, false, out_rows, s);
    else if (shape == 8 && tab_ok) LaunchMfccT<FBANK, 512, 8, true>(m, f, g, pcm, feats, ld, false, out_rows, s);
    else if (shape == 17) LaunchMfccT<FBANK, 512, 16>(m, f, g, pcm, feats, ld, false, out_rows, s);
    else LaunchMfccT<FBANK, 512, 4>(m, f, g, pcm, feats, ld, false, out_rows, s);
  } else if (m.padded == 256) {
    // An 8 kHz model's window: 128 complex points, the record-driven levels with half the lanes at work, one round of the
    // post-processing pass.  The 4-wave form only (DESIGN.md section 5 has its time per frame beside the 512-point window's).
    LaunchMfccT<FBANK, 256, 4>(m, f, g, pcm, feats, ld, exclusive, out_rows, s);
  } else if (m.padded == 1024) {
    LaunchMfccT<FBANK, 1024, 4>(m, f, g, pcm, feats, ld, exclusive, out_rows, s);
  } else {
    LaunchMfccT<FBANK, 2048, 4>(m, f, g, pcm, feats, ld, exclusive, out_rows, s);
  }
}

void LaunchMfcc(const MfccDev &m, const BatchGeom &g, const int16_t *pcm, float *feats, int ld, hipStream_t s, bool exclusive,
                const int *out_rows) {
  LaunchFeatureKernel<false>(m, nullptr, g, pcm, feats, ld, s, exclusive, out_rows);
}

void LaunchFbank(const MfccDev &m, const FbankDev &f, const BatchGeom &g, const int16_t *pcm, float *feats, int ld, hipStream_t s, bool exclusive,
                 const int *out_rows) {
  LaunchFeatureKernel<true>(m, &f, g, pcm, feats, ld, s, exclusive, out_rows);
}

// ------------------------------------------------------------------------------------------ online CMVN
// Workgroup per utterance, frames in chunks staged through LDS.  Per chunk: (1) thread d walks the frames with the same
// add-new / subtract-old double-precision update ComputeStatsForFrame performs (the only sequential part: two adds
// per frame), (2) one thread per frame does SmoothOnlineCmvnStats' per-frame scalars (the two fp64 divisions), (3) all
// threads apply the mean-only ApplyCmvn to the chunk in parallel with coalesced stores.  No speaker stats: the
// reference starts every utterance from a fresh process.
constexpr int kCmvnTC = 32;      // frames per chunk (the feature dimension is at most 128: engine.cc)
//
// Streams (t_begin != null): utterance u resumes at frame t_begin[u] with the running sums and the window count parked in
// state[(D + 1) * state_slot[u]] by the launch that produced frame t_begin[u] - 1, and parks them again at frame T; the frames
// that leave the window are re-read from `in`, which holds the whole stream.
// (the kernel: online_cmvn_kernel.inc)
#define RS_CMVN_SPK 0
#include "online_cmvn_kernel.inc"
#undef RS_CMVN_SPK
#define RS_CMVN_SPK 1
#include "online_cmvn_kernel.inc"
#undef RS_CMVN_SPK

void LaunchOnlineCmvn(const CmvnDev &c, const BatchGeom &g, const float *in, float *out, int ld, hipStream_t s, const int *t_begin,
                      double *state, const int *state_slot, const double *spk, const int *spk_slot) {
  if (g.n_utts == 0) return;
  const int D = c.dim;
  if (spk) {
    // (the plain kernel's LDS, then the speaker sums and weights behind it on an 8-byte boundary)
    const size_t smem_spk = sizeof(double) * ((size_t)kCmvnTC * D + D + 2 * kCmvnTC) + sizeof(float) * ((size_t)2 * kCmvnTC * D + kCmvnTC + 2 * D) +
                            sizeof(double) * ((size_t)D + kCmvnTC);
    static bool attr_spk_set = false;
    if (!attr_spk_set) { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&OnlineCmvnSpkKernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 74 * 1024); attr_spk_set = true; }
    if (D <= 40) hipLaunchKernelGGL(OnlineCmvnSpkKernel<5>, dim3(g.n_utts), dim3(256), smem_spk, s, c, g, in, out, ld, t_begin, state, state_slot, spk, spk_slot);
    else if (D <= 64) hipLaunchKernelGGL(OnlineCmvnSpkKernel<8>, dim3(g.n_utts), dim3(256), smem_spk, s, c, g, in, out, ld, t_begin, state, state_slot, spk, spk_slot);
    else hipLaunchKernelGGL(OnlineCmvnSpkKernel<16>, dim3(g.n_utts), dim3(256), smem_spk, s, c, g, in, out, ld, t_begin, state, state_slot, spk, spk_slot);
    return;
  }
  // (D <= 128: engine.cc refuses more cepstral coefficients when the model is loaded; kPer = 16 covers 32 frames x 128)
  const size_t smem = sizeof(double) * ((size_t)kCmvnTC * D + D + 2 * kCmvnTC) + sizeof(float) * ((size_t)2 * kCmvnTC * D + kCmvnTC + 2 * D);
  static bool attr_set = false;
  if (!attr_set) { (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&OnlineCmvnKernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024); attr_set = true; }
  if (D <= 40) hipLaunchKernelGGL(OnlineCmvnKernel<5>, dim3(g.n_utts), dim3(256), smem, s, c, g, in, out, ld, t_begin, state, state_slot);
  else if (D <= 64) hipLaunchKernelGGL(OnlineCmvnKernel<8>, dim3(g.n_utts), dim3(256), smem, s, c, g, in, out, ld, t_begin, state, state_slot);
  else hipLaunchKernelGGL(OnlineCmvnKernel<16>, dim3(g.n_utts), dim3(256), smem, s, c, g, in, out, ld, t_begin, state, state_slot);
}

// ------------------------------------------------------------------------------------------ row copies
// dst row dst_row[i] <- src row src_row[i], `width` 4-byte words each (one workgroup per row).  The streaming engine's
// glue: pool rows <-> the dense transient buffers of one advance (clamped context gathers, state parking).
__global__ __launch_bounds__(256) void CopyRowsKernel(const unsigned *__restrict__ src, long src_ld, const int *__restrict__ src_row,
                                                      unsigned *__restrict__ dst, long dst_ld, const int *__restrict__ dst_row, int width) {
  const int i = blockIdx.x;
  const unsigned *sp = src + (size_t)(src_row ? src_row[i] : i) * src_ld;
  unsigned *dp = dst + (size_t)(dst_row ? dst_row[i] : i) * dst_ld;
  if (((reinterpret_cast<uintptr_t>(sp) | reinterpret_cast<uintptr_t>(dp)) & 15) == 0) {
    const int w4 = width >> 2;
    for (int k = threadIdx.x; k < w4; k += 256) reinterpret_cast<uint4 *>(dp)[k] = reinterpret_cast<const uint4 *>(sp)[k];
    for (int k = (w4 << 2) + threadIdx.x; k < width; k += 256) dp[k] = sp[k];
  } else {
    for (int k = threadIdx.x; k < width; k += 256) dp[k] = sp[k];
  }
}
// up to four such copies with the same row lists in one launch (blockIdx.y = which)
__global__ __launch_bounds__(256) void CopyRowsMultiKernel(CopyRowsSet set, const int *__restrict__ src_row, const int *__restrict__ dst_row) {
  const int i = blockIdx.x;
  const CopyRowsSet::One c = set.a[blockIdx.y];
  const unsigned *sp = static_cast<const unsigned *>(c.src) + (size_t)(src_row ? src_row[i] : i) * c.ld;
  unsigned *dp = static_cast<unsigned *>(c.dst) + (size_t)(dst_row ? dst_row[i] : i) * c.ld;
  if (((reinterpret_cast<uintptr_t>(sp) | reinterpret_cast<uintptr_t>(dp)) & 15) == 0) {
    const int w4 = c.width >> 2;
    for (int k = threadIdx.x; k < w4; k += 256) reinterpret_cast<uint4 *>(dp)[k] = reinterpret_cast<const uint4 *>(sp)[k];
    for (int k = (w4 << 2) + threadIdx.x; k < c.width; k += 256) dp[k] = sp[k];
  } else {
    for (int k = threadIdx.x; k < c.width; k += 256) dp[k] = sp[k];
  }
}
void LaunchCopyRowsMulti(const CopyRowsSet &set, const int *src_row, const int *dst_row, int n, hipStream_t s) {
  if (n <= 0 || set.count <= 0) return;
  hipLaunchKernelGGL(CopyRowsMultiKernel, dim3(n, set.count), dim3(256), 0, s, set, src_row, dst_row);
}

// zero fill of a list of regions (blockIdx.y = region, 16 workgroups per region)
__global__ __launch_bounds__(256) void ZeroRegionsKernel(ZeroRegions z) {
  const ZeroRegions::One r = z.r[blockIdx.y];
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
  if (((reinterpret_cast<uintptr_t>(r.p) | r.bytes) & 15) == 0) {
    uint4 *p = static_cast<uint4 *>(r.p);
    for (size_t k = t; k < r.bytes / 16; k += nthreads) p[k] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    unsigned *p = static_cast<unsigned *>(r.p);
    for (size_t k = t; k < r.bytes / 4; k += nthreads) p[k] = 0u;
  }
}
void LaunchZeroRegions(const ZeroRegions &z, hipStream_t s) {
  if (z.count <= 0) return;
  hipLaunchKernelGGL(ZeroRegionsKernel, dim3(16, z.count), dim3(256), 0, s, z);
}

void LaunchCopyRows(const void *src, long src_ld_words, const int *src_row, void *dst, long dst_ld_words, const int *dst_row, int n, int width_words,
                    hipStream_t s) {
  if (n <= 0 || width_words <= 0) return;
  hipLaunchKernelGGL(CopyRowsKernel, dim3(n), dim3(256), 0, s, static_cast<const unsigned *>(src), src_ld_words, src_row,
                     static_cast<unsigned *>(dst), dst_ld_words, dst_row, width_words);
}

// A call's results (word counts, costs, counters, the first words of every transcript) stored into page-locked host memory by a
// kernel: four small device-to-host copies on the copy engine wait behind whatever the other calls in flight have queued there
// (their 25 MB sample uploads).
__global__ __launch_bounds__(64) void ResultsToHostKernel(const int *__restrict__ nw, const float *__restrict__ costs, const long long *__restrict__ ctr,
                                                          const int *__restrict__ words, int max_words, int inline_words, int h_stride, int *h_nw,
                                                          float *h_costs, long long *h_ctr, int *h_words, const int *__restrict__ ali, int ali_ld,
                                                          int *h_ali) {
  const int u = blockIdx.x, t = threadIdx.x;
  if (t == 0) h_nw[u] = nw[u];
  if (t < 4) h_costs[(size_t)u * 4 + t] = costs[(size_t)u * 4 + t];
  if (t < 8) h_ctr[(size_t)u * 8 + t] = ctr[(size_t)u * 8 + t];
  for (int k = t; k < inline_words; k += 64) h_words[(size_t)u * h_stride + k] = words[(size_t)u * max_words + k];
  if (ali != nullptr)      // (rs_decode_opts.emit_alignment: the alignment rows ride along)
    for (int k = t; k < ali_ld; k += 64) h_ali[(size_t)u * ali_ld + k] = ali[(size_t)u * ali_ld + k];
}
void LaunchResultsToHost(const int *nw, const float *costs, const long long *ctr, const int *words, int max_words, int inline_words, int h_stride, int n,
                         int *h_nw, float *h_costs, long long *h_ctr, int *h_words, hipStream_t s, const int *ali, int ali_ld, int *h_ali) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ResultsToHostKernel, dim3(n), dim3(64), 0, s, nw, costs, ctr, words, max_words, inline_words, h_stride, h_nw, h_costs, h_ctr, h_words,
                     h_ali ? ali : nullptr, ali_ld, h_ali);
}

// ------------------------------------------------------------------------------------------ row geometry
// Per-row lookup tables of the ragged time-major layout (kernels.h), derived on the device from the per-utterance row
// bases: utterance of a row, its frame index relative to the utterance (negative / >= T in the halo), and -- offline --
// the iVector row it reads.
__global__ void RowGeometryKernel(int n_utts, int rows, int L, const int *__restrict__ row_base, const int *__restrict__ ivrow_base,
                                  int *__restrict__ row_utt, int *__restrict__ row_t, int *__restrict__ row_ivec) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  int lo = 0, hi = n_utts;          // largest u with row_base[u] <= r
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (row_base[mid] <= r) lo = mid; else hi = mid; }
  row_utt[r] = lo;
  row_t[r] = r - row_base[lo] - L;
  if (row_ivec) row_ivec[r] = ivrow_base[lo];
}
__global__ void FrameRowsKernel(int n_utts, int n_segs, int total, int L, int slab_len, const int *__restrict__ seg_off,
                                const int *__restrict__ row_base, int *__restrict__ frame_rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int lo = 0, hi = n_segs;          // largest segment with seg_off[seg] <= i
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seg_off[mid] <= i) lo = mid; else hi = mid; }
  const int k = lo / n_utts, u = lo % n_utts;
  frame_rows[i] = row_base[u] + L + k * slab_len + (i - seg_off[lo]);
}
// RowGeometryKernel + one FrameRowsKernel per list, as block ranges of one launch
__global__ __launch_bounds__(256) void BatchSetupKernel(BatchSetup b) {
  int blk = blockIdx.x;
  const int geo_blocks = (b.rows + 255) / 256;
  if (blk < geo_blocks) {
    const int r = blk * 256 + threadIdx.x;
    if (r >= b.rows) return;
    int lo = 0, hi = b.n_utts;          // largest u with row_base[u] <= r
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (b.row_base[mid] <= r) lo = mid; else hi = mid; }
    b.row_utt[r] = lo;
    b.row_t[r] = r - b.row_base[lo] - b.L;
    if (b.row_ivec) b.row_ivec[r] = b.ivrow_base[lo];
    return;
  }
  blk -= geo_blocks;
  for (int l = 0; l < b.n_lists; l++) {      // (block-uniform)
    const int nb = (b.lists[l].total + 255) / 256;
    if (blk < nb) {
      const BatchSetup::List &ls = b.lists[l];
      const int i = blk * 256 + threadIdx.x;
      if (i >= ls.total) return;
      int lo = 0, hi = ls.n_segs;          // largest segment with seg_off[seg] <= i
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ls.seg_off[mid] <= i) lo = mid; else hi = mid; }
      const int k = lo / b.n_utts, u = lo % b.n_utts;
      ls.out[i] = b.row_base[u] + ls.L + k * ls.slab_len + ls.first + ls.stride * (i - ls.seg_off[lo]);
      return;
    }
    blk -= nb;
  }
}
void LaunchBatchSetup(const BatchSetup &b, hipStream_t s) {
  int blocks = (b.rows + 255) / 256;
  for (int l = 0; l < b.n_lists; l++) blocks += (b.lists[l].total + 255) / 256;
  if (blocks <= 0) return;
  hipLaunchKernelGGL(BatchSetupKernel, dim3(blocks), dim3(256), 0, s, b);
}
void LaunchFrameRows(int n_utts, int n_segs, int total, int L, int slab_len, const int *seg_off, const int *row_base, int *frame_rows,
                     hipStream_t s) {
  if (total <= 0) return;
  hipLaunchKernelGGL(FrameRowsKernel, dim3((total + 255) / 256), dim3(256), 0, s, n_utts, n_segs, total, L, slab_len, seg_off, row_base, frame_rows);
}
void LaunchRowGeometry(int n_utts, int rows, int L, const int *row_base, const int *ivrow_base, int *row_utt, int *row_t, int *row_ivec,
                       hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(RowGeometryKernel, dim3((rows + 255) / 256), dim3(256), 0, s, n_utts, rows, L, row_base, ivrow_base, row_utt, row_t, row_ivec);
}

}  // namespace rs

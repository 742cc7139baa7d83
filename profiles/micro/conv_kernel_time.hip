// The convolution kernel (rhasspy_speech_amd/csrc/nnet_conv.hip) alone on the layers of a CNN-TDNN recipe, 256 utterances of
// 300 frames: 1->64 and 64->64 filters on 40 heights, 64->128 with height subsampling 2 (40 -> 20), 128->256 (20 -> 10), 3x3
// offsets, ReLU and BatchNorm fused as in a model.  Per layer: the plan the model load would choose, the median time of `repeats`
// launches after `warmup` (HIP events around each launch, one process), and the useful FLOP rate as a fraction of the FP32
// matrix-core peak (157.3 TFLOP/s).  Built and run by conv_kernel_time.py against librhasspy_speech_hip.so.
//   usage: conv_kernel_time [repeats, default 20] [warmup, default 3]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/conv_plan.h"
#include "../../rhasspy_speech_amd/csrc/kernels.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
  const int repeats = argc > 1 ? std::atoi(argv[1]) : 20, warmup = argc > 2 ? std::atoi(argv[2]) : 3;
  const int rows = 256 * 300, halo = 8;
  struct Layer { int fi, fo, hi, ho, sub; } layers[] = {{1, 64, 40, 40, 1}, {64, 64, 40, 40, 1}, {64, 128, 40, 20, 2}, {128, 256, 20, 10, 2}};
  hipStream_t s;
  CHECK(hipStreamCreate(&s));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::mt19937 rng(1);
  std::normal_distribution<float> nd(0.0f, 1.0f);
  std::printf("layer                 plan                                                         median us   min us  TFLOP/s  of peak\n");
  for (const Layer &l : layers) {
    rs::ConvGeom g;
    g.filters_in = l.fi; g.filters_out = l.fo; g.height_in = l.hi; g.height_out = l.ho; g.height_sub = l.sub;
    for (int t = -1; t <= 1; t++)
      for (int h = -1; h <= 1; h++) g.offsets.emplace_back(t, h);
    g.time_offsets = {-1, 0, 1};
    const rs::ConvLaunchPlan p = rs::PlanConv(g, "layer");
    rs::MatF W;
    W.Resize(l.fo, g.K());
    for (float &w : W.d) w = nd(rng) / std::sqrt((float)g.K());
    std::vector<float> wt, bias(l.fo, 0.1f), scale((size_t)l.ho * l.fo, 1.25f), offset((size_t)l.ho * l.fo, -0.3f);
    std::vector<int> koff;
    rs::ConvWeightImage(g, p, W, &wt, &koff);
    const size_t in_dim = (size_t)l.hi * l.fi, out_dim = (size_t)l.ho * l.fo;
    std::vector<float> in((size_t)(rows + 2 * halo) * in_dim);
    for (float &x : in) x = nd(rng);
    float *d_in, *d_out, *d_wt, *d_bias, *d_scale, *d_offset;
    int *d_koff;
    CHECK(hipMalloc(&d_in, in.size() * 4));
    CHECK(hipMalloc(&d_out, (size_t)rows * out_dim * 4));
    CHECK(hipMalloc(&d_wt, wt.size() * 4));
    CHECK(hipMalloc(&d_koff, koff.size() * 4));
    CHECK(hipMalloc(&d_bias, bias.size() * 4));
    CHECK(hipMalloc(&d_scale, scale.size() * 4));
    CHECK(hipMalloc(&d_offset, offset.size() * 4));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_wt, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_koff, koff.data(), koff.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_scale, scale.data(), scale.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_offset, offset.data(), offset.size() * 4, hipMemcpyHostToDevice));
    rs::ConvDev d;
    std::memset(&d, 0, sizeof(d));
    d.src = d_in + (size_t)halo * in_dim; d.ld = (int)in_dim; d.col0 = 0;      // (rows -1 and `rows` exist: the halo)
    d.n_t = 3;
    for (int i = 0; i < 3; i++) d.row_off[i] = i - 1;
    d.wt = d_wt; d.koff = d_koff; d.bias = d_bias;
    d.nstages = 2;
    d.stages[0].kind = 0;
    d.stages[1].kind = 1; d.stages[1].scale = d_scale; d.stages[1].offset = d_offset;
    d.out = d_out; d.ldo = (int)out_dim;
    d.filters_in = l.fi; d.filters_out = l.fo; d.height_in = l.hi; d.height_out = l.ho; d.height_sub = l.sub;
    d.plan = p;
    std::vector<float> us;
    for (int i = 0; i < warmup + repeats; i++) {
      CHECK(hipEventRecord(e0, s));
      rs::LaunchConv(d, rows, s);
      CHECK(hipEventRecord(e1, s));
      CHECK(hipEventSynchronize(e1));
      CHECK(hipGetLastError());
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (i >= warmup) us.push_back(ms * 1e3f);
    }
    std::sort(us.begin(), us.end());
    const double med = us[us.size() / 2], flop = 2.0 * rows * l.ho * l.fo * (double)g.K(), tf = flop / (med * 1e-6) / 1e12;
    char name[64], plan[128];
    std::snprintf(name, sizeof name, "%d->%d @%d->%d", l.fi, l.fo, l.hi, l.ho);
    std::snprintf(plan, sizeof plan, "conv16x16x4<m%d,n%d> rows/block %d tiles %d chunks %d lds %d grid %d", p.mpw, p.nacc, p.rows_per_block, p.m_tiles,
                  p.n_chunks, p.lds_bytes, rs::ConvGridX(p, rows));
    std::printf("%-21s %-60s %9.0f %8.0f %8.2f %7.1f%%\n", name, plan, med, (double)us[0], tf, 100.0 * tf / 157.3);
    for (void *ptr : {(void *)d_in, (void *)d_out, (void *)d_wt, (void *)d_koff, (void *)d_bias, (void *)d_scale, (void *)d_offset}) CHECK(hipFree(ptr));
  }
  return 0;
}

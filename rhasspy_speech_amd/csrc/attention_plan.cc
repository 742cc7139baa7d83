// See attention_plan.h.
#include "attention_plan.h"

#include <algorithm>
#include <sstream>

namespace rs {

namespace {
int Pitch(const AttentionGeom &g, int hg) { return (hg * (g.key_dim + g.value_dim)) | 1; }
}  // namespace

long AttentionLdsFloats(const AttentionGeom &g, int frames, int hg) {
  const int C = g.Context();
  const long cap_rows = frames + (long)(C - 1) * g.stride;
  return frames + cap_rows * Pitch(g, hg) + (long)frames * hg * (g.key_dim + C + C);
}

AttentionLaunchPlan PlanAttention(const AttentionGeom &g, const std::string &name) {
  const std::string what = "nnet3: attention " + name + ": ";
  const int C = g.Context();
  if (g.heads <= 0 || g.key_dim <= 0 || g.value_dim <= 0 || g.left < 0 || g.right < 0 || C < 2 || g.stride <= 0) Fail(what + "bad dimensions");
  if (g.key_dim > kAttnMaxDim) Fail(what + "key-dim " + std::to_string(g.key_dim) + " is more than the " + std::to_string(kAttnMaxDim) + " the HIP attention kernel takes");
  if (g.value_dim > kAttnMaxDim) Fail(what + "value-dim " + std::to_string(g.value_dim) + " is more than the " + std::to_string(kAttnMaxDim) + " the HIP attention kernel takes");
  if (C > kAttnMaxContext)
    Fail(what + std::to_string(C) + " context positions (num-left-inputs + 1 + num-right-inputs); the HIP attention kernel takes at most " + std::to_string(kAttnMaxContext));
  if (g.heads > kAttnMaxHeads) Fail(what + std::to_string(g.heads) + " heads; the HIP attention kernel takes at most " + std::to_string(kAttnMaxHeads));
  if (g.stride > kAttnMaxStride) Fail(what + "time-stride " + std::to_string(g.stride) + " is more than the " + std::to_string(kAttnMaxStride) + " the HIP attention kernel takes");
  const long budget = kAttnMaxLdsBytes / (long)sizeof(float);
  // the most frames whose rows, context rows, queries and softmax inputs fit, for hg heads a workgroup
  auto frames_for = [&](int hg) {
    const long per_frame = 1 + Pitch(g, hg) + (long)hg * (g.key_dim + C + C), fixed = (long)(C - 1) * g.stride * Pitch(g, hg);
    return (int)std::min<long>(kAttnMaxFrames, budget > fixed ? (budget - fixed) / per_frame : 0);
  };
  // as many heads as leave a tile at least four times its context rows long (a quarter of the staged rows at most is halo), else
  // one head and the longest tile that fits
  const int want = std::min(kAttnMaxFrames, 4 * (C - 1) * g.stride);
  int hg = 1;
  for (int h = g.heads; h > 1; h--)
    if (frames_for(h) >= want) { hg = h; break; }
  const int frames = frames_for(hg);
  if (frames < 1)
    Fail(what + "the rows one frame reads (" + std::to_string((C - 1) * g.stride + 1) + " rows x (key-dim " + std::to_string(g.key_dim) + " + value-dim " +
         std::to_string(g.value_dim) + "), " + std::to_string(AttentionLdsFloats(g, 1, 1) * (long)sizeof(float)) + " bytes with its query) do not fit the " +
         std::to_string(kAttnMaxLdsBytes) + " bytes of LDS the HIP attention kernel stages them in");
  AttentionLaunchPlan p;
  p.frames = frames;
  p.heads_per_block = hg;
  p.head_groups = (g.heads + hg - 1) / hg;
  p.cap_rows = frames + (C - 1) * g.stride;
  p.pitch = Pitch(g, hg);
  p.q_pitch = g.key_dim + C;
  p.lds_bytes = (int)(AttentionLdsFloats(g, frames, hg) * (long)sizeof(float));
  return p;
}

std::string DescribeAttention(const std::string &name, const AttentionGeom &g, const AttentionLaunchPlan &p) {
  std::ostringstream os;
  os << name << " heads=" << g.heads << " key=" << g.key_dim << " value=" << g.value_dim << " left=" << g.left << " right=" << g.right << " stride=" << g.stride
     << " key_scale=" << g.key_scale << " context=" << (g.output_context ? 1 : 0) << " in=" << g.InDim() << " out=" << g.OutDim() << " kernel=attn_valu<w"
     << kAttnWaves << "> frames=" << p.frames << " heads_per_block=" << p.heads_per_block << " head_groups=" << p.head_groups << " staged_rows=" << p.cap_rows
     << " pitch=" << p.pitch << " lds=" << p.lds_bytes << " grid=rows/" << p.frames << "x" << p.head_groups;
  return os.str();
}

}  // namespace rs

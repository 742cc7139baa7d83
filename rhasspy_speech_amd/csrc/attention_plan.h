// RestrictedAttentionComponent on the device (nnet_attention.hip): the descriptor the kernel takes by value and the host-only
// planner that decides, when the model loads, how many frames and heads a workgroup takes, what it stages in LDS and on which
// grid.  Nothing here includes a HIP header (tests/host/attention_plan_check.cc compiles it with g++).
//
// The layer (AttentionGeom, model.h): per frame t and head, C = left + 1 + right dot products of K elements against the keys of
// the rows t + (o - left) stride, a softmax over them, and the sum of those rows' values weighted by it.  Exact FP32 on the VALU:
// with K, V <= 128 and C <= 32 no product is worth a matrix core, and the layer is bound by its rows' bytes.  A workgroup of eight
// waves takes `frames` consecutive rows of the op's row list and `heads_per_block` heads.  It walks the frames in runs: a run is as
// many frames as have all their context rows inside `cap_rows` consecutive physical rows (frames + (C - 1) stride of them: every
// run of a dense list is the whole tile; rows of two utterances, or a list with gaps, make shorter runs).  Per run it stages the
// [key | value] columns of those rows for its heads once (`pitch` floats a row, odd: the C rows a frame reads fall on different
// banks) and the frames' query columns, then computes b, the softmax and the weighted sum from LDS.  Every input row so comes from
// HBM once per (frames + (C - 1) stride) / frames tiles instead of C times.  Workgroup barriers only; one output element is one
// thread's sum in the order k = 0 .. K-1, o = 0 .. C-1, whatever the frame's place in the tile, the batch or the chunk.
#pragma once
#include <string>

#include "model.h"

namespace rs {

constexpr int kAttnMaxDim = 128;              // key-dim, value-dim
constexpr int kAttnMaxContext = 32;           // left + 1 + right
constexpr int kAttnMaxHeads = 64;
constexpr int kAttnMaxStride = 32;
constexpr int kAttnMaxFrames = 128;           // frames of a workgroup
constexpr int kAttnWaves = 8;                 // waves of a workgroup: sixteen to a CU beside a second workgroup
constexpr int kAttnMaxLdsBytes = 64 * 1024;   // two workgroups to a CU's 160 KiB

struct AttentionLaunchPlan {
  int frames = 0;            // rows of the op's row list a workgroup takes
  int heads_per_block = 0;   // heads a workgroup takes
  int head_groups = 0;       // ceil(heads / heads_per_block): the grid's y
  int cap_rows = 0;          // physical rows a run stages at most: frames + (C - 1) stride
  int pitch = 0;             // floats per staged row: heads_per_block (K + V), made odd
  int q_pitch = 0;           // floats per staged (frame, head) query: K + C
  int lds_bytes = 0;         // frames ints (physical rows) + cap_rows pitch + frames heads_per_block (q_pitch + C) floats
};

// Fails (rs::Error) with a message naming the layer when a size is beyond the kernel's or one frame does not fit LDS.
AttentionLaunchPlan PlanAttention(const AttentionGeom &g, const std::string &name);
inline int AttentionGridX(const AttentionLaunchPlan &p, int rows) { return (rows + p.frames - 1) / p.frames; }
// LDS floats a plan of `frames` frames and `hg` heads per workgroup needs (the planner's own formula, for the check program)
long AttentionLdsFloats(const AttentionGeom &g, int frames, int hg);
// "name heads=2 key=8 value=8 left=2 right=1 stride=1 key_scale=0.353553 context=1 kernel=attn_valu<w8> frames=128 heads_per_block=2 ..."
std::string DescribeAttention(const std::string &name, const AttentionGeom &g, const AttentionLaunchPlan &p);

struct AttentionDev {
  const float *src;       // the source buffer (row 0)
  int ld, col0;
  int row_off;            // the descriptor's Offset(): context position o of list row i reads physical row i + row_off + (o - left) stride
  int heads, key_dim, value_dim, left, context, stride, output_context;
  float key_scale;
  float *out;
  int ldo;
  const int *row_map;     // null, or `rows` entries: list row i is physical row row_map[i] of the source and of the result
  AttentionLaunchPlan plan;
};

}  // namespace rs

// TimeHeightConvolutionComponent on the device (nnet_conv.hip): the descriptor the kernel takes by value and the host-only
// planner that decides, when the model loads, which instantiation runs a layer, how many frames a workgroup takes, what it
// stages in LDS and on which grid.  Nothing here includes a HIP header (tests/host/conv_plan_check.cc compiles it with g++).
//
// The layer as a GEMM: row (t, h_out), column f_out, k = offset index * filters_in + f_in,
//   out[t][h_out * F_out + f_out] = bias[f_out] + sum_k W[f_out][k] * in[t + dt(k)][(h_out * sub + dh(k)) * F_in + f_in(k)],
// terms whose input height falls outside [0, height_in) being zero (convolution.h:118-123).  A workgroup of four waves takes
// `rows_per_block` frames: it stages their input rows t + dt -- every distinct dt once, `pad_lo` zero heights below and `pad_hi`
// above -- in LDS, `fs` floats per height (filters_in made odd: neighbouring heights fall on different banks), and every wave
// multiplies 16-pixel tiles of those frames by 16-filter tiles of W on v_mfma_f32_16x16x4_f32 -- the (pixel tile group, filter
// chunk) pairs of the workgroup dealt round to its waves, so that the frames are staged once whatever the number of filters.
// The A operand of k-step s is LDS[pixel base + koff[4 s + (lane >> 4)]]: one table lookup per step, no bounds test (the
// padding is in LDS).  The sum over k of one output element runs in the order of W's columns, four per MFMA, whatever the
// frame's place in the tile, the batch or the chunk.
#pragma once
#include <string>
#include <vector>

#include "gemm_dev.h"
#include "model.h"

namespace rs {

constexpr int kConvMaxTimeOffsets = 8;
constexpr int kConvWaves = 4;                  // waves of a workgroup
constexpr int kConvMaxLdsBytes = 96 * 1024;    // staged input of one workgroup (of the CU's 160 KiB)

struct ConvLaunchPlan {
  int mpw = 0;              // 16-pixel tiles a wave holds at a time: 1 or 2
  int nacc = 0;             // 16-filter tiles per pixel tile a wave holds at a time: 1, 2 or 4
  int rows_per_block = 0;   // frames of a workgroup
  int m_tiles = 0;          // 16-pixel tiles of a workgroup: ceil(rows_per_block * height_out / 16) <= kConvWaves * mpw
  int pad_lo = 0, pad_hi = 0, hp = 0;   // zero heights staged below / above, hp = pad_lo + height_in + pad_hi
  int fs = 0;               // floats per staged height
  int slot = 0;             // floats per staged (frame, time offset): hp * fs
  int lds_bytes = 0;
  int k = 0, k_pad = 0;     // filters_in * offsets, rounded up to the k-step of 4
  int n_pad = 0;            // filters_out rounded up to 16 * nacc
  int n_chunks = 0;         // n_pad / (16 * nacc): the filter chunks a workgroup's waves share out with its pixel tiles
};

// Fails (rs::Error) with a message naming the layer when no instantiation covers the geometry or one frame does not fit LDS.
ConvLaunchPlan PlanConv(const ConvGeom &g, const std::string &name);
inline int ConvGridX(const ConvLaunchPlan &p, int rows) { return (rows + p.rows_per_block - 1) / p.rows_per_block; }
// W in the kernel's order, [k_pad][n_pad] (zero padded), and the LDS offset of every k relative to its pixel's base
void ConvWeightImage(const ConvGeom &g, const ConvLaunchPlan &p, const MatF &W, std::vector<float> *wt, std::vector<int> *koff);
// "name filters=1->8 heights=40->40 sub=1 offsets=9 k=9 kernel=conv16x16x4<m1,n1> rows_per_block=3 ... filter_chunks=1 grid=rows/3"
std::string DescribeConv(const std::string &name, const ConvGeom &g, const ConvLaunchPlan &p);

struct ConvDev {
  const float *src;       // the source buffer (row 0), the same for every time offset
  int ld, col0;
  int n_t;
  int row_off[kConvMaxTimeOffsets];   // rows relative to the output row, per distinct time offset
  const float *wt;        // [k_pad][n_pad]
  const int *koff;        // k_pad entries
  const float *bias;      // filters_out
  int nstages;
  EltStageDev stages[kMaxStages];
  float *out;
  int ldo;
  const int *row_map;     // null, or `rows` entries: list row i is physical row row_map[i] of the source and of the result
  int filters_in, filters_out, height_in, height_out, height_sub;
  ConvLaunchPlan plan;
};

// PermuteComponent over the parts of an Append: out[row][i] = parts[part[i]][row + row_off][col0 + col[i]]
struct GatherDev {
  int nparts;
  struct Part { const float *src; int ld, col0, row_off; } parts[8];
  const int *part, *col;  // dim entries each
  int dim;
  float *out;
  int ldo;
  const int *row_map;
};

}  // namespace rs

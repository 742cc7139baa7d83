// Recurrent blocks of the output-gate projected GRU (nnet3's fast-opgru-layer / fast-norm-opgru-layer) on the device
// (nnet_gru.hip): the descriptor the kernel takes by value and the host-only planner that decides, when the model loads, what a
// workgroup keeps in LDS and on which grid.  Nothing here includes a HIP header (tests/host/gru_plan_check.cc compiles it with g++).
//
// A block (model.h: GruBlock) per row t, with the delay d:
//   z = Sigmoid(pre_z[t] + W_z,s s[t - d]);  o = Sigmoid(pre_o[t] + W_o,s s[t - d]);  h = Tanh(pre_h[t] + w_h . c[t - d])
//   c = h - z . h + z . c[t - d];  y = W_y (c . o) + b_y;  s[t] = scale y[0:rec]  (norm: scale Normalize(y[0:rec]))
// pre = [W_z,x; W_o,x; W_hpart] x + b has no dependence on time and is one layer GEMM over all rows.  What is serial is walked by
// this kernel the way nnet_lstm.hip walks an LSTM block (lstm_plan.h): row t needs row t - d only, so the rows of an utterance fall
// into d independent chains (d / stride of them under --frame-subsampling-factor); a workgroup owns kRecChains chains for the whole
// launch and walks their steps with workgroup barriers only, the grid is the number of chains over kRecChains.
//
// A step: the 16 chains' s[t - d] rows are in LDS (zero where a chain has no earlier row), W_zo,s s for 16 cells x 2 gates per wave
// item on v_mfma_f32_16x16x4_f32 (the accumulators start from pre[t]), the sigmoids, h and c in the accumulators' registers against
// c[t - d] (the lane's own store of the step before), c . o into LDS, W_y (c . o) on the same instruction, the scaled first rec
// columns into the state buffer and into the other s tile.  The norm variant first leaves the unscaled columns in that tile and,
// behind one more barrier, scales each chain's row by 1 / sqrt(max(floor, sum x^2 / rec)): the sum runs per lane over k = lane,
// lane + 64, ... and then over the wave's 64 lanes in a fixed tree, an order that is a function of rec alone.  Both products are
// exact FP32 with FP32 accumulation, k in the weight's column order, four per MFMA, whatever the chain's place in the tile, the
// workgroup or the batch -- a row's result is a function of its inputs alone.
//
// The composed form of the same cell (opgru-layer / norm-opgru-layer, model.h: GruBlock::composed; w_h is then the <Params> of
// W_h.UW_elementwise) shares the descriptor, the planner, the weight images and the limits; it is walked by a kernel of its own
// (nnet_gruc.hip: GrucKernel), the same step with c = h . (1 - z) + c[t - d] . z in that form's roundings.
#pragma once
#include <string>
#include <vector>

#include "lstm_plan.h"
#include "model.h"

namespace rs {

constexpr int kGruMaxCell = 2048;                  // cell dim
constexpr int kGruMaxProj = 4096;                  // recurrent + non-recurrent dim

struct GruLaunchPlan {
  int x_cols = 0, s_cols = 0;      // columns of W_z / W_o: the feed-forward input's (the layer GEMM), the recurrent input's (this kernel)
  int cell_tiles = 0;              // 16-cell tiles: ceil(cell / 16); a wave item = one tile's two gates
  int out_tiles = 0;               // 16-column tiles of y
  int k_s = 0, k_c = 0;            // k extents of the two products, rounded up to four MFMA k-steps (16): recurrent dim, cell dim
  int n_gates = 0, n_out = 0;      // column pitch of the transposed weights: 2 * 16 * cell_tiles, 16 * out_tiles
  int ld_s = 0, ld_c = 0;          // LDS row pitch of the staged s rows / the c . o rows, in floats (k extent + 4: rows on different banks)
  int lds_bytes = 0;
  int rows_per_block = 0;          // kRecChains
};

// Fails (rs::Error) with a message naming the block when a dim is beyond the kernel's limits or the LDS tiles do not fit.
GruLaunchPlan PlanGru(const GruBlock &b, const std::string &name);
// the weights in the kernel's order, zero padded: W_s as [k_s][n_gates] with gate g (0: z, 1: o) of cell c in column 2 c + g (a
// lane's two gate weights of a k-step are one 8-byte load), W_y as [k_c][n_out]
void GruWeightImages(const GruBlock &b, const GruLaunchPlan &p, std::vector<float> *ws_t, std::vector<float> *wy_t);
// "name input=32 cell=32 rec=8 nonrec=8 delay=3 scale=1 norm=0 dropout=0 kernel=gru16x16x4<w8> rows_per_block=16 lds=... grid=chains/16"
std::string DescribeGru(const std::string &name, const GruBlock &b, const GruLaunchPlan &p);

struct GruDev {
  // frame buffers (row 0 of the call's layout, kernels.h) and their pitches
  const float *pre;      // [z | o | hpart], 3 cell
  float *hc;             // [h | c]
  float *y;              // rec + nonrec
  float *st;             // s, rec
  int ld_pre, ld_hc, ld_y, ld_st;
  const float *ws_t, *wy_t, *b_y, *w_h;      // GruWeightImages; b_y: rec + nonrec; w_h: cell
  int cell, rec, out_dim;
  float scale;
  int norm;              // 1: Normalize in front of the scale
  float norm_alpha;      // 1 / (rec * target_rms^2)
  RecWalk walk;          // the call's rows and streams (recurrent_walk.h); a parked state row is [c | s], cell + rec
  GruLaunchPlan plan;
};

}  // namespace rs

// Recurrent blocks around a GruNonlinearityComponent (nnet3's fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer) on the device
// (nnet_pgru.hip): the descriptor the kernel takes by value and the host-only planner that decides, when the model loads, what a
// workgroup keeps in LDS and on which grid.  Nothing here includes a HIP header (tests/host/pgru_plan_check.cc compiles it with g++).
//
// A block (model.h: PgruBlock) per row t, with the delay d, R the recurrent dim:
//   r = Sigmoid(pre_r[t] + W_r,s s[t - d]);  sdotr = r . s[t - d]
//   z = Sigmoid(pre_z[t] + W_z,s s[t - d]);  h = Tanh(pre_h[t] + W_h sdotr);  c = h - z . h + z . c[t - d]
//   y = W_y c + b_y;  s[t] = scale y[0:R]  (norm: scale Normalize(y[0:R]));   without a projection R = cell, s[t] = scale c and
//   c[t - d] is s[t - d]
// pre = [W_z,x; W_r,x; W_hpart] x + b has no dependence on time and is one layer GEMM over all rows.  What is serial is walked by
// this kernel the way nnet_gru.hip walks an OPGRU block (gru_plan.h): a workgroup of kRecWaves waves owns kRecChains chains for
// the whole launch and walks their steps with workgroup barriers only; the grid is the number of chains over kRecChains.
//
// A step has one phase and one barrier more than the OPGRU block's, because h waits for all of r:
//   1. r: a wave item is 16 columns of r for the 16 chains, the accumulator starts from pre_r[t] and takes W_r,s s on
//      v_mfma_f32_16x16x4_f32; r . s[t - d] (one rounding) goes to the sdotr tile in LDS; barrier
//   2. z and h: a wave item is 16 cells, two accumulators -- z from pre_z[t] over the s tile, h from pre_h[t] over the sdotr tile,
//      the two weights of a k are one 8-byte load --, the sigmoid, the tanh and c in the accumulators' registers against c[t - d]
//      (the lane's own store of the step before, or the parked row); c goes to the c tile in LDS (without a projection: scale c
//      goes to the other s tile and the step ends here); barrier
//   3. y = W_y c + b_y, rows to the output buffer, the first R columns scaled into the other s tile and the state buffer; barrier
//   4. norm variant: as gru_plan.h, a wave takes two chains, a fixed tree over the 64 lanes; barrier
// All products are exact FP32 with FP32 accumulation, k in the weight's column order, four per MFMA, whatever the chain's place in
// the tile, the workgroup or the batch -- a row's result is a function of its inputs alone.
//
// LDS: two tiles of s rows, the sdotr tile (pitch k_s + 4 floats each) and, with a projection, the tile of c rows (pitch k_c + 4).
// Without a projection the three tiles are cell wide: 64 * 3 * (k_c + 4) bytes within kRecMaxLdsBytes lets k_c be 752 at most.
//
// The composed form of the same cell (gru-layer / pgru-layer / norm-pgru-layer, model.h: PgruBlock::composed; W_h is then the
// recurrent columns of the affine W_h.UW) shares the descriptor, the planner, the weight images and the limits; it is walked by a
// kernel of its own (nnet_gruc.hip: PgrucKernel), the same phases with c = h . (1 - z) + c[t - d] . z in that form's roundings.
#pragma once
#include <string>
#include <vector>

#include "lstm_plan.h"
#include "model.h"

namespace rs {

constexpr int kPgruMaxCell = 2048;                  // cell dim
constexpr int kPgruMaxProj = 4096;                  // recurrent + non-recurrent dim

struct PgruLaunchPlan {
  int x_cols = 0, s_cols = 0;      // columns of W_z / W_r: the feed-forward input's (the layer GEMM), the recurrent input's (this kernel)
  int cell_tiles = 0;              // 16-cell tiles: ceil(cell / 16); a wave item of phase 2 = one tile's z and h
  int rec_tiles = 0;               // 16-column tiles of r: ceil(R / 16)
  int out_tiles = 0;               // 16-column tiles of y; 0 without a projection
  int k_s = 0, k_c = 0;            // k extents, rounded up to four MFMA k-steps (16): recurrent dim, cell dim
  int n_zh = 0, n_r = 0, n_out = 0;   // column pitch of the transposed weights: 2 * 16 * cell_tiles, 16 * rec_tiles, 16 * out_tiles
  int ld_s = 0, ld_c = 0;          // LDS row pitch of the s / sdotr rows and of the c rows, in floats (k extent + 4); ld_c = 0 without a projection
  int lds_bytes = 0;
  int rows_per_block = 0;          // kRecChains
};

// Fails (rs::Error) with a message naming the block when a dim is beyond the kernel's limits or the LDS tiles do not fit.
PgruLaunchPlan PlanPgru(const PgruBlock &b, const std::string &name);
// the weights in the kernel's order, zero padded: W_r,s as [k_s][n_r]; W_z,s and W_h as [k_s][n_zh] with z's weight of cell c in
// column 2 c and h's in column 2 c + 1 (a lane's two weights of a k-step are one 8-byte load); W_y as [k_c][n_out] (empty without a
// projection)
void PgruWeightImages(const PgruBlock &b, const PgruLaunchPlan &p, std::vector<float> *wr_t, std::vector<float> *wzh_t, std::vector<float> *wy_t);
// "name input=32 cell=32 rec=8 nonrec=8 delay=3 scale=1 norm=0 dropout=0 kernel=pgru16x16x4<w8> rows_per_block=16 lds=... grid=chains/16"
std::string DescribePgru(const std::string &name, const PgruBlock &b, const PgruLaunchPlan &p);

struct PgruDev {
  // frame buffers (row 0 of the call's layout, kernels.h) and their pitches
  const float *pre;      // [z | r | hpart], 2 cell + R
  float *hc;             // [h | c]
  float *y;              // rec + nonrec; null without a projection
  float *st;             // s, R
  int ld_pre, ld_hc, ld_y, ld_st;
  const float *wr_t, *wzh_t, *wy_t, *b_y;      // PgruWeightImages; b_y: rec + nonrec
  int cell, rec, out_dim;                      // rec: R (the cell dim without a projection); out_dim: rec + nonrec, 0 without a projection
  int proj;              // 1: W_y and a state row [c | s]; 0: s = scale c, a state row [s]
  float scale;
  int norm;              // 1: Normalize in front of the scale
  float norm_alpha;      // 1 / (rec * target_rms^2)
  RecWalk walk;          // the call's rows and streams (recurrent_walk.h); a parked state row is [c | s], without a projection [s]
  PgruLaunchPlan plan;
};

}  // namespace rs

// Recurrent blocks of the LSTM cell behind a bottleneck (nnet3's lstmb-layer) on the device (nnet_lstmb.hip): the descriptor the
// kernel takes by value and the host-only planner that decides, when the model loads, what a workgroup keeps in LDS and on which
// grid.  Nothing here includes a HIP header (tests/host/lstmb_plan_check.cc compiles it with g++).
//
// A block (model.h: LstmBlock with bottleneck > 0) per row t, with the delay d, C the cell dim, B the bottleneck dim:
//   b = pre_b[t] + W_a,m sm[t - d];  g = W_b b;  g' = g * so_scale;  g' = g' + so_offset
//   (c, m) = LstmNonlinearity(g', sc[t - d]; params);  sc[t] = scale c;  sm[t] = self_scale (scale m)
// pre_b = W_a,x x has no dependence on time and is a layer GEMM over all rows, B wide, without a bias.  What is serial is walked by
// this kernel the way nnet_lstm.hip walks a fast block (lstm_plan.h): a workgroup of kRecWaves waves owns kRecChains chains for
// the whole launch and walks their steps with workgroup barriers only; the grid is the number of chains over kRecChains.
//
// A step has two phases:
//   A. b: a wave item is 16 columns of b for the 16 chains, the accumulator starts from pre_b[t] and takes W_a,m sm on
//      v_mfma_f32_16x16x4_f32, k over the cell dim in column order (never split: an item's sum is one wave's); b goes to the b tile
//      in LDS; barrier
//   B. the gates: a wave item is the four gates of 16 cells, the accumulators start from zero and take W_b b, k over the bottleneck
//      dim; scale and offset as two roundings, the nonlinearity in the accumulators' registers against sc[t - d] (the lane's own
//      store of the step before, or the parked row); c and m go to the [c | m] buffer, sc and sm to the state buffer, sm into the
//      sm tile (phase A's readers of it are behind the barrier); barrier
// Both products are exact FP32 with FP32 accumulation, k in the weight's column order, four per MFMA, whatever the chain's place in
// the tile, the workgroup or the batch -- a row's result is a function of its inputs alone.
//
// LDS: the tile of sm rows (pitch k_m + 4 floats) and the tile of b rows (pitch k_b + 4).
#pragma once
#include <string>
#include <vector>

#include "lstm_plan.h"
#include "model.h"

namespace rs {

constexpr int kLstmbMaxCell = 2048;                  // cell dim
constexpr int kLstmbMaxBottleneck = 2048;            // bottleneck dim (the LDS bound is the tighter one where both are wide)

struct LstmbLaunchPlan {
  int x_cols = 0, m_cols = 0;      // W_all_a's columns: the feed-forward input's (the layer GEMM), the recurrent input's (this kernel)
  int cell_tiles = 0;              // 16-cell tiles: ceil(cell / 16); a wave item of phase B = one tile's four gates
  int b_tiles = 0;                 // 16-column tiles of b: ceil(bottleneck / 16); a wave item of phase A
  int k_m = 0, k_b = 0;            // k extents of the two products, rounded up to four MFMA k-steps (16): cell dim, bottleneck dim
  int n_b = 0, n_gates = 0;        // column pitch of the transposed weights: 16 * b_tiles, 4 * 16 * cell_tiles
  int ld_m = 0, ld_b = 0;          // LDS row pitch of the sm rows / the b rows, in floats (k extent + 4: rows on different banks)
  int lds_bytes = 0;
  int rows_per_block = 0;          // kRecChains
};

// Fails (rs::Error) with a message naming the block when a dim is beyond the kernel's limits or the two LDS tiles do not fit.
LstmbLaunchPlan PlanLstmb(const LstmBlock &b, const std::string &name);
// the weights in the kernel's order, zero padded: W_a,m as [k_m][n_b]; W_b as [k_b][n_gates] with gate g of cell c in column 4 c + g
// (a lane's four gate weights of a k-step are one 16-byte load, as LstmWeightImages' wr_t)
void LstmbWeightImages(const LstmBlock &b, const LstmbLaunchPlan &p, std::vector<float> *wam_t, std::vector<float> *wb_t);
// "name input=32 cell=32 bottleneck=16 delay=3 scale=1 self_scale=1 kernel=lstmb16x16x4<w8> rows_per_block=16 lds=... grid=chains/16"
std::string DescribeLstmb(const std::string &name, const LstmBlock &b, const LstmbLaunchPlan &p);

struct LstmbDev {
  // frame buffers (row 0 of the call's layout, kernels.h) and their pitches
  const float *pre;      // pre_b, bottleneck wide
  float *cm;             // [c | m]
  float *st;             // [sc | sm]
  int ld_pre, ld_cm, ld_st;
  const float *wam_t, *wb_t;                        // LstmbWeightImages
  const float *so_scale, *so_offset, *params;       // 4 cell each (gate order i, f, c, o); params: 3 x cell
  int cell, bottleneck;
  float scale, self_scale;
  RecWalk walk;          // the call's rows and streams (recurrent_walk.h); a parked state row is [sc | sm], 2 cell
  LstmbLaunchPlan plan;
};

}  // namespace rs

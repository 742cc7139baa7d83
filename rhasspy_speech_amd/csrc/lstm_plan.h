// Recurrent blocks (nnet3's fast-lstmp-layer / fast-lstm-layer) on the device (nnet_lstm.hip): the descriptor the kernel takes by
// value and the host-only planner that decides, when the model loads, which instantiation walks a block, how many chains a
// workgroup owns, what it keeps in LDS and on which grid.  Nothing here includes a HIP header (tests/host/lstm_plan_check.cc compiles
// it with g++).  The composed form of the same cell (lstmp-layer / lstm-layer, model.h: LstmBlock::composed) shares the descriptor, the
// planner and the weight images; it is walked by a kernel of its own (nnet_lstmp.hip) in that form's arithmetic order.
//
// A block (model.h: LstmBlock) per row t, with the delay d:
//   gates = pre[t] + W_r s_r[t - d];  (c, m) = LstmNonlinearity(gates, s_c[t - d]);  rp = W_rp m + b;  s_c[t] = scale c, s_r[t] = scale rp[0:rec]
// pre = W_x x + b has no dependence on time and is a layer GEMM over all rows (W_all's first x_cols columns; the remaining r_cols
// are W_r).  What is serial is walked by this kernel.  Row t needs row t - d only, so the rows of an utterance fall into d
// independent CHAINS, t = first, first + d, first + 2 d, ... (d / stride of them where only every stride-th row is read,
// --frame-subsampling-factor), and the chains of different utterances never meet.  A workgroup owns kRecChains chains for the
// whole launch and walks their steps with workgroup barriers only: no kernel waits for another workgroup, the grid is the number of
// chains over kRecChains whatever the device holds.
//
// A step: the 16 chains' s_r[t - d] rows are in LDS (zero where a chain has no earlier row; the previous step left them there --
// a chain's step n + 1 reads what its step n wrote, so nothing one wave stores to global memory is read by another inside a
// launch), W_r s_r for 16 cells x 4 gates per wave item on v_mfma_f32_16x16x4_f32 (the accumulators start from pre[t]), the
// nonlinearity in the accumulators' registers against s_c[t - d] (the lane's own store of the step before), m into LDS, W_rp m on
// the same instruction, the scaled copies into the state buffer and into the other s_r tile.  Both products are exact FP32 with
// FP32 accumulation; one element's sum runs over k in the order of the weight's columns, four per MFMA, whatever the chain's place
// in the tile, the workgroup or the batch -- a row's result is a function of its inputs alone.
#pragma once
#include <string>
#include <vector>

#include "model.h"

namespace rs {

// (chains and waves of a workgroup and its LDS bound -- here two tiles of s_r rows and the tile of m rows --: recurrent_walk.h)
constexpr int kLstmMaxCell = 2048;             // cell dim (the LDS bound below is the tighter one with a wide recurrent input)
constexpr int kLstmMaxProj = 4096;              // recurrent + non-recurrent projection dim

struct LstmLaunchPlan {
  int x_cols = 0, r_cols = 0;      // W_all's columns: the feed-forward input's (the layer GEMM), the recurrent input's (this kernel)
  int cell_tiles = 0;              // 16-cell tiles: ceil(cell / 16); a wave item = one tile's four gates
  int out_tiles = 0;               // 16-column tiles of rp (0 without a projection)
  int k_r = 0, k_m = 0;            // k extents of the two products, rounded up to four MFMA k-steps (16): recurrent dim, cell dim
  int n_gates = 0, n_out = 0;      // column pitch of the transposed weights: 4 * 16 * cell_tiles, 16 * out_tiles
  int ld_r = 0, ld_m = 0;          // LDS row pitch of the staged s_r rows / the m rows, in floats (k extent + 4: rows on different banks)
  int lds_bytes = 0;
  int rows_per_block = 0;          // kRecChains
};

// Fails (rs::Error) with a message naming the block when a dim is beyond the kernel's limits or the two LDS tiles do not fit.
LstmLaunchPlan PlanLstm(const LstmBlock &b, const std::string &name);
// chains and grid of a launch: RecChainsPerUtt, RecGridX (recurrent_walk.h)
// the weights in the kernel's order, zero padded: W_r as [k_r][n_gates] with gate g of cell c in column 4 c + g (a lane's four gate
// weights of a k-step are one 16-byte load), W_rp as [k_m][n_out]
void LstmWeightImages(const LstmBlock &b, const LstmLaunchPlan &p, std::vector<float> *wr_t, std::vector<float> *wrp_t);
// "name input=32 cell=32 rec=8 nonrec=8 delay=3 scale=1 dropout_mask=0 kernel=lstm16x16x4<w8> rows_per_block=16 lds=... grid=chains/16"
std::string DescribeLstm(const std::string &name, const LstmBlock &b, const LstmLaunchPlan &p);
// the line of a block in its composed form (lstmp-layer / lstm-layer; the same plan, walked by nnet_lstmp.hip):
// "name input=32 cell=32 rec=8 nonrec=8 delay=3 scale_c=1 scale_r=1 dropout=0 kernel=lstmp16x16x4<w8> rows_per_block=16 lds=... grid=chains/16"
std::string DescribeLstmp(const std::string &name, const LstmBlock &b, const LstmLaunchPlan &p);

struct LstmDev {
  // frame buffers (row 0 of the call's layout, kernels.h) and their pitches
  const float *pre;      // 4 cell
  float *cm;             // [c | m]
  float *rp;             // rec + nonrec; null without a projection
  float *st;             // [s_c | s_r]
  int ld_pre, ld_cm, ld_rp, ld_st;
  const float *wr_t, *wrp_t, *b_rp, *params;      // LstmWeightImages; params: 3 x cell
  int cell, rec_dim, out_dim, rec;                // rec_dim: width of s_r; out_dim / rec: rp's width and its recurrent part (0 without a projection)
  float scale;
  float scale_r;         // the composed form only (nnet_lstmp.hip): `scale` is the cell's truncation component's, this the recurrent state's
  RecWalk walk;          // the call's rows and streams (recurrent_walk.h); a parked state row is [s_c | s_r], cell + rec_dim
  LstmLaunchPlan plan;
};

}  // namespace rs

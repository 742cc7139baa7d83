// See lstm_plan.h.
#include "lstm_plan.h"

#include <sstream>

namespace rs {

LstmLaunchPlan PlanLstm(const LstmBlock &b, const std::string &name) {
  const std::string what = "nnet3: recurrent block " + name + ": ";
  if (b.cell <= 0 || b.in_dim <= 0 || b.rec < 0 || b.nonrec < 0 || (b.rec == 0 && b.nonrec != 0)) Fail(what + "bad dimensions");
  if (b.delay < 1 || b.delay > kLstmMaxDelay) Fail(what + "a delay of " + std::to_string(b.delay) + " frames; the HIP kernel takes 1 to " + std::to_string(kLstmMaxDelay));
  if (b.cell > kLstmMaxCell) Fail(what + "cell dim " + std::to_string(b.cell) + " is more than the " + std::to_string(kLstmMaxCell) + " the HIP kernel takes");
  if (b.rec + b.nonrec > kLstmMaxProj)
    Fail(what + "projection dim " + std::to_string(b.rec + b.nonrec) + " (recurrent + non-recurrent) is more than the " + std::to_string(kLstmMaxProj) + " the HIP kernel takes");
  LstmLaunchPlan p;
  p.x_cols = b.in_dim;
  p.r_cols = b.RecDim();
  p.cell_tiles = (b.cell + 15) / 16;
  p.out_tiles = b.proj() ? (b.rec + b.nonrec + 15) / 16 : 0;
  p.k_r = (p.r_cols + 15) / 16 * 16;
  p.k_m = 16 * p.cell_tiles;
  p.n_gates = 4 * 16 * p.cell_tiles;
  p.n_out = 16 * p.out_tiles;
  p.ld_r = p.k_r + 4;
  p.ld_m = p.k_m + 4;
  p.rows_per_block = kRecChains;
  // two tiles of s_r rows (the one a step reads, the one it writes for the next step) and, with a projection, the tile of m rows
  const long lds = (long)kRecChains * (2 * p.ld_r + (b.proj() ? p.ld_m : 0)) * (long)sizeof(float);
  if (lds > kRecMaxLdsBytes)
    Fail(what + "the state and output rows of " + std::to_string(kRecChains) + " chains (cell dim " + std::to_string(b.cell) + " + recurrent dim " +
         std::to_string(p.r_cols) + ", " + std::to_string(lds) + " bytes) do not fit the " + std::to_string(kRecMaxLdsBytes) +
         " bytes of LDS the HIP kernel keeps them in");
  p.lds_bytes = (int)lds;
  return p;
}

void LstmWeightImages(const LstmBlock &b, const LstmLaunchPlan &p, std::vector<float> *wr_t, std::vector<float> *wrp_t) {
  const int C = b.cell;
  wr_t->assign((size_t)p.k_r * p.n_gates, 0.0f);
  for (int g = 0; g < 4; g++)
    for (int c = 0; c < C; c++)
      for (int k = 0; k < p.r_cols; k++) (*wr_t)[(size_t)k * p.n_gates + 4 * c + g] = b.W_r(g * C + c, k);
  wrp_t->assign((size_t)p.k_m * p.n_out, 0.0f);
  if (b.proj())
    for (int n = 0; n < b.rec + b.nonrec; n++)
      for (int k = 0; k < C; k++) (*wrp_t)[(size_t)k * p.n_out + n] = b.W_rp(n, k);
}

std::string DescribeLstm(const std::string &name, const LstmBlock &b, const LstmLaunchPlan &p) {
  std::ostringstream os;
  os << name << " input=" << b.in_dim << " cell=" << b.cell << " rec=" << b.rec << " nonrec=" << b.nonrec << " delay=" << b.delay << " scale=" << b.scale
     << " dropout_mask=" << (b.dropout_mask ? 1 : 0) << " kernel=lstm16x16x4<w" << kRecWaves << "> rows_per_block=" << p.rows_per_block << " lds=" << p.lds_bytes
     << " w_all=" << p.x_cols << "+" << p.r_cols << " cell_tiles=" << p.cell_tiles << " out_tiles=" << p.out_tiles << " grid=chains/" << p.rows_per_block;
  return os.str();
}

std::string DescribeLstmp(const std::string &name, const LstmBlock &b, const LstmLaunchPlan &p) {
  std::ostringstream os;
  os << name << " input=" << b.in_dim << " cell=" << b.cell << " rec=" << b.rec << " nonrec=" << b.nonrec << " delay=" << b.delay << " scale_c=" << b.scale
     << " scale_r=" << b.scale_r << " dropout=" << (b.dropout ? 1 : 0) << " kernel=lstmp16x16x4<w" << kRecWaves << "> rows_per_block=" << p.rows_per_block
     << " lds=" << p.lds_bytes << " w_x=" << p.x_cols << " w_r=" << p.r_cols << " cell_tiles=" << p.cell_tiles << " out_tiles=" << p.out_tiles
     << " grid=chains/" << p.rows_per_block;
  return os.str();
}

}  // namespace rs

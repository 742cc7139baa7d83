// See lstmb_plan.h.
#include "lstmb_plan.h"

#include <sstream>

namespace rs {

LstmbLaunchPlan PlanLstmb(const LstmBlock &b, const std::string &name) {
  const std::string what = "nnet3: recurrent block " + name + ": ";
  if (b.cell <= 0 || b.in_dim <= 0 || b.bottleneck <= 0 || b.rec != 0 || b.nonrec != 0) Fail(what + "bad dimensions");
  if (b.delay < 1 || b.delay > kLstmMaxDelay) Fail(what + "a delay of " + std::to_string(b.delay) + " frames; the HIP kernel takes 1 to " + std::to_string(kLstmMaxDelay));
  if (b.cell > kLstmbMaxCell) Fail(what + "cell dim " + std::to_string(b.cell) + " is more than the " + std::to_string(kLstmbMaxCell) + " the HIP kernel takes");
  if (b.bottleneck > kLstmbMaxBottleneck)
    Fail(what + "bottleneck dim " + std::to_string(b.bottleneck) + " is more than the " + std::to_string(kLstmbMaxBottleneck) + " the HIP kernel takes");
  LstmbLaunchPlan p;
  p.x_cols = b.in_dim;
  p.m_cols = b.cell;
  p.cell_tiles = (b.cell + 15) / 16;
  p.b_tiles = (b.bottleneck + 15) / 16;
  p.k_m = 16 * p.cell_tiles;
  p.k_b = 16 * p.b_tiles;
  p.n_b = 16 * p.b_tiles;
  p.n_gates = 4 * 16 * p.cell_tiles;
  p.ld_m = p.k_m + 4;
  p.ld_b = p.k_b + 4;
  p.rows_per_block = kRecChains;
  // the tile of sm rows and the tile of b rows
  const long lds = (long)kRecChains * (p.ld_m + p.ld_b) * (long)sizeof(float);
  if (lds > kRecMaxLdsBytes)
    Fail(what + "the state and bottleneck rows of " + std::to_string(kRecChains) + " chains (cell dim " + std::to_string(b.cell) + " + bottleneck dim " +
         std::to_string(b.bottleneck) + ", " + std::to_string(lds) + " bytes) do not fit the " + std::to_string(kRecMaxLdsBytes) +
         " bytes of LDS the HIP kernel keeps them in");
  p.lds_bytes = (int)lds;
  return p;
}

void LstmbWeightImages(const LstmBlock &b, const LstmbLaunchPlan &p, std::vector<float> *wam_t, std::vector<float> *wb_t) {
  const int C = b.cell, B = b.bottleneck;
  wam_t->assign((size_t)p.k_m * p.n_b, 0.0f);
  for (int n = 0; n < B; n++)
    for (int k = 0; k < C; k++) (*wam_t)[(size_t)k * p.n_b + n] = b.W_r(n, k);
  wb_t->assign((size_t)p.k_b * p.n_gates, 0.0f);
  for (int g = 0; g < 4; g++)
    for (int c = 0; c < C; c++)
      for (int k = 0; k < B; k++) (*wb_t)[(size_t)k * p.n_gates + 4 * c + g] = b.W_b(g * C + c, k);
}

std::string DescribeLstmb(const std::string &name, const LstmBlock &b, const LstmbLaunchPlan &p) {
  std::ostringstream os;
  os << name << " input=" << b.in_dim << " cell=" << b.cell << " bottleneck=" << b.bottleneck << " delay=" << b.delay << " scale=" << b.scale
     << " self_scale=" << b.self_scale << " kernel=lstmb16x16x4<w" << kRecWaves << "> rows_per_block=" << p.rows_per_block << " lds=" << p.lds_bytes
     << " w_a=" << p.x_cols << "+" << p.m_cols << " cell_tiles=" << p.cell_tiles << " b_tiles=" << p.b_tiles << " grid=chains/" << p.rows_per_block;
  return os.str();
}

}  // namespace rs

// See gru_plan.h.
#include "gru_plan.h"

#include <sstream>

namespace rs {

GruLaunchPlan PlanGru(const GruBlock &b, const std::string &name) {
  const std::string what = "nnet3: recurrent block " + name + ": ";
  if (b.cell <= 0 || b.in_dim <= 0 || b.rec <= 0 || b.nonrec < 0) Fail(what + "bad dimensions");
  if (b.delay < 1 || b.delay > kLstmMaxDelay) Fail(what + "a delay of " + std::to_string(b.delay) + " frames; the HIP kernel takes 1 to " + std::to_string(kLstmMaxDelay));
  if (b.cell > kGruMaxCell) Fail(what + "cell dim " + std::to_string(b.cell) + " is more than the " + std::to_string(kGruMaxCell) + " the HIP kernel takes");
  if (b.rec + b.nonrec > kGruMaxProj)
    Fail(what + "output dim " + std::to_string(b.rec + b.nonrec) + " (recurrent + non-recurrent) is more than the " + std::to_string(kGruMaxProj) + " the HIP kernel takes");
  GruLaunchPlan p;
  p.x_cols = b.in_dim;
  p.s_cols = b.rec;
  p.cell_tiles = (b.cell + 15) / 16;
  p.out_tiles = (b.rec + b.nonrec + 15) / 16;
  p.k_s = (b.rec + 15) / 16 * 16;
  p.k_c = 16 * p.cell_tiles;
  p.n_gates = 2 * 16 * p.cell_tiles;
  p.n_out = 16 * p.out_tiles;
  p.ld_s = p.k_s + 4;
  p.ld_c = p.k_c + 4;
  p.rows_per_block = kRecChains;
  // two tiles of s rows (the one a step reads, the one it writes for the next step) and the tile of c . o rows
  const long lds = (long)kRecChains * (2 * p.ld_s + p.ld_c) * (long)sizeof(float);
  if (lds > kRecMaxLdsBytes)
    Fail(what + "the state and product rows of " + std::to_string(kRecChains) + " chains (cell dim " + std::to_string(b.cell) + " + recurrent dim " +
         std::to_string(b.rec) + ", " + std::to_string(lds) + " bytes) do not fit the " + std::to_string(kRecMaxLdsBytes) +
         " bytes of LDS the HIP kernel keeps them in");
  p.lds_bytes = (int)lds;
  return p;
}

void GruWeightImages(const GruBlock &b, const GruLaunchPlan &p, std::vector<float> *ws_t, std::vector<float> *wy_t) {
  const int C = b.cell;
  ws_t->assign((size_t)p.k_s * p.n_gates, 0.0f);
  for (int g = 0; g < 2; g++)
    for (int c = 0; c < C; c++)
      for (int k = 0; k < p.s_cols; k++) (*ws_t)[(size_t)k * p.n_gates + 2 * c + g] = b.W_s(g * C + c, k);
  wy_t->assign((size_t)p.k_c * p.n_out, 0.0f);
  for (int n = 0; n < b.rec + b.nonrec; n++)
    for (int k = 0; k < C; k++) (*wy_t)[(size_t)k * p.n_out + n] = b.W_y(n, k);
}

std::string DescribeGru(const std::string &name, const GruBlock &b, const GruLaunchPlan &p) {
  std::ostringstream os;
  os << name << " input=" << b.in_dim << " cell=" << b.cell << " rec=" << b.rec << " nonrec=" << b.nonrec << " delay=" << b.delay << " scale=" << b.scale
     << " norm=" << (b.norm ? 1 : 0) << " dropout=" << (b.dropout ? 1 : 0) << " kernel=" << (b.composed ? "gruc" : "gru") << "16x16x4<w" << kRecWaves << "> rows_per_block=" << p.rows_per_block
     << " lds=" << p.lds_bytes << " w_zo=" << p.x_cols << "+" << p.s_cols << " cell_tiles=" << p.cell_tiles << " out_tiles=" << p.out_tiles << " grid=chains/"
     << p.rows_per_block;
  if (b.composed) os << " form=composed";      // (opgru-layer / norm-opgru-layer: walked by nnet_gruc.hip on the same plan)
  return os.str();
}

}  // namespace rs

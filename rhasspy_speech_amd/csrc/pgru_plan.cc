// See pgru_plan.h.
#include "pgru_plan.h"

#include <sstream>

namespace rs {

PgruLaunchPlan PlanPgru(const PgruBlock &b, const std::string &name) {
  const std::string what = "nnet3: recurrent block " + name + ": ";
  if (b.cell <= 0 || b.in_dim <= 0 || b.rec < 0 || b.nonrec < 0 || (b.rec == 0 && b.nonrec != 0)) Fail(what + "bad dimensions");
  if (b.delay < 1 || b.delay > kLstmMaxDelay) Fail(what + "a delay of " + std::to_string(b.delay) + " frames; the HIP kernel takes 1 to " + std::to_string(kLstmMaxDelay));
  if (b.cell > kPgruMaxCell) Fail(what + "cell dim " + std::to_string(b.cell) + " is more than the " + std::to_string(kPgruMaxCell) + " the HIP kernel takes");
  if (b.rec + b.nonrec > kPgruMaxProj)
    Fail(what + "output dim " + std::to_string(b.rec + b.nonrec) + " (recurrent + non-recurrent) is more than the " + std::to_string(kPgruMaxProj) + " the HIP kernel takes");
  const int R = b.RecDim();
  PgruLaunchPlan p;
  p.x_cols = b.in_dim;
  p.s_cols = R;
  p.cell_tiles = (b.cell + 15) / 16;
  p.rec_tiles = (R + 15) / 16;
  p.out_tiles = b.proj() ? (b.rec + b.nonrec + 15) / 16 : 0;
  p.k_s = 16 * p.rec_tiles;
  p.k_c = 16 * p.cell_tiles;
  p.n_zh = 2 * 16 * p.cell_tiles;
  p.n_r = 16 * p.rec_tiles;
  p.n_out = 16 * p.out_tiles;
  p.ld_s = p.k_s + 4;
  p.ld_c = b.proj() ? p.k_c + 4 : 0;
  p.rows_per_block = kRecChains;
  // two tiles of s rows (the one a step reads, the one it writes for the next step), the tile of r . s rows and, with a projection,
  // the tile of c rows
  const long lds = (long)kRecChains * (3 * p.ld_s + p.ld_c) * (long)sizeof(float);
  if (lds > kRecMaxLdsBytes)
    Fail(what + "the state, product and cell rows of " + std::to_string(kRecChains) + " chains (cell dim " + std::to_string(b.cell) + ", recurrent dim " +
         std::to_string(R) + ", " + std::to_string(lds) + " bytes) do not fit the " + std::to_string(kRecMaxLdsBytes) +
         " bytes of LDS the HIP kernel keeps them in");
  p.lds_bytes = (int)lds;
  return p;
}

void PgruWeightImages(const PgruBlock &b, const PgruLaunchPlan &p, std::vector<float> *wr_t, std::vector<float> *wzh_t, std::vector<float> *wy_t) {
  const int C = b.cell, R = b.RecDim();
  wr_t->assign((size_t)p.k_s * p.n_r, 0.0f);
  for (int n = 0; n < R; n++)
    for (int k = 0; k < R; k++) (*wr_t)[(size_t)k * p.n_r + n] = b.W_rs(n, k);
  wzh_t->assign((size_t)p.k_s * p.n_zh, 0.0f);
  for (int c = 0; c < C; c++)
    for (int k = 0; k < R; k++) {
      (*wzh_t)[(size_t)k * p.n_zh + 2 * c] = b.W_zs(c, k);
      (*wzh_t)[(size_t)k * p.n_zh + 2 * c + 1] = b.W_h(c, k);
    }
  wy_t->assign((size_t)p.k_c * p.n_out, 0.0f);
  for (int n = 0; n < b.rec + b.nonrec; n++)
    for (int k = 0; k < C; k++) (*wy_t)[(size_t)k * p.n_out + n] = b.W_y(n, k);
}

std::string DescribePgru(const std::string &name, const PgruBlock &b, const PgruLaunchPlan &p) {
  std::ostringstream os;
  os << name << " input=" << b.in_dim << " cell=" << b.cell << " rec=" << b.rec << " nonrec=" << b.nonrec << " delay=" << b.delay << " scale=" << b.scale
     << " norm=" << (b.norm ? 1 : 0) << " dropout=" << (b.dropout ? 1 : 0) << " kernel=" << (b.composed ? "pgruc" : "pgru") << "16x16x4<w" << kRecWaves << "> rows_per_block=" << p.rows_per_block
     << " lds=" << p.lds_bytes << " w_zr=" << p.x_cols << "+" << p.s_cols << " cell_tiles=" << p.cell_tiles << " rec_tiles=" << p.rec_tiles
     << " out_tiles=" << p.out_tiles << " grid=chains/" << p.rows_per_block;
  if (b.composed) os << " form=composed";      // (gru-layer / pgru-layer / norm-pgru-layer: walked by nnet_gruc.hip on the same plan)
  return os.str();
}

}  // namespace rs

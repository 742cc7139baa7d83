// See conv_plan.h.
#include "conv_plan.h"

#include <algorithm>
#include <sstream>

namespace rs {

ConvLaunchPlan PlanConv(const ConvGeom &g, const std::string &name) {
  const std::string what = "nnet3: convolution " + name + ": ";
  ConvLaunchPlan p;
  if ((int)g.time_offsets.size() > kConvMaxTimeOffsets)
    Fail(what + std::to_string(g.time_offsets.size()) + " distinct time offsets; the HIP convolution kernel takes at most " + std::to_string(kConvMaxTimeOffsets));
  int dh_min = 0, dh_max = 0;
  for (size_t i = 0; i < g.offsets.size(); i++) {
    dh_min = i == 0 ? g.offsets[i].second : std::min(dh_min, g.offsets[i].second);
    dh_max = i == 0 ? g.offsets[i].second : std::max(dh_max, g.offsets[i].second);
  }
  p.pad_lo = std::max(0, -dh_min);
  p.pad_hi = std::max(0, (g.height_out - 1) * g.height_sub + dh_max - (g.height_in - 1));
  p.hp = p.pad_lo + g.height_in + p.pad_hi;
  p.fs = g.filters_in | 1;
  p.slot = p.hp * p.fs;
  p.k = g.K();
  p.k_pad = (p.k + 3) / 4 * 4;
  const int n_tiles = (g.filters_out + 15) / 16;
  p.nacc = n_tiles >= 4 ? 4 : n_tiles >= 2 ? 2 : 1;
  p.n_pad = (n_tiles + p.nacc - 1) / p.nacc * p.nacc * 16;
  p.n_chunks = p.n_pad / (16 * p.nacc);
  // as many frames as two 16-pixel tiles per wave and the LDS budget allow
  const long row_bytes = (long)g.time_offsets.size() * p.slot * (long)sizeof(float);
  if (row_bytes > kConvMaxLdsBytes)
    Fail(what + "the input rows of one frame (" + std::to_string(g.time_offsets.size()) + " time offsets x " + std::to_string(p.hp) + " heights x " +
         std::to_string(g.filters_in) + " filters, " + std::to_string(row_bytes) + " bytes) do not fit the " + std::to_string(kConvMaxLdsBytes) +
         " bytes of LDS the HIP convolution kernel stages them in");
  const int max_tiles = kConvWaves * 2;
  if ((g.height_out + 15) / 16 > max_tiles)
    Fail(what + "height_out " + std::to_string(g.height_out) + " is more than the " + std::to_string(16 * max_tiles) + " pixels a workgroup of the HIP convolution kernel covers");
  int tr = 1;
  while (tr < 16 && ((tr + 1) * g.height_out + 15) / 16 <= max_tiles && (tr + 1) * row_bytes <= kConvMaxLdsBytes) tr++;
  p.rows_per_block = tr;
  p.m_tiles = (tr * g.height_out + 15) / 16;
  p.mpw = p.m_tiles > kConvWaves ? 2 : 1;
  p.lds_bytes = (int)(tr * row_bytes);
  return p;
}

void ConvWeightImage(const ConvGeom &g, const ConvLaunchPlan &p, const MatF &W, std::vector<float> *wt, std::vector<int> *koff) {
  wt->assign((size_t)p.k_pad * p.n_pad, 0.0f);
  koff->assign(p.k_pad, 0);
  for (size_t o = 0; o < g.offsets.size(); o++) {
    const int ti = (int)(std::lower_bound(g.time_offsets.begin(), g.time_offsets.end(), g.offsets[o].first) - g.time_offsets.begin());
    for (int f = 0; f < g.filters_in; f++) {
      const int k = (int)o * g.filters_in + f;
      (*koff)[k] = (ti * p.hp + g.offsets[o].second + p.pad_lo) * p.fs + f;
      for (int n = 0; n < g.filters_out; n++) (*wt)[(size_t)k * p.n_pad + n] = W(n, k);
    }
  }
}

std::string DescribeConv(const std::string &name, const ConvGeom &g, const ConvLaunchPlan &p) {
  std::ostringstream os;
  os << name << " filters=" << g.filters_in << "->" << g.filters_out << " heights=" << g.height_in << "->" << g.height_out << " sub=" << g.height_sub
     << " offsets=" << g.offsets.size() << " time_offsets=" << g.time_offsets.size() << " k=" << p.k << " kernel=conv16x16x4<m" << p.mpw << ",n" << p.nacc
     << "> rows_per_block=" << p.rows_per_block << " pixel_tiles=" << p.m_tiles << " pad=" << p.pad_lo << "," << p.pad_hi << " lds=" << p.lds_bytes
     << " filter_chunks=" << p.n_chunks << " grid=rows/" << p.rows_per_block;
  return os.str();
}

}  // namespace rs

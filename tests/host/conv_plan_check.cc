// Host-only check of the convolution reader and planner (rhasspy_speech_amd/csrc/model.{h,cc}, conv_plan.{h,cc}): reads the
// final.mdl files named on the command line, compiles their networks and plans every convolution the way the model load does,
// built by tests/test_conv_cpu.py under the address and undefined-behaviour sanitizers.  Arguments: pairs of <case name> <path of
// final.mdl>.  Per convolution one line `<case> <DescribeConv's text>` after the plan and the weight image have been walked the way
// the kernel walks them (every LDS address a pixel of the tile can form inside the staged bytes, every table entry inside one staged
// frame, every weight of the model in the image exactly once, the tile inside the workgroup's waves); `<case> error: <message>` when
// the reader, the compiler or the planner refuses the model.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/conv_plan.h"
#include "../../rhasspy_speech_amd/csrc/model.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "conv_plan_check: %s\n", what); std::exit(2); }
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: conv_plan_check <name> <final.mdl> ...");
  for (int a = 1; a + 1 < argc; a += 2) {
    const std::string name = argv[a], path = argv[a + 1];
    try {
      rs::AcousticModel am;
      am.Read(path);
      int convs = 0;
      for (const rs::LayerOp &op : am.nnet.ops) {
        if (op.kind == rs::LayerOp::kGather) {
          Require((int)op.gather_part.size() == op.out_dim && (int)op.gather_col.size() == op.out_dim, "gather table size");
          for (int i = 0; i < op.out_dim; i++) {
            Require(op.gather_part[i] >= 0 && op.gather_part[i] < (int)op.terms.size(), "gather part");
            const rs::SumTerm &t = op.terms[op.gather_part[i]];
            Require(op.gather_col[i] >= 0 && t.src_col + op.gather_col[i] < am.nnet.bufs[t.src_buf].dim, "gather column outside its source");
          }
        }
        if (op.kind != rs::LayerOp::kConv) continue;
        convs++;
        const rs::ConvGeom &g = op.conv;
        const rs::ConvLaunchPlan p = rs::PlanConv(g, op.name);
        Require(op.terms.size() == g.time_offsets.size() && (int)op.terms.size() <= rs::kConvMaxTimeOffsets, "one term per time offset");
        Require(p.mpw >= 1 && p.mpw <= 2 && (p.nacc == 1 || p.nacc == 2 || p.nacc == 4), "instantiation");
        Require(p.m_tiles >= 1 && p.m_tiles <= rs::kConvWaves * p.mpw && p.m_tiles * 16 >= p.rows_per_block * g.height_out, "pixel tiles");
        Require(p.n_pad % (16 * p.nacc) == 0 && p.n_pad >= g.filters_out && p.n_chunks * 16 * p.nacc == p.n_pad, "filter tiles");
        Require(p.k == g.K() && p.k_pad % 4 == 0 && p.k_pad >= p.k && p.k_pad < p.k + 4, "k padding");
        const long lds_floats = (long)p.rows_per_block * (long)g.time_offsets.size() * p.slot;
        Require(p.lds_bytes == lds_floats * 4 && p.lds_bytes <= rs::kConvMaxLdsBytes && p.slot == p.hp * p.fs && p.fs >= g.filters_in, "LDS size");
        std::vector<float> wt;
        std::vector<int> koff;
        rs::ConvWeightImage(g, p, op.W, &wt, &koff);
        Require((long)wt.size() == (long)p.k_pad * p.n_pad && (int)koff.size() == p.k_pad, "image size");
        const long frame = (long)g.time_offsets.size() * p.slot;
        for (int k = 0; k < p.k_pad; k++) Require(koff[k] >= 0 && koff[k] < frame, "table entry outside a staged frame");
        for (int j = 0; j < p.rows_per_block; j++)
          for (int h = 0; h < g.height_out; h++) {
            const long base = j * frame + (long)h * g.height_sub * p.fs;
            for (int k = 0; k < p.k; k++) Require(base + koff[k] >= 0 && base + koff[k] < lds_floats, "LDS address outside the staged bytes");
          }
        long nz_model = 0, nz_image = 0;
        for (float w : op.W.d) nz_model += w != 0.0f;
        for (float w : wt) nz_image += w != 0.0f;
        Require(nz_model == nz_image, "the image's padding is not zero");
        for (int k = 0; k < p.k; k++)
          for (int n = 0; n < g.filters_out; n++) Require(wt[(size_t)k * p.n_pad + n] == op.W(n, k), "weight in the wrong place");
        std::printf("%s %s\n", name.c_str(), rs::DescribeConv(op.name, g, p).c_str());
      }
      if (convs == 0) std::printf("%s no convolution\n", name.c_str());
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}

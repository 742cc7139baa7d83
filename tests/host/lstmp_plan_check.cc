// Host-only check of the reader's recogniser and lowering of the composed LSTM(P) block (lstmp-layer / lstm-layer;
// rhasspy_speech_amd/csrc/model.{h,cc}, nnet3_setup.cc) and of the plan it shares with the fast block (lstm_plan.{h,cc}): reads the
// final.mdl files named on the command line, compiles their networks and plans every recurrent block the way the model load does,
// built by tests/test_lstmp_cpu.py under the address and undefined-behaviour sanitizers.  Arguments: pairs of <case name> <path of
// final.mdl>.  Per block, in network order, one line `<case> lstmp: <DescribeLstmp's text>` (a fast block: `<case> lstm: ...`) after
// the lowering has been walked (the stacked layer GEMM in front, four gate row blocks of W_r, three peephole rows, the buffers of
// equal extent) and the weight images have been compared element by element; `<case> error: <message>` when the reader, the
// compiler or the planner refuses the model.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/lstm_plan.h"
#include "../../rhasspy_speech_amd/csrc/model.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "lstmp_plan_check: %s\n", what); std::exit(2); }
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: lstmp_plan_check <name> <final.mdl> ...");
  for (int a = 1; a + 1 < argc; a += 2) {
    const std::string name = argv[a], path = argv[a + 1];
    try {
      rs::AcousticModel am;
      am.Read(path);
      const rs::Nnet &nn = am.nnet;
      int blocks = 0;
      for (size_t i = 0; i < nn.ops.size(); i++) {
        const rs::LayerOp &op = nn.ops[i];
        if (op.kind != rs::LayerOp::kLstm && op.kind != rs::LayerOp::kLstmp) continue;
        blocks++;
        const rs::LstmBlock &k = op.lstm;
        const bool composed = op.kind == rs::LayerOp::kLstmp;
        Require(k.composed == composed, "the block's form and the op's kind");
        const rs::LstmLaunchPlan p = rs::PlanLstm(k, op.name);
        // the stacked feed-forward columns are the layer GEMM in front of the walk, with the four biases; its output is what the walk reads
        Require(i > 0 && nn.ops[i - 1].kind == rs::LayerOp::kGemm && nn.ops[i - 1].out_buf == k.pre_buf && nn.ops[i - 1].W.cols == p.x_cols &&
                    nn.ops[i - 1].W.rows == 4 * k.cell, "the stacked layer GEMM of the feed-forward columns");
        Require(!composed || (int)nn.ops[i - 1].bias.size() == 4 * k.cell, "the stacked biases");
        Require(p.x_cols == k.in_dim && p.r_cols == k.RecDim() && k.W_r.rows == 4 * k.cell && k.W_r.cols == p.r_cols, "the recurrent columns");
        Require(k.params.rows == 3 && k.params.cols == k.cell && (long)k.params.d.size() == 3L * k.cell, "the peephole rows");
        Require(k.delay >= 1 && k.delay <= rs::kLstmMaxDelay && k.need_lext >= 0 && k.need_lext <= nn.bufs[k.pre_buf].lext, "delay / extents");
        const int bufs[4] = {k.pre_buf, k.cm_buf, k.st_buf, k.rp_buf};
        const int dims[4] = {4 * k.cell, 2 * k.cell, k.cell + k.RecDim(), k.rec + k.nonrec};
        for (int b = 0; b < 4; b++) {
          if (bufs[b] < 0) { Require(b == 3 && !k.proj(), "a missing buffer"); continue; }
          const rs::BufferInfo &bi = nn.bufs[bufs[b]], &b0 = nn.bufs[k.pre_buf];
          Require(bi.dim == dims[b] && bi.lext == b0.lext && bi.rext == b0.rext && bi.stride == b0.stride, "the block's buffers hold the same rows");
        }
        const long lds_floats = (long)rs::kRecChains * (2 * p.ld_r + (k.proj() ? p.ld_m : 0));
        Require(p.lds_bytes == lds_floats * 4 && p.lds_bytes <= rs::kRecMaxLdsBytes && p.rows_per_block == rs::kRecChains, "LDS size");
        Require(16 * p.cell_tiles >= p.k_m && (k.proj() || 16 * p.cell_tiles >= p.k_r), "a tile's padding columns are written");
        std::vector<float> wr_t, wrp_t;
        rs::LstmWeightImages(k, p, &wr_t, &wrp_t);
        Require((long)wr_t.size() == (long)p.k_r * p.n_gates && (long)wrp_t.size() == (long)p.k_m * p.n_out, "image sizes");
        for (int g = 0; g < 4; g++)
          for (int c = 0; c < k.cell; c++)
            for (int kk = 0; kk < p.r_cols; kk++)
              Require(wr_t[(size_t)kk * p.n_gates + 4 * c + g] == k.W_r(g * k.cell + c, kk), "W_r weight in the wrong place");
        if (k.proj()) {
          Require(k.W_rp.rows == k.rec + k.nonrec && k.W_rp.cols == k.cell && (int)k.b_rp.size() == k.W_rp.rows, "projection dims");
          for (int n = 0; n < k.W_rp.rows; n++)
            for (int kk = 0; kk < k.cell; kk++) Require(wrp_t[(size_t)kk * p.n_out + n] == k.W_rp(n, kk), "W_rp weight in the wrong place");
        }
        if (composed) std::printf("%s lstmp: %s\n", name.c_str(), rs::DescribeLstmp(op.name, k, p).c_str());
        else std::printf("%s lstm: %s\n", name.c_str(), rs::DescribeLstm(op.name, k, p).c_str());
      }
      if (blocks == 0) std::printf("%s no recurrent block\n", name.c_str());
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}

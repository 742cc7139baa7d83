// Host-only check of the reader's recogniser and lowering of the LSTM block behind a bottleneck (lstmb-layer;
// rhasspy_speech_amd/csrc/model.{h,cc}, nnet3_setup.cc) and of its planner (lstmb_plan.{h,cc}): reads the final.mdl files named on
// the command line, compiles their networks and plans every recurrent block the way the model load does, built by
// tests/test_lstmb_cpu.py under the address and undefined-behaviour sanitizers.  Arguments: pairs of <case name> <path of final.mdl>.
// Per block, in network order, one line `<case> lstmb: <DescribeLstmb's text>` (a fast block: `<case> lstm: ...`, a composed one:
// `<case> lstmp: ...`) after the lowering has been walked (the bottleneck-wide layer GEMM without a bias in front, W_all_a's
// recurrent columns, W_all_b, the scale / offset vectors with EnsureNonzero applied, the buffers of equal extent) and the weight
// images have been compared element by element; `<case> error: <message>` when the reader, the compiler or the planner refuses
// the model.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/lstm_plan.h"
#include "../../rhasspy_speech_amd/csrc/lstmb_plan.h"
#include "../../rhasspy_speech_amd/csrc/model.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "lstmb_plan_check: %s\n", what); std::exit(2); }
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: lstmb_plan_check <name> <final.mdl> ...");
  for (int a = 1; a + 1 < argc; a += 2) {
    const std::string name = argv[a], path = argv[a + 1];
    try {
      rs::AcousticModel am;
      am.Read(path);
      const rs::Nnet &nn = am.nnet;
      int blocks = 0;
      for (size_t i = 0; i < nn.ops.size(); i++) {
        const rs::LayerOp &op = nn.ops[i];
        if (op.kind == rs::LayerOp::kLstm || op.kind == rs::LayerOp::kLstmp) {
          blocks++;
          Require(op.lstm.bottleneck == 0, "a fast or composed block has no bottleneck");
          const rs::LstmLaunchPlan p = rs::PlanLstm(op.lstm, op.name);
          if (op.kind == rs::LayerOp::kLstmp) std::printf("%s lstmp: %s\n", name.c_str(), rs::DescribeLstmp(op.name, op.lstm, p).c_str());
          else std::printf("%s lstm: %s\n", name.c_str(), rs::DescribeLstm(op.name, op.lstm, p).c_str());
          continue;
        }
        if (op.kind != rs::LayerOp::kLstmb) continue;
        blocks++;
        const rs::LstmBlock &k = op.lstm;
        const int C = k.cell, B = k.bottleneck;
        Require(B > 0 && !k.composed && k.rec == 0 && k.nonrec == 0 && k.rp_buf < 0, "the block's form");
        const rs::LstmbLaunchPlan p = rs::PlanLstmb(k, op.name);
        // W_all_a's feed-forward columns are the layer GEMM in front of the walk, a LinearComponent's: no bias; its output is what the walk reads
        Require(i > 0 && nn.ops[i - 1].kind == rs::LayerOp::kGemm && nn.ops[i - 1].out_buf == k.pre_buf && nn.ops[i - 1].W.cols == p.x_cols &&
                    nn.ops[i - 1].W.rows == B && nn.ops[i - 1].bias.empty() && nn.ops[i - 1].stages.empty(), "the layer GEMM of the feed-forward columns");
        Require(p.x_cols == k.in_dim && p.m_cols == C && k.W_r.rows == B && k.W_r.cols == C, "W_all_a's recurrent columns");
        Require(k.W_b.rows == 4 * C && k.W_b.cols == B, "W_all_b");
        Require((int)k.so_scale.size() == 4 * C && (int)k.so_offset.size() == 4 * C, "the scale / offset vectors");
        for (float s : k.so_scale) Require(std::fabs(s) >= 1.0e-4f, "EnsureNonzero at load");
        Require(k.params.rows == 3 && k.params.cols == C && (long)k.params.d.size() == 3L * C, "the peephole rows");
        Require(k.delay >= 1 && k.delay <= rs::kLstmMaxDelay && k.need_lext >= 0 && k.need_lext <= nn.bufs[k.pre_buf].lext, "delay / extents");
        const int bufs[3] = {k.pre_buf, k.cm_buf, k.st_buf};
        const int dims[3] = {B, 2 * C, 2 * C};
        for (int b = 0; b < 3; b++) {
          Require(bufs[b] >= 0, "a missing buffer");
          const rs::BufferInfo &bi = nn.bufs[bufs[b]], &b0 = nn.bufs[k.pre_buf];
          Require(bi.dim == dims[b] && bi.lext == b0.lext && bi.rext == b0.rext && bi.stride == b0.stride, "the block's buffers hold the same rows");
        }
        Require(p.cell_tiles == (C + 15) / 16 && p.b_tiles == (B + 15) / 16 && p.k_m == 16 * p.cell_tiles && p.k_b == 16 * p.b_tiles &&
                    p.n_b == p.k_b && p.n_gates == 4 * p.k_m && p.ld_m == p.k_m + 4 && p.ld_b == p.k_b + 4, "tiles and k extents");
        const long lds_floats = (long)rs::kRecChains * (p.ld_m + p.ld_b);
        Require(p.lds_bytes == lds_floats * 4 && p.lds_bytes <= rs::kRecMaxLdsBytes && p.rows_per_block == rs::kRecChains, "LDS size");
        Require(rs::RecGridX(256, k.delay, 1) == (256 * k.delay + 15) / 16, "the grid");
        std::vector<float> wam_t, wb_t;
        rs::LstmbWeightImages(k, p, &wam_t, &wb_t);
        Require((long)wam_t.size() == (long)p.k_m * p.n_b && (long)wb_t.size() == (long)p.k_b * p.n_gates, "image sizes");
        for (int kk = 0; kk < p.k_m; kk++)
          for (int n = 0; n < p.n_b; n++)
            Require(wam_t[(size_t)kk * p.n_b + n] == (kk < C && n < B ? k.W_r(n, kk) : 0.0f), "W_a,m weight in the wrong place");
        for (int kk = 0; kk < p.k_b; kk++)
          for (int col = 0; col < p.n_gates; col++) {
            const int c = col / 4, g = col % 4;
            Require(wb_t[(size_t)kk * p.n_gates + col] == (kk < B && c < C ? k.W_b(g * C + c, kk) : 0.0f), "W_b weight in the wrong place");
          }
        std::printf("%s lstmb: %s\n", name.c_str(), rs::DescribeLstmb(op.name, k, p).c_str());
      }
      if (blocks == 0) std::printf("%s no recurrent block\n", name.c_str());
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}

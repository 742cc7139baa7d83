// Host-only check of the reader, the recogniser and the planners on GRU blocks in their composed form -- gru-layer / pgru-layer /
// norm-pgru-layer / opgru-layer / norm-opgru-layer (rhasspy_speech_amd/csrc/model.{h,cc}, nnet3_setup.cc, gru_plan.{h,cc},
// pgru_plan.{h,cc}): reads the final.mdl files named on the command line, compiles their networks and plans every GRU block the way
// the model load does, built by tests/test_gruc_cpu.py under the address and undefined-behaviour sanitizers.  The walks of the plans
// and weight images themselves are gru_plan_check.cc's and pgru_plan_check.cc's: the composed form shares both.
// Arguments: pairs of <case name> <path of final.mdl>.  Per block one line `<case> gru: <DescribeGru's text>` or `<case> pgru:
// <DescribePgru's text>` after the stacked layer GEMM in front of the walk, the operand dims and the weight images' sizes have been
// checked; an LSTM block of the same network prints `<case> lstm: <name>`; `<case> error: <message>` when the reader, the compiler or
// a planner refuses the model (the edited configs of the test's refusal table go through here too).
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/gru_plan.h"
#include "../../rhasspy_speech_amd/csrc/model.h"
#include "../../rhasspy_speech_amd/csrc/pgru_plan.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "gruc_plan_check: %s\n", what); std::exit(2); }
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: gruc_plan_check <name> <final.mdl> ...");
  for (int a = 1; a + 1 < argc; a += 2) {
    const std::string name = argv[a], path = argv[a + 1];
    try {
      rs::AcousticModel am;
      am.Read(path);
      const rs::Nnet &nn = am.nnet;
      int blocks = 0;
      for (size_t i = 0; i < nn.ops.size(); i++) {
        const rs::LayerOp &op = nn.ops[i];
        if (op.kind == rs::LayerOp::kLstm) { blocks++; std::printf("%s lstm: %s\n", name.c_str(), op.name.c_str()); }
        if (op.kind == rs::LayerOp::kGru) {
          blocks++;
          const rs::GruBlock &k = op.gru;
          const rs::GruLaunchPlan p = rs::PlanGru(k, op.name);
          const int C = k.cell, R = k.rec, out = k.rec + k.nonrec;
          Require(i > 0 && nn.ops[i - 1].kind == rs::LayerOp::kGemm && nn.ops[i - 1].out_buf == k.pre_buf && nn.ops[i - 1].W.cols == k.in_dim &&
                      nn.ops[i - 1].W.rows == 3 * C && (int)nn.ops[i - 1].bias.size() == 3 * C, "the stacked layer GEMM of an output-gate block");
          Require(k.W_s.rows == 2 * C && k.W_s.cols == R && (int)k.w_h.size() == C && k.W_y.rows == out && k.W_y.cols == C && (int)k.b_y.size() == out,
                  "operand dims of an output-gate block");
          Require(nn.bufs[k.hc_buf].dim == 2 * C && nn.bufs[k.y_buf].dim == out && nn.bufs[k.s_buf].dim == R, "buffers of an output-gate block");
          std::vector<float> ws_t, wy_t;
          rs::GruWeightImages(k, p, &ws_t, &wy_t);
          Require((long)ws_t.size() == (long)p.k_s * p.n_gates && (long)wy_t.size() == (long)p.k_c * p.n_out, "image sizes of an output-gate block");
          std::printf("%s gru: %s\n", name.c_str(), rs::DescribeGru(op.name, k, p).c_str());
        }
        if (op.kind == rs::LayerOp::kPgru) {
          blocks++;
          const rs::PgruBlock &k = op.pgru;
          const rs::PgruLaunchPlan p = rs::PlanPgru(k, op.name);
          const int C = k.cell, R = k.RecDim(), out = k.rec + k.nonrec, pre = 2 * C + R;
          Require(i > 0 && nn.ops[i - 1].kind == rs::LayerOp::kGemm && nn.ops[i - 1].out_buf == k.pre_buf && nn.ops[i - 1].W.cols == k.in_dim &&
                      nn.ops[i - 1].W.rows == pre && (int)nn.ops[i - 1].bias.size() == pre, "the stacked layer GEMM of a reset-gate block");
          Require(k.W_zs.rows == C && k.W_zs.cols == R && k.W_rs.rows == R && k.W_rs.cols == R && k.W_h.rows == C && k.W_h.cols == R,
                  "operand dims of a reset-gate block");
          if (k.proj()) Require(k.W_y.rows == out && k.W_y.cols == C && (int)k.b_y.size() == out && nn.bufs[k.y_buf].dim == out, "W_s.ys of a reset-gate block");
          else Require(k.W_y.rows == 0 && k.y_buf < 0 && !k.norm, "a reset-gate block without a projection");
          Require(nn.bufs[k.hc_buf].dim == 2 * C && nn.bufs[k.s_buf].dim == R, "buffers of a reset-gate block");
          std::vector<float> wr_t, wzh_t, wy_t;
          rs::PgruWeightImages(k, p, &wr_t, &wzh_t, &wy_t);
          Require((long)wr_t.size() == (long)p.k_s * p.n_r && (long)wzh_t.size() == (long)p.k_s * p.n_zh && (long)wy_t.size() == (long)p.k_c * p.n_out,
                  "image sizes of a reset-gate block");
          for (int c = 0; c < C; c++)
            for (int kk = 0; kk < R; kk++) Require(wzh_t[(size_t)kk * p.n_zh + 2 * c + 1] == k.W_h(c, kk), "W_h.UW's recurrent column in the wrong place");
          std::printf("%s pgru: %s\n", name.c_str(), rs::DescribePgru(op.name, k, p).c_str());
        }
      }
      if (blocks == 0) std::printf("%s no recurrent block\n", name.c_str());
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}

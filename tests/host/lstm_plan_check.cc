// Host-only check of the recurrent-block reader and planner (rhasspy_speech_amd/csrc/model.{h,cc}, nnet3_setup.cc,
// lstm_plan.{h,cc}): reads the final.mdl files named on the command line, compiles their networks and plans every recurrent block
// the way the model load does, built by tests/test_lstm_cpu.py under the address and undefined-behaviour sanitizers.  Arguments:
// pairs of <case name> <path of final.mdl>.  Per block one line `<case> lstm: <DescribeLstm's text>` after the plan and the two weight
// images have been walked the way the kernel walks them (every LDS address of the three tiles inside the planned bytes, every weight
// of the model in its image exactly once, the block's buffers of equal extent); `<case> error: <message>` when the reader, the
// compiler or the planner refuses the model.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/lstm_plan.h"
#include "../../rhasspy_speech_amd/csrc/model.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "lstm_plan_check: %s\n", what); std::exit(2); }
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: lstm_plan_check <name> <final.mdl> ...");
  for (int a = 1; a + 1 < argc; a += 2) {
    const std::string name = argv[a], path = argv[a + 1];
    try {
      rs::AcousticModel am;
      am.Read(path);
      const rs::Nnet &nn = am.nnet;
      int blocks = 0;
      for (size_t i = 0; i < nn.ops.size(); i++) {
        const rs::LayerOp &op = nn.ops[i];
        if (op.kind != rs::LayerOp::kLstm) continue;
        blocks++;
        const rs::LstmBlock &k = op.lstm;
        const rs::LstmLaunchPlan p = rs::PlanLstm(k, op.name);
        // the feed-forward columns are the layer GEMM in front of the walk; its output is what the walk reads
        Require(i > 0 && nn.ops[i - 1].kind == rs::LayerOp::kGemm && nn.ops[i - 1].out_buf == k.pre_buf && nn.ops[i - 1].W.cols == p.x_cols &&
                    nn.ops[i - 1].W.rows == 4 * k.cell, "the layer GEMM of W_all's feed-forward columns");
        Require(p.x_cols == k.in_dim && p.r_cols == k.RecDim() && k.W_r.rows == 4 * k.cell && k.W_r.cols == p.r_cols, "split of W_all");
        Require(k.params.rows == 3 && k.params.cols == k.cell, "<Params>");
        Require(k.delay >= 1 && k.delay <= rs::kLstmMaxDelay && k.need_lext >= 0 && k.need_lext <= nn.bufs[k.pre_buf].lext, "delay / extents");
        const int bufs[4] = {k.pre_buf, k.cm_buf, k.st_buf, k.rp_buf};
        const int dims[4] = {4 * k.cell, 2 * k.cell, k.cell + k.RecDim(), k.rec + k.nonrec};
        for (int b = 0; b < 4; b++) {
          if (bufs[b] < 0) { Require(b == 3 && !k.proj(), "a missing buffer"); continue; }
          const rs::BufferInfo &bi = nn.bufs[bufs[b]], &b0 = nn.bufs[k.pre_buf];
          Require(bi.dim == dims[b] && bi.lext == b0.lext && bi.rext == b0.rext && bi.stride == b0.stride, "the block's buffers hold the same rows");
        }
        Require(p.cell_tiles * 16 >= k.cell && (p.cell_tiles - 1) * 16 < k.cell, "cell tiles");
        Require(k.proj() ? (p.out_tiles * 16 >= k.rec + k.nonrec && (p.out_tiles - 1) * 16 < k.rec + k.nonrec) : p.out_tiles == 0, "projection tiles");
        Require(p.k_r % 16 == 0 && p.k_r >= p.r_cols && p.k_r < p.r_cols + 16 && p.k_m % 16 == 0 && p.k_m >= k.cell && p.k_m < k.cell + 16, "k padding");
        Require(p.n_gates == 4 * 16 * p.cell_tiles && p.n_out == 16 * p.out_tiles && p.ld_r > p.k_r && p.ld_m > p.k_m, "pitches");
        const long lds_floats = (long)rs::kRecChains * (2 * p.ld_r + (k.proj() ? p.ld_m : 0));
        Require(p.lds_bytes == lds_floats * 4 && p.lds_bytes <= rs::kRecMaxLdsBytes && p.rows_per_block == rs::kRecChains, "LDS size");
        // the kernel's LDS addresses: tile base + chain * pitch + k
        for (int tile = 0; tile < (k.proj() ? 3 : 2); tile++) {
          const long base = tile < 2 ? (long)tile * rs::kRecChains * p.ld_r : 2L * rs::kRecChains * p.ld_r;
          const int ld = tile < 2 ? p.ld_r : p.ld_m, kmax = tile < 2 ? p.k_r : p.k_m;
          for (int c = 0; c < rs::kRecChains; c++) Require(base + (long)c * ld + kmax - 1 < lds_floats, "LDS address outside the planned bytes");
        }
        // the tiles the waves write cover the k extents the next product reads (16 cell_tiles >= k_m, and k_r without a projection)
        Require(16 * p.cell_tiles >= p.k_m && (k.proj() || 16 * p.cell_tiles >= p.k_r), "a tile's padding columns are written");
        std::vector<float> wr_t, wrp_t;
        rs::LstmWeightImages(k, p, &wr_t, &wrp_t);
        Require((long)wr_t.size() == (long)p.k_r * p.n_gates && (long)wrp_t.size() == (long)p.k_m * p.n_out, "image sizes");
        long nz_model = 0, nz_image = 0;
        for (float w : k.W_r.d) nz_model += w != 0.0f;
        for (float w : wr_t) nz_image += w != 0.0f;
        Require(nz_model == nz_image, "W_r image: the padding is not zero");
        for (int g = 0; g < 4; g++)
          for (int c = 0; c < k.cell; c++)
            for (int kk = 0; kk < p.r_cols; kk++)
              Require(wr_t[(size_t)kk * p.n_gates + 4 * c + g] == k.W_r(g * k.cell + c, kk), "W_r weight in the wrong place");
        if (k.proj()) {
          Require(k.W_rp.rows == k.rec + k.nonrec && k.W_rp.cols == k.cell && (int)k.b_rp.size() == k.W_rp.rows, "projection dims");
          nz_model = nz_image = 0;
          for (float w : k.W_rp.d) nz_model += w != 0.0f;
          for (float w : wrp_t) nz_image += w != 0.0f;
          Require(nz_model == nz_image, "W_rp image: the padding is not zero");
          for (int n = 0; n < k.W_rp.rows; n++)
            for (int kk = 0; kk < k.cell; kk++) Require(wrp_t[(size_t)kk * p.n_out + n] == k.W_rp(n, kk), "W_rp weight in the wrong place");
        }
        // grid: every chain of a call in exactly one workgroup
        for (int utts : {1, 5, 256})
          for (int stride : {1, k.delay})
            Require(rs::RecGridX(utts, k.delay, stride) * rs::kRecChains >= utts * rs::RecChainsPerUtt(k.delay, stride) &&
                        (rs::RecGridX(utts, k.delay, stride) - 1) * rs::kRecChains < utts * rs::RecChainsPerUtt(k.delay, stride), "grid");
        std::printf("%s lstm: %s\n", name.c_str(), rs::DescribeLstm(op.name, k, p).c_str());
      }
      if (blocks == 0) std::printf("%s no recurrent block\n", name.c_str());
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}

// Host-only check of the GRU-block reader and planner (rhasspy_speech_amd/csrc/model.{h,cc}, nnet3_setup.cc, gru_plan.{h,cc}):
// reads the final.mdl files named on the command line, compiles their networks and plans every GRU block the way the model load
// does, built by tests/test_gru_cpu.py under the address and undefined-behaviour sanitizers.  Arguments: pairs of <case name> <path
// of final.mdl>.  Per block one line `<case> gru: <DescribeGru's text>` after the plan and the two weight images have been walked the
// way the kernel walks them (every LDS address of the three tiles inside the planned bytes, every weight of the model in its image
// exactly once and the padding zero, the stacked layer GEMM in front of the walk, the block's buffers of equal extent); an LSTM block
// of the same network prints `<case> lstm: <name>`; `<case> error: <message>` when the reader, the compiler or the planner refuses
// the model.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/gru_plan.h"
#include "../../rhasspy_speech_amd/csrc/model.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "gru_plan_check: %s\n", what); std::exit(2); }
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: gru_plan_check <name> <final.mdl> ...");
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
        if (op.kind != rs::LayerOp::kGru) continue;
        blocks++;
        const rs::GruBlock &k = op.gru;
        const rs::GruLaunchPlan p = rs::PlanGru(k, op.name);
        const int C = k.cell, R = k.rec, out = k.rec + k.nonrec;
        // the feed-forward columns of W_z, W_o and W_hpart are one layer GEMM in front of the walk; its output is what the walk reads
        Require(i > 0 && nn.ops[i - 1].kind == rs::LayerOp::kGemm && nn.ops[i - 1].out_buf == k.pre_buf && nn.ops[i - 1].W.cols == p.x_cols &&
                    nn.ops[i - 1].W.rows == 3 * C && (int)nn.ops[i - 1].bias.size() == 3 * C, "the stacked layer GEMM");
        Require(p.x_cols == k.in_dim && p.s_cols == R && k.W_s.rows == 2 * C && k.W_s.cols == R, "split of W_z / W_o");
        Require((int)k.w_h.size() == C && k.W_y.rows == out && k.W_y.cols == C && (int)k.b_y.size() == out && R > 0 && k.nonrec >= 0, "w_h / W_y dims");
        Require(k.delay >= 1 && k.delay <= rs::kLstmMaxDelay && k.need_lext >= 0 && k.need_lext <= nn.bufs[k.pre_buf].lext, "delay / extents");
        const int bufs[4] = {k.pre_buf, k.hc_buf, k.y_buf, k.s_buf};
        const int dims[4] = {3 * C, 2 * C, out, R};
        for (int b = 0; b < 4; b++) {
          Require(bufs[b] >= 0, "a missing buffer");
          const rs::BufferInfo &bi = nn.bufs[bufs[b]], &b0 = nn.bufs[k.pre_buf];
          Require(bi.dim == dims[b] && bi.lext == b0.lext && bi.rext == b0.rext && bi.stride == b0.stride, "the block's buffers hold the same rows");
        }
        Require(p.cell_tiles * 16 >= C && (p.cell_tiles - 1) * 16 < C && p.out_tiles * 16 >= out && (p.out_tiles - 1) * 16 < out, "tiles");
        Require(p.k_s % 16 == 0 && p.k_s >= R && p.k_s < R + 16 && p.k_c % 16 == 0 && p.k_c >= C && p.k_c < C + 16, "k padding");
        Require(p.n_gates == 2 * 16 * p.cell_tiles && p.n_out == 16 * p.out_tiles && p.ld_s > p.k_s && p.ld_c > p.k_c, "pitches");
        const long lds_floats = (long)rs::kRecChains * (2 * p.ld_s + p.ld_c);
        Require(p.lds_bytes == lds_floats * 4 && p.lds_bytes <= rs::kRecMaxLdsBytes && p.rows_per_block == rs::kRecChains, "LDS size");
        // the kernel's LDS addresses: tile base + chain * pitch + k
        for (int tile = 0; tile < 3; tile++) {
          const long base = tile < 2 ? (long)tile * rs::kRecChains * p.ld_s : 2L * rs::kRecChains * p.ld_s;
          const int ld = tile < 2 ? p.ld_s : p.ld_c, kmax = tile < 2 ? p.k_s : p.k_c;
          for (int c = 0; c < rs::kRecChains; c++) Require(base + (long)c * ld + kmax - 1 < lds_floats, "LDS address outside the planned bytes");
        }
        // the c . o tile's padding columns are written by the cell tiles; the s tiles' padding columns stay at the kernel's zeros
        Require(16 * p.cell_tiles >= p.k_c && 16 * p.out_tiles >= R, "a tile's columns are written");
        std::vector<float> ws_t, wy_t;
        rs::GruWeightImages(k, p, &ws_t, &wy_t);
        Require((long)ws_t.size() == (long)p.k_s * p.n_gates && (long)wy_t.size() == (long)p.k_c * p.n_out, "image sizes");
        // the widest addresses the kernel forms: an 8-byte load at [k_s - 1][2 (16 cell_tiles - 1)], a load at [k_c - 1][n_out - 1]
        Require((size_t)(p.k_s - 1) * p.n_gates + 2 * (16 * p.cell_tiles - 1) + 1 < ws_t.size() && (size_t)(p.k_c - 1) * p.n_out + p.n_out - 1 < wy_t.size(),
                "a weight address outside its image");
        long nz_model = 0, nz_image = 0;
        for (float w : k.W_s.d) nz_model += w != 0.0f;
        for (float w : ws_t) nz_image += w != 0.0f;
        Require(nz_model == nz_image, "W_s image: the padding is not zero");
        for (int g = 0; g < 2; g++)
          for (int c = 0; c < C; c++)
            for (int kk = 0; kk < R; kk++) Require(ws_t[(size_t)kk * p.n_gates + 2 * c + g] == k.W_s(g * C + c, kk), "W_s weight in the wrong place");
        nz_model = nz_image = 0;
        for (float w : k.W_y.d) nz_model += w != 0.0f;
        for (float w : wy_t) nz_image += w != 0.0f;
        Require(nz_model == nz_image, "W_y image: the padding is not zero");
        for (int n = 0; n < out; n++)
          for (int kk = 0; kk < C; kk++) Require(wy_t[(size_t)kk * p.n_out + n] == k.W_y(n, kk), "W_y weight in the wrong place");
        // grid: every chain of a call in exactly one workgroup
        for (int utts : {1, 5, 256})
          for (int stride : {1, k.delay})
            Require(rs::RecGridX(utts, k.delay, stride) * rs::kRecChains >= utts * rs::RecChainsPerUtt(k.delay, stride) &&
                        (rs::RecGridX(utts, k.delay, stride) - 1) * rs::kRecChains < utts * rs::RecChainsPerUtt(k.delay, stride), "grid");
        std::printf("%s gru: %s\n", name.c_str(), rs::DescribeGru(op.name, k, p).c_str());
      }
      if (blocks == 0) std::printf("%s no recurrent block\n", name.c_str());
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}

// Host-only check of the reader and planner of the blocks around a GruNonlinearityComponent (rhasspy_speech_amd/csrc/model.{h,cc},
// nnet3_setup.cc, pgru_plan.{h,cc}): reads the final.mdl files named on the command line, compiles their networks and plans every
// such block the way the model load does, built by tests/test_pgru_cpu.py under the address and undefined-behaviour sanitizers.
// Arguments: pairs of <case name> <path of final.mdl>.  Per block one line `<case> pgru: <DescribePgru's text>` after the plan and
// the three weight images have been walked the way the kernel walks them (every LDS address of the tiles inside the planned bytes,
// every weight of the model in its image exactly once and the padding zero, the stacked layer GEMM in front of the walk, the block's
// buffers of equal extent); an LSTM or OPGRU block of the same network prints `<case> lstm: <name>` / `<case> gru: <name>`;
// `<case> error: <message>` when the reader, the compiler or the planner refuses the model.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/model.h"
#include "../../rhasspy_speech_amd/csrc/pgru_plan.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "pgru_plan_check: %s\n", what); std::exit(2); }
}

static long NonZero(const std::vector<float> &v) {
  long n = 0;
  for (float w : v) n += w != 0.0f;
  return n;
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: pgru_plan_check <name> <final.mdl> ...");
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
        if (op.kind == rs::LayerOp::kGru) { blocks++; std::printf("%s gru: %s\n", name.c_str(), op.name.c_str()); }
        if (op.kind != rs::LayerOp::kPgru) continue;
        blocks++;
        const rs::PgruBlock &k = op.pgru;
        const rs::PgruLaunchPlan p = rs::PlanPgru(k, op.name);
        const bool proj = k.proj();
        const int C = k.cell, R = k.RecDim(), out = k.rec + k.nonrec, pre = 2 * C + R;
        // the feed-forward columns of W_z, W_r and W_hpart are one layer GEMM in front of the walk; its output is what the walk reads
        Require(i > 0 && nn.ops[i - 1].kind == rs::LayerOp::kGemm && nn.ops[i - 1].out_buf == k.pre_buf && nn.ops[i - 1].W.cols == p.x_cols &&
                    nn.ops[i - 1].W.rows == pre && (int)nn.ops[i - 1].bias.size() == pre, "the stacked layer GEMM");
        Require(p.x_cols == k.in_dim && p.s_cols == R && k.W_zs.rows == C && k.W_zs.cols == R && k.W_rs.rows == R && k.W_rs.cols == R &&
                    k.W_h.rows == C && k.W_h.cols == R, "split of W_z / W_r, <w_h>");
        if (proj) Require(k.W_y.rows == out && k.W_y.cols == C && (int)k.b_y.size() == out && k.rec > 0 && k.nonrec >= 0, "W_y dims");
        else Require(k.rec == 0 && k.nonrec == 0 && k.W_y.rows == 0 && k.y_buf < 0 && !k.norm, "no projection");
        Require(k.delay >= 1 && k.delay <= rs::kLstmMaxDelay && k.need_lext >= 0 && k.need_lext <= nn.bufs[k.pre_buf].lext, "delay / extents");
        const int bufs[4] = {k.pre_buf, k.hc_buf, k.s_buf, k.y_buf};
        const int dims[4] = {pre, 2 * C, R, out};
        for (int b = 0; b < (proj ? 4 : 3); b++) {
          Require(bufs[b] >= 0, "a missing buffer");
          const rs::BufferInfo &bi = nn.bufs[bufs[b]], &b0 = nn.bufs[k.pre_buf];
          Require(bi.dim == dims[b] && bi.lext == b0.lext && bi.rext == b0.rext && bi.stride == b0.stride, "the block's buffers hold the same rows");
        }
        Require(p.cell_tiles * 16 >= C && (p.cell_tiles - 1) * 16 < C && p.rec_tiles * 16 >= R && (p.rec_tiles - 1) * 16 < R, "tiles");
        Require(proj ? p.out_tiles * 16 >= out && (p.out_tiles - 1) * 16 < out : p.out_tiles == 0, "output tiles");
        Require(p.k_s == 16 * p.rec_tiles && p.k_c == 16 * p.cell_tiles && (proj || p.k_s == p.k_c), "k padding");
        Require(p.n_zh == 2 * 16 * p.cell_tiles && p.n_r == 16 * p.rec_tiles && p.n_out == 16 * p.out_tiles && p.ld_s > p.k_s && (proj ? p.ld_c > p.k_c : p.ld_c == 0),
                "pitches");
        const long lds_floats = (long)rs::kRecChains * (3 * p.ld_s + p.ld_c);
        Require(p.lds_bytes == lds_floats * 4 && p.lds_bytes <= rs::kRecMaxLdsBytes && p.rows_per_block == rs::kRecChains, "LDS size");
        // the kernel's LDS addresses: tile base + chain * pitch + k; the widest column a phase writes is 16 * tiles - 1
        for (int tile = 0; tile < (proj ? 4 : 3); tile++) {
          const long base = (long)tile * rs::kRecChains * p.ld_s;
          const int ld = tile < 3 ? p.ld_s : p.ld_c, kmax = tile < 3 ? p.k_s : p.k_c;
          for (int c = 0; c < rs::kRecChains; c++) Require(base + (long)c * ld + kmax - 1 < lds_floats, "LDS address outside the planned bytes");
        }
        Require(16 * p.rec_tiles <= p.k_s && 16 * p.cell_tiles <= p.k_c && (proj || 16 * p.cell_tiles <= p.k_s), "a phase writes outside its tile's k extent");
        std::vector<float> wr_t, wzh_t, wy_t;
        rs::PgruWeightImages(k, p, &wr_t, &wzh_t, &wy_t);
        Require((long)wr_t.size() == (long)p.k_s * p.n_r && (long)wzh_t.size() == (long)p.k_s * p.n_zh && (long)wy_t.size() == (long)p.k_c * p.n_out, "image sizes");
        // the widest addresses the kernel forms: [k_s - 1][n_r - 1], an 8-byte load at [k_s - 1][2 (16 cell_tiles - 1)], [k_c - 1][n_out - 1]
        Require((size_t)(p.k_s - 1) * p.n_r + p.n_r - 1 < wr_t.size() && (size_t)(p.k_s - 1) * p.n_zh + 2 * (16 * p.cell_tiles - 1) + 1 < wzh_t.size() &&
                    (!proj || (size_t)(p.k_c - 1) * p.n_out + p.n_out - 1 < wy_t.size()), "a weight address outside its image");
        Require(NonZero(k.W_rs.d) == NonZero(wr_t), "W_r image: the padding is not zero");
        for (int n = 0; n < R; n++)
          for (int kk = 0; kk < R; kk++) Require(wr_t[(size_t)kk * p.n_r + n] == k.W_rs(n, kk), "W_r weight in the wrong place");
        Require(NonZero(k.W_zs.d) + NonZero(k.W_h.d) == NonZero(wzh_t), "W_z / W_h image: the padding is not zero");
        for (int c = 0; c < C; c++)
          for (int kk = 0; kk < R; kk++)
            Require(wzh_t[(size_t)kk * p.n_zh + 2 * c] == k.W_zs(c, kk) && wzh_t[(size_t)kk * p.n_zh + 2 * c + 1] == k.W_h(c, kk), "W_z / W_h weight in the wrong place");
        if (proj) {
          Require(NonZero(k.W_y.d) == NonZero(wy_t), "W_y image: the padding is not zero");
          for (int n = 0; n < out; n++)
            for (int kk = 0; kk < C; kk++) Require(wy_t[(size_t)kk * p.n_out + n] == k.W_y(n, kk), "W_y weight in the wrong place");
        }
        // grid: every chain of a call in exactly one workgroup
        for (int utts : {1, 5, 256})
          for (int stride : {1, k.delay})
            Require(rs::RecGridX(utts, k.delay, stride) * rs::kRecChains >= utts * rs::RecChainsPerUtt(k.delay, stride) &&
                        (rs::RecGridX(utts, k.delay, stride) - 1) * rs::kRecChains < utts * rs::RecChainsPerUtt(k.delay, stride), "grid");
        std::printf("%s pgru: %s\n", name.c_str(), rs::DescribePgru(op.name, k, p).c_str());
      }
      if (blocks == 0) std::printf("%s no recurrent block\n", name.c_str());
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}

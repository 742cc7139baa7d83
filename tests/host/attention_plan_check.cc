// Host-only check of the attention reader and planner (rhasspy_speech_amd/csrc/model.{h,cc}, nnet3_setup.cc,
// attention_plan.{h,cc}): reads the final.mdl files named on the command line, compiles their networks and plans every attention op
// the way the model load does, built by tests/test_attention_cpu.py under the address and undefined-behaviour sanitizers.
// Arguments: pairs of <case name> <path of final.mdl>.  Per op one line `<case> <DescribeAttention's text>` after the plan has been
// walked the way the kernel walks it (the four LDS regions inside the planned bytes and apart from each other; every address a run
// can form -- a dense tile, a tile of every third row, a tile of single-frame runs -- inside its region; every head in exactly one
// head group; the op's one term and the rows it reads inside its source buffer's extent); `<case> error: <message>` when the reader,
// the compiler or the planner refuses the model.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/attention_plan.h"
#include "../../rhasspy_speech_amd/csrc/model.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "attention_plan_check: %s\n", what); std::exit(2); }
}

// The kernel's walk over one tile whose frames lie on physical rows first, first + step, ...: the runs it forms and every LDS
// address it touches, by region.
static void WalkTile(const rs::AttentionGeom &g, const rs::AttentionLaunchPlan &p, int step) {
  const int C = g.Context(), K = g.key_dim, V = g.value_dim, KV = K + V, reach = (C - 1) * g.stride, nh = std::min(p.heads_per_block, g.heads);
  const long kv_floats = (long)p.cap_rows * p.pitch, q_floats = (long)p.frames * p.heads_per_block * p.q_pitch, b_floats = (long)p.frames * p.heads_per_block * C;
  std::vector<long> prow(p.frames);
  for (int j = 0; j < p.frames; j++) prow[j] = 1000 + (long)j * step;
  int j0 = 0, runs = 0;
  while (j0 < p.frames) {
    long lo = prow[j0], hi = lo;
    int j1 = j0 + 1;
    while (j1 < p.frames) {
      const long nlo = std::min(lo, prow[j1]), nhi = std::max(hi, prow[j1]);
      if (nhi - nlo + reach + 1 > p.cap_rows) break;
      lo = nlo; hi = nhi; j1++;
    }
    const int nrun = j1 - j0;
    const long span = hi - lo + reach + 1;
    Require(nrun >= 1 && span <= p.cap_rows, "a run stages more rows than planned");
    Require((span - 1) * p.pitch + (long)(nh - 1) * KV + KV - 1 < kv_floats, "staged row outside the key / value region");
    Require((long)(nrun * nh - 1) * p.q_pitch + K + C - 1 < q_floats, "staged query outside the query region");
    for (int j = 0; j < nrun; j++)
      for (int o = 0; o < C; o++) {
        const long r = prow[j0 + j] - lo + (long)o * g.stride;
        Require(r >= 0 && r < span, "a context row outside the run's staged rows");
        Require(r * p.pitch + (long)(nh - 1) * KV + KV - 1 < kv_floats, "key / value address outside its region");
      }
    Require((long)nrun * nh * C <= b_floats, "softmax rows outside their region");
    runs++;
    j0 = j1;
  }
  if (step == 1) Require(runs == 1, "a dense tile is one run");
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: attention_plan_check <name> <final.mdl> ...");
  for (int a = 1; a + 1 < argc; a += 2) {
    const std::string name = argv[a], path = argv[a + 1];
    try {
      rs::AcousticModel am;
      am.Read(path);
      const rs::Nnet &nn = am.nnet;
      int ops = 0;
      for (const rs::LayerOp &op : nn.ops) {
        if (op.kind != rs::LayerOp::kAttention) continue;
        ops++;
        const rs::AttentionGeom &g = op.attention;
        const rs::AttentionLaunchPlan p = rs::PlanAttention(g, op.name);
        const int C = g.Context();
        Require(op.terms.size() == 1 && op.terms[0].scale == 1.0f && op.stages.empty() && op.segs.empty(), "one term, no fused stage");
        Require(op.out_dim == g.OutDim() && nn.bufs[op.out_buf].dim == g.OutDim(), "output dim");
        const rs::BufferInfo &sb = nn.bufs[op.terms[0].src_buf], &ob = nn.bufs[op.out_buf];
        Require(op.terms[0].src_col >= 0 && op.terms[0].src_col + g.InDim() <= sb.dim, "input columns outside the source buffer");
        for (int o = 0; o < C; o++) {
          const int off = op.terms[0].offset + g.TimeOffset(o);
          Require(sb.lext >= ob.lext - off && sb.rext >= ob.rext + off, "a context row outside the source buffer's extent");
        }
        Require(g.TimeOffset(0) == -g.left * g.stride && g.TimeOffset(C - 1) == g.right * g.stride, "time offsets");
        Require(p.frames >= 1 && p.frames <= rs::kAttnMaxFrames && p.heads_per_block >= 1 && p.heads_per_block <= g.heads, "tile");
        Require(p.head_groups * p.heads_per_block >= g.heads && (p.head_groups - 1) * p.heads_per_block < g.heads, "every head in exactly one head group");
        Require(p.cap_rows == p.frames + (C - 1) * g.stride && p.pitch >= p.heads_per_block * (g.key_dim + g.value_dim) && p.pitch % 2 == 1 &&
                    p.q_pitch == g.key_dim + C, "staged rows and pitches");
        const long lds_floats = (long)p.frames + (long)p.cap_rows * p.pitch + (long)p.frames * p.heads_per_block * (p.q_pitch + C);
        Require(p.lds_bytes == lds_floats * 4 && lds_floats == rs::AttentionLdsFloats(g, p.frames, p.heads_per_block) && p.lds_bytes <= rs::kAttnMaxLdsBytes, "LDS size");
        // one frame or one head more would not have fitted, or the limits hold it
        Require(p.frames == rs::kAttnMaxFrames || rs::AttentionLdsFloats(g, p.frames + 1, p.heads_per_block) * 4 > rs::kAttnMaxLdsBytes, "the tile is as long as LDS allows");
        for (int step : {1, 2, 3, g.stride, 1000}) WalkTile(g, p, step);
        for (int rows : {1, p.frames, p.frames + 1, 76800})
          Require(rs::AttentionGridX(p, rows) * p.frames >= rows && (rs::AttentionGridX(p, rows) - 1) * p.frames < rows, "grid");
        std::printf("%s %s\n", name.c_str(), rs::DescribeAttention(op.name, g, p).c_str());
      }
      if (ops == 0) std::printf("%s no attention op\n", name.c_str());
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}

// Stand-alone check of csrc/call_plan.{h,cc} (tests/test_call_plan_cpu.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers, and runs it as a child process).  Commands on stdin, one per line; one line of output each.
//   cfg window shift chunk L R Rm has_iv sl sr fsf     the PlanConfig of what follows
//   sched ns                                           one-shot flushed schedule: the last statistics frame of every chunk
//   batch ns...                                        PlanBatchSchedule: ivrow_base | row_ivec | fb | fe | orow | act
//   stream flush verbose cap d1 d2 ...                 one stream advanced at the cumulative sample counts d1 < d2 < ...; the last
//                                                      advance is final (with the flush, if flush = 1).  Per advance a group
//                                                      "ticks chunks dec_frames t0 t1 [idx last]... [/ n_riv...]", groups joined by |
//   span window first entries first entries ...        SpanOfRuns
//   lists n_slabs max_lists trim L R n T... nops (lext rext stride)...     PlanRowLists
// The program asserts for itself that every index array of an advance plan stays inside its stream's rows (CheckAdvance).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../rhasspy_speech_amd/csrc/call_plan.h"

using namespace rs;

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "call_plan_check: %s failed: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::abort(); } } while (0)

static int RoundUp(int x, int m) { return (x + m - 1) / m * m; }

// every gather / scatter row inside [row0, row0 + cap), every iVector row inside the stream's, every step range inside [0, sb - sa)
static void CheckAdvance(const PlanConfig &c, const AdvancePlan &p, const StreamView &v, int cap) {
  const StreamAdvance &a = p.pl[0];
  const int iv0 = v.row0 / c.chunk, iv1 = (v.row0 + cap) / c.chunk;
  auto rows_ok = [&](const std::vector<int> &rows, const char *what) {
    for (int r : rows) CHECK(r >= v.row0 && r < v.row0 + cap, "%s row %d outside [%d, %d) at %ld samples", what, r, v.row0, v.row0 + cap, v.n_samples);
  };
  rows_ok(p.m_out, "MFCC output"); rows_ok(p.i_src, "iVector gather"); rows_ok(p.n_src, "nnet gather"); rows_ok(p.n_lldst, "log-likelihood");
  for (int r : p.n_riv) CHECK(r >= iv0 && r < iv1, "nnet iVector row %d outside [%d, %d)", r, iv0, iv1);
  for (int r : p.n_llsrc) CHECK(r >= 0 && r < p.rowsN, "subsampled source row %d outside [0, %d)", r, p.rowsN);
  CHECK((int)p.n_src.size() == p.rowsN && (int)p.n_riv.size() == p.rowsN && (int)p.i_src.size() == p.rowsI && (int)p.m_out.size() == p.rowsM, "row counts");
  CHECK(p.steps.fb.size() == (size_t)p.max_new_chunks * std::max(p.nI, 1), "step table size");
  for (size_t k = 0; k < p.steps.fb.size(); k++) {
    if (p.nI == 0) { CHECK(p.steps.act[k] == 0, "an active step without an iVector segment"); continue; }
    if (k < a.chunks.size()) CHECK(p.steps.orow[k] >= iv0 && p.steps.orow[k] < iv1, "estimator output row %d outside [%d, %d)", p.steps.orow[k], iv0, iv1);
    else CHECK(p.steps.orow[k] == -1 && !p.steps.act[k], "a step beyond the new chunks");
    if (p.steps.act[k]) CHECK(0 <= p.steps.fb[k] && p.steps.fb[k] < p.steps.fe[k] && p.steps.fe[k] <= a.sb - a.sa, "step range [%d, %d) outside [0, %d)", p.steps.fb[k], p.steps.fe[k], a.sb - a.sa);
  }
  CHECK(a.sb <= a.avail && a.t1 <= a.avail && a.t0 <= a.t1 && a.avail + 2 <= cap, "frame ranges: sb %d t0 %d t1 %d avail %d cap %d", a.sb, a.t0, a.t1, a.avail, cap);
  CHECK(p.stage.size() >= p.o.row0 + 1 && p.stage[p.o.row0] == v.row0 && p.stage[p.o.slots] == v.slot, "staging block");
}

static void Stream(const PlanConfig &c, std::istringstream &in) {
  int flush = 0, verbose = 0, cap = 0;
  in >> flush >> verbose >> cap;
  std::vector<long> deliveries;
  for (long d; in >> d;) deliveries.push_back(d);
  CHECK(cap % c.chunk == 0 && cap >= 2 * c.chunk, "cap %d", cap);
  StreamView v;
  v.row0 = 5 * c.chunk; v.slot = 3;
  AdvancePlan plan;
  std::string out;
  for (size_t d = 0; d < deliveries.size(); d++) {
    const bool final = d + 1 == deliveries.size(), fl = final && flush;
    v.n_samples = deliveries[d];
    PlanAdvanceSchedule(c, &v, 1, fl, &plan);
    if (plan.pl[0].avail + 2 > cap) {      // (StreamGrow: twice the rows somewhere else)
      int want = cap;
      while (want < plan.pl[0].avail + 2) want *= 2;
      v.row0 = RoundUp(v.row0 + cap + 3 * c.chunk, c.chunk);
      cap = want;
    }
    PlanAdvanceRows(c, &v, 1, fl, final, &plan);
    CheckAdvance(c, plan, v, cap);
    const StreamAdvance &a = plan.pl[0];
    if (d) out += " |";
    out += " " + std::to_string(a.sched.ticks_done) + " " + std::to_string(a.sched.chunks_sched) + " " + std::to_string(c.DecFrames(a.t1)) + " " + std::to_string(a.t0) + " " + std::to_string(a.t1);
    for (auto &ch : a.chunks) out += " " + std::to_string(ch.first) + " " + std::to_string(ch.second);
    if (verbose) { out += " /"; for (int r : plan.n_riv) out += " " + std::to_string(r - v.row0 / c.chunk); }
    v.sched = a.sched; v.frames_mfcc = a.avail; v.stats_done = a.sb; v.ll_done = a.t1; v.frames_decoded = c.DecFrames(a.t1); v.dec_started = true;      // (the bookkeeping of an advance)
  }
  std::cout << "stream" << out << "\n";
}

static void Print(const std::vector<int> &v) { for (int x : v) std::cout << " " << x; }

int main() {
  PlanConfig c;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "cfg") {
      int has_iv = 0;
      in >> c.window >> c.shift >> c.chunk >> c.L >> c.R >> c.Rm >> has_iv >> c.sl >> c.sr >> c.fsf;
      CHECK(!in.fail(), "cfg");
      c.has_iv = has_iv != 0;
      std::cout << "cfg\n";
    } else if (cmd == "sched") {
      long ns = 0;
      in >> ns;
      ChunkCursor cur;
      ChunkList chunks;
      ScheduleChunks(c, ns, true, &cur, &chunks);
      std::cout << "sched";
      for (size_t k = 0; k < chunks.size(); k++) { CHECK(chunks[k].first == (int)k, "chunk index"); std::cout << " " << chunks[k].second; }
      std::cout << "\n";
    } else if (cmd == "batch") {
      std::vector<long> ns;
      for (long d; in >> d;) ns.push_back(d);
      const int n = (int)ns.size();
      std::vector<int> T(n), row_base(n + 1, 0);
      for (int u = 0; u < n; u++) { T[u] = c.Frames(ns[u]); row_base[u + 1] = row_base[u] + T[u] + c.L + c.R; }
      std::vector<int> row_ivec(row_base[n]);
      BatchSchedule bs;
      PlanBatchSchedule(c, ns.data(), T.data(), row_base.data(), n, row_ivec.data(), &bs);
      std::cout << "batch " << bs.max_chunks << " |"; Print(bs.ivrow_base); std::cout << " |"; Print(row_ivec);
      std::cout << " |"; Print(bs.steps.fb); std::cout << " |"; Print(bs.steps.fe); std::cout << " |"; Print(bs.steps.orow); std::cout << " |"; Print(bs.steps.act);
      std::cout << "\n";
    } else if (cmd == "stream") {
      Stream(c, in);
    } else if (cmd == "span") {
      int window = 0;
      in >> window;
      std::vector<std::pair<int, int>> runs;
      for (int f, e; in >> f >> e;) runs.emplace_back(f, e);
      std::cout << "span " << SpanOfRuns(runs, window) << "\n";
    } else if (cmd == "lists") {
      int n_slabs = 1, max_lists = 0, trim = 1, L = 0, R = 0, n = 0, nops = 0;
      in >> n_slabs >> max_lists >> trim >> L >> R >> n;
      std::vector<int> T(n), row_base(n + 1, 0);
      int maxT = 0;
      for (int u = 0; u < n; u++) { in >> T[u]; maxT = std::max(maxT, T[u]); row_base[u + 1] = row_base[u] + T[u] + L + R; }
      in >> nops;
      std::vector<BufExtent> ops(nops);
      for (auto &o : ops) in >> o.lext >> o.rext >> o.stride;
      CHECK(!in.fail(), "lists");
      RowListPlan lp;
      const RowListStatus st = PlanRowLists(T.data(), row_base.data(), n, maxT, L, R, ops, n_slabs, std::max(1, (maxT + n_slabs - 1) / n_slabs), max_lists, trim != 0, &lp);
      std::cout << "lists " << (int)st << " |"; Print(lp.slab_off);
      if (st == RowListStatus::kOk)
        for (auto &l : lp.lists) {
          std::cout << " | " << l.lext << " " << l.rext << " " << l.stride << " " << l.first << " " << l.n_segs << " " << l.total << " " << l.L_eff << " " << l.slab_len << " " << l.span128 << " " << l.span160 << " :";
          for (int k = 0; k <= l.n_segs; k++) std::cout << " " << lp.segs.at(l.seg_at + k);
        }
      std::cout << "\n";
    } else {
      CHECK(false, "unknown command %s", cmd.c_str());
    }
  }
  return 0;
}

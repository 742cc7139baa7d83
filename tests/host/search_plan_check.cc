// Stand-alone check of csrc/search_plan.{h,cc} (tests/test_search_plan_cpu.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers, and runs it as a child process).  Fabricates the facts of a set of graphs -- sizes only, nothing is
// dereferenced -- and walks a sweep of request kinds, batch sizes, CU counts, utterance lengths and RS_* settings.  The switches are
// set in the environment, so ReadSearchSwitches is part of what is checked.  One line per case:
//     <graph> <request> n<n_utts> T<maxT> cu<CUs> <switches without their RS_ prefix, or -> | <DescribeSearchCall>
// compared by the test with tests/host/search_plan_expected.txt.  A stream advance that searches nothing prints "no launch", an
// advance that does prints no capacities (it has none), and a call the plan refuses prints its error alone.
// A second mode, `--graph FILE CUS n_utts nbest exact [n_utts nbest exact ...]`, plans for a real graph instead (tests/
// test_search_shapes_cpu.py): FILE holds "states pdfs arcs" and then one "src dst emitting" line per arc in forward order; the program
// prints what WalkSearchGraph finds ("walk: ..."), DescribeSearchLoad for a device of CUS compute units ("search: ...", the line
// rs_model_describe reports) and, per triple, DescribeSearchCall of a whole-utterance batch call of 298 frames under the RS_*
// switches of its environment ("call n<n_utts> nbest<nbest> exact<exact> | ...").  The default run prints what it always printed.
// For every case the program also asserts that the planned LDS bytes cover the last byte of every region the shared carve-up
// (search_dev.h) defines, that they stay within a CU's 160 KB, and that tok_cap fits an int unless the plan carries the error.
//
// The expected file is a recording of the code as it was BEFORE the policy moved into search_plan.cc: that tree's decode_reg.hip,
// decode_dense.hip and decode_live.hip with every hipLaunchKernelGGL of a search or lattice kernel replaced by a snprintf of the
// template arguments, grid, threads and LDS bytes (and the CU query by a variable), called in the order and under the conditions of
// that tree's Model::Model / ToDevice / PlanSearch / AllocSearch / LaunchSearch / CollectResults and of stream.cc's advance, whose
// statements were copied around them into RecordParent(); linked with this file compiled with -DSEARCH_PLAN_RECORD.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// depth: longest epsilon path (-1: cyclic); max_e / max_x: largest emitting / epsilon out-degree
struct GraphSpec { const char *name; int S, n_e, n_x, P, eps_dst, depth, max_e, max_x; };
// stream: 0 a batch call, 1 an advance (a window launch in which no stream ends), 2 a finishing call; f_end: -1 = to the end
struct CallSpec { const char *name; int nbest; float lat_scale; int emit_lattice; float acoustic_scale; bool best_path_only, token_lists; int stream; int max_active, max_tokens_per_frame, exact_token_order; int f_end; };

#ifdef SEARCH_PLAN_RECORD
void RecordParent(const GraphSpec &gs, const CallSpec &cs, int n_utts, int maxT, int num_cu, char *line, size_t size);
#else
#include "../../rhasspy_speech_amd/csrc/search_plan.h"
using namespace rs;
#endif

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "search_plan_check: %s failed: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::abort(); } } while (0)

// ---------------------------------------------------------------------------------------------- graphs
static const GraphSpec kGraphs[] = {
    // the register shapes: <512,4,2> holds 2048 emitting / 1024 epsilon arcs, <512,8,4> twice, <256,32,16> four times as many
    // (<256,8,4> and <256,16,8> hold what the 512-thread shapes hold: the crowded rule launches them)
    {"grammar625", 625, 1800, 600, 362, 300, 1, 12, 4},
    {"reg_e2048", 700, 2048, 1024, 362, 300, 1, 12, 4},
    {"reg_e2049", 700, 2049, 1024, 362, 300, 1, 12, 4},
    {"reg_x1025", 700, 2048, 1025, 362, 300, 1, 12, 4},
    {"reg_e4096", 1500, 4096, 2048, 362, 500, 2, 40, 4},
    {"reg_e4097", 1500, 4097, 2048, 362, 500, 2, 40, 4},
    {"reg_e8192", 3000, 8192, 4096, 362, 900, 3, 40, 8},
    {"reg_e8193", 3000, 8193, 4096, 362, 900, 3, 40, 8},      // the first graph that fits no register shape: LDS-resident dense search
    {"reg_s5000", 5000, 6000, 1000, 362, 700, 1, 12, 4},      // kRegMaxStates
    {"reg_s5001", 5001, 6000, 1000, 362, 700, 1, 12, 4},
    // the exact kernel: S <= 4 NT (1024 for the 256-thread shapes: never the binding rule below exact_ok's 1000 states)
    {"exact_s1000", 1000, 1800, 600, 362, 300, 1, 32, 32},
    {"exact_s1001", 1001, 1800, 600, 362, 300, 1, 32, 32},
    {"exact_s1024", 1024, 1800, 600, 362, 300, 1, 32, 32},
    {"exact_s1025", 1025, 1800, 600, 362, 300, 1, 32, 32},
    {"exact_depth0", 625, 1800, 0, 362, 0, 0, 12, 0},
    {"exact_depth2", 625, 1800, 600, 362, 300, 2, 12, 4},
    {"exact_e33", 625, 1800, 600, 362, 300, 1, 33, 4},
    {"exact_x33", 625, 1800, 600, 362, 300, 1, 12, 33},
    {"eps_depth6", 625, 1800, 600, 362, 300, 6, 12, 4},
    {"eps_depth7", 625, 1800, 600, 362, 300, 7, 12, 4},       // deeper than 6: the closure votes
    {"eps_cyclic", 625, 1800, 600, 362, 300, -1, 12, 4},
    // the dense search's LDS budget: 12 S + 4 P + sizeof(Red<4>) + 1 KB <= 144 KB; with the reverse graph in LDS or not
    {"dense_s11408", 11408, 30000, 9000, 2000, 4000, 3, 40, 8},
    {"dense_s11409", 11409, 30000, 9000, 2000, 4000, 3, 40, 8},      // token-list search
    {"dense_graph_in", 100, 8905, 0, 100, 0, 0, 120, 0},
    {"dense_graph_out", 100, 8906, 0, 100, 0, 0, 120, 0},
    // the dense lattice: 2048 states, 8192 arcs
    {"dl_s2048", 2048, 4000, 1000, 362, 600, 1, 12, 4},
    {"dl_s2049", 2049, 4000, 1000, 362, 600, 1, 12, 4},
    {"dl_a8192", 2000, 6192, 2000, 362, 600, 1, 12, 4},
    {"dl_a8193", 2000, 6193, 2000, 362, 600, 1, 12, 4},
    // every rung of its arcs-per-thread ladder at 512 threads: 2, 4, 6, 8, 12, 16 (grammar625 is rung 6, dl_a8192 rung 16)
    {"dl_a1024", 400, 800, 224, 362, 100, 1, 12, 4},
    {"dl_a1025", 400, 801, 224, 362, 100, 1, 12, 4},
    {"dl_a2048", 600, 1600, 448, 362, 100, 1, 12, 4},
    {"dl_a3073", 900, 2500, 573, 362, 100, 1, 12, 4},
    {"dl_a4097", 1200, 3297, 800, 362, 100, 1, 12, 4},
    {"dl_a6144", 1500, 5000, 1144, 362, 100, 1, 12, 4},
    {"dl_a6145", 1500, 5001, 1144, 362, 100, 1, 12, 4},
    // graphs only the token-list searches take: an ARPA-size one for the live table, one at the 2^30 arcs its records cannot name
    {"arpa", 2000000, 5000000, 1000000, 3000, 400000, 3, 5000, 2},
    {"arcs_2p30m1", 100000, (1 << 30) - 4097, 4096, 3000, 4000, 3, 5000, 2},
    {"arcs_2p30", 100000, (1 << 30) - 4096, 4096, 3000, 4000, 3, 5000, 2},
    {"big_s100000", 100000, 300000, 50000, 3000, 20000, 3, 5000, 2},
    {"no_pdfs", 625, 1800, 600, 0, 300, 1, 12, 4},
};
static const GraphSpec &Graph(const char *name) {
  for (const GraphSpec &g : kGraphs) if (!std::strcmp(g.name, name)) return g;
  CHECK(false, "graph %s", name);
  return kGraphs[0];
}

// ---------------------------------------------------------------------------------------------- requests
static const CallSpec kCalls[] = {
    {"best", 1, 1.0f, 0, 1.0f, false, false, 0, 7000, 0, 0, -1},
    {"nbest5", 5, 1.0f, 0, 1.0f, false, false, 0, 7000, 0, 0, -1},
    {"lat_scale", 1, 0.5f, 0, 1.0f, false, false, 0, 7000, 0, 0, -1},
    {"emit_lattice", 1, 1.0f, 1, 1.0f, false, false, 0, 7000, 0, 0, -1},
    {"ac_scale", 1, 1.0f, 0, 0.1f, false, false, 0, 7000, 0, 0, -1},
    {"best_path_only", 1, 1.0f, 1, 1.0f, true, false, 0, 7000, 0, 0, -1},
    {"token_lists", 1, 1.0f, 0, 1.0f, true, true, 0, 7000, 0, 0, -1},
    {"window", 1, 1.0f, 0, 1.0f, false, false, 1, 7000, 0, 0, -1},
    {"finish", 1, 1.0f, 0, 1.0f, false, false, 2, 7000, 0, 0, -1},
    {"finish_nbest5", 5, 1.0f, 0, 1.0f, false, false, 2, 7000, 0, 0, -1},
    {"slab", 1, 1.0f, 0, 1.0f, false, false, 0, 7000, 0, 0, 100},      // a time slab that ends no utterance (maxT >= 100)
    {"exact", 1, 1.0f, 0, 1.0f, false, false, 0, 7000, 0, 1, -1},
    {"exact_nbest5", 5, 1.0f, 0, 1.0f, false, false, 0, 7000, 0, 1, -1},
    {"exact_window", 1, 1.0f, 0, 1.0f, false, false, 1, 7000, 0, 1, -1},
    {"active1000", 1, 1.0f, 0, 1.0f, false, true, 0, 1000, 0, 0, -1},
    {"per_frame500", 1, 1.0f, 0, 1.0f, false, true, 0, 7000, 500, 0, -1},
    {"nbest5_per_frame500", 5, 1.0f, 0, 1.0f, false, false, 0, 7000, 500, 0, -1},
};
static const CallSpec &Call(const char *name) {
  for (const CallSpec &c : kCalls) if (!std::strcmp(c.name, name)) return c;
  CHECK(false, "request %s", name);
  return kCalls[0];
}

// ---------------------------------------------------------------------------------------------- switches
static const char *const kSwitchNames[] = {"DECODER", "LATTICE_SEARCH", "LATTICE_KERNEL", "EXACT_ORDER", "HASH_SLOT_LIMIT", "HASH_LDS_LOG", "REG_NO_HIST"};
static void SetSwitches(const std::string &spec) {      // "DECODER=dense,EXACT_ORDER=1" or "-"
  for (const char *n : kSwitchNames) unsetenv((std::string("RS_") + n).c_str());
  if (spec == "-") return;
  size_t at = 0;
  while (at < spec.size()) {
    const size_t end = std::min(spec.find(',', at), spec.size()), eq = spec.find('=', at);
    CHECK(eq < end, "switch spec %s", spec.c_str());
    setenv(("RS_" + spec.substr(at, eq - at)).c_str(), spec.substr(eq + 1, end - eq - 1).c_str(), 1);
    at = end + 1;
  }
}

// ---------------------------------------------------------------------------------------------- one case
#ifndef SEARCH_PLAN_RECORD
static SearchGraph Facts(const GraphSpec &gs) {
  SearchGraph g;
  g.states = gs.S; g.arcs = gs.n_e + gs.n_x; g.pdfs = gs.P;
  g.in_e = gs.n_e; g.in_x = gs.n_x; g.eps_dst = gs.eps_dst;
  g.eps_depth = gs.depth; g.max_out_e = gs.max_e; g.max_out_x = gs.max_x;
  g.live_tables = (long long)gs.n_e + gs.n_x < (1ll << 30);      // (ToDevice builds them for graphs whose arcs their records can name)
  return g;
}

static void CheckLds(const SearchGraph &g, const SearchLoad &l, const SearchCall &c, const char *what) {
  const size_t kCu = 160 * 1024;
  const int S = g.states;
  if (c.search == SearchCall::kReg || c.search == SearchCall::kRegExact) {
    const RegLaunch &r = c.reg;
    CHECK(r.nt * r.ke >= g.in_e && r.nt * r.kx >= g.in_x, "%s: <%d,%d,%d> does not hold the arcs", what, r.nt, r.ke, r.kx);
    CHECK((size_t)l.key_base >= (size_t)(S + 1) * 4 && l.key_base % 16 == 0, "%s: keys at %d overlap the costs", what, l.key_base);
    CHECK(lds::RegBytes(l.key_base, S) < 65536, "%s: 16-bit LDS addresses", what);
    CHECK(r.lds_bytes >= lds::RegBytes(l.key_base, S) && r.lds_bytes >= r.stage_bytes, "%s: %zu bytes for keys and staging", what, r.lds_bytes);
    CHECK(r.exact == (c.search == SearchCall::kRegExact), "%s: exact", what);
    if (r.exact) {
      CHECK(lds::RegOrderRank(l.key_base, S) >= lds::RegBytes(l.key_base, S) && lds::RegOrderKeys(l.key_base, S) >= lds::RegOrderRank(l.key_base, S) + 2 * (size_t)S, "%s: order", what);
      CHECK(r.lds_bytes >= lds::RegOrderArcs(l.key_base, S) + 4 * (size_t)std::max(r.nt * r.ke, S), "%s: %zu bytes for the order's arrays", what, r.lds_bytes);
      CHECK(S <= 4 * r.nt, "%s: four states per thread", what);
    }
    CHECK(r.lds_bytes <= kCu, "%s: %zu bytes of LDS", what, r.lds_bytes);
  }
  if (c.search == SearchCall::kDense) {
    const DenseLaunch &d = c.dense;
    CHECK(lds::DenseCost(S) >= 8 * (size_t)S && lds::DenseLoglikes(S) >= lds::DenseCost(S) + 4 * (size_t)S && lds::DenseGraph(S, g.pdfs) >= lds::DenseLoglikes(S) + 4 * (size_t)g.pdfs, "%s: dense", what);
    size_t end = lds::DenseGraph(S, g.pdfs);
    if (d.graph_in_lds) {
      CHECK(lds::DenseGraphBeginX(S, g.pdfs) >= end + 4 * (size_t)(S + 1) && lds::DenseGraphInE(S, g.pdfs) >= lds::DenseGraphBeginX(S, g.pdfs) + 4 * (size_t)(S + 1), "%s: graph", what);
      CHECK(lds::DenseGraphInX(S, g.pdfs, g.in_e) >= lds::DenseGraphInE(S, g.pdfs) + 16 * (size_t)g.in_e, "%s: graph", what);
      CHECK(lds::DenseGraphEpsDst(S, g.pdfs, g.in_e, g.in_x) >= lds::DenseGraphInX(S, g.pdfs, g.in_e) + 16 * (size_t)g.in_x, "%s: graph", what);
      end = lds::DenseGraphEpsDst(S, g.pdfs, g.in_e, g.in_x) + 4 * (size_t)g.eps_dst;
    }
    CHECK(d.lds_bytes >= end, "%s: %zu bytes for %zu", what, d.lds_bytes, end);
    CHECK(d.lds_bytes + kDenseRedBytes <= kCu, "%s: %zu bytes of LDS", what, d.lds_bytes);
    CHECK(d.nt == 64 || d.nt == 256 || d.nt == 1024, "%s: %d threads", what, d.nt);
  }
  if (c.lattice == SearchCall::kDenseRows) {
    const DenseLatticeLaunch &d = c.dl;
    CHECK(lds::DenseLatticeExtra(S) >= 3 * 4 * (size_t)S && lds::DenseLatticeRank(S) >= lds::DenseLatticeExtra(S) + 2 * 4 * (size_t)S, "%s: lattice rows", what);
    CHECK(d.lds_bytes >= lds::DenseLatticeRank(S) + 2 * 2 * (size_t)S && d.lds_bytes <= kCu, "%s: %zu bytes of LDS", what, d.lds_bytes);
    CHECK((long)d.nt * d.ka >= g.arcs && S <= kDLMaxStates && g.arcs <= kDLMaxArcs, "%s: <%d,%d> does not hold the arcs", what, d.nt, d.ka);
    CHECK(c.search == SearchCall::kReg, "%s: dense rows without the search that leaves them", what);
  }
  CHECK(c.rows_lattice() == (c.lattice != SearchCall::kNoLattice && c.rows()), "%s: rows and lattice route", what);
  CHECK(c.error || (long long)(c.maxT + 2) * c.cap_pf == c.tok_cap, "%s: tok_cap %d", what, c.tok_cap);
  CHECK(c.live_slot_limit >= 0 && c.live_tab == kLiveTableSize, "%s: live table", what);
}
#endif

static int g_cases = 0;
static void Case(const GraphSpec &gs, const CallSpec &cs, int n_utts, int maxT, int num_cu, const char *switches) {
  SetSwitches(switches);
  char what[200], line[600];
  std::snprintf(what, sizeof(what), "%s %s n%d T%d cu%d %s", gs.name, cs.name, n_utts, maxT, num_cu, switches);
#ifdef SEARCH_PLAN_RECORD
  RecordParent(gs, cs, n_utts, maxT, num_cu, line, sizeof(line));
#else
  const SearchGraph g = Facts(gs);
  const SearchLoad l = PlanSearchLoad(g, ReadSearchSwitches());      // (the model's constructor)
  SearchRequest rq;
  rq.n_utts = n_utts; rq.maxT = maxT; rq.nbest = cs.nbest; rq.lat_scale = cs.lat_scale;
  rq.best_path_only = cs.best_path_only; rq.token_lists = cs.token_lists;
  rq.beam = 13.0f; rq.lattice_beam = 6.0f; rq.beam_delta = 0.5f; rq.acoustic_scale = cs.acoustic_scale;
  rq.max_active = cs.max_active; rq.min_active = 200; rq.max_tokens_per_frame = cs.max_tokens_per_frame;
  rq.emit_lattice = cs.emit_lattice; rq.exact_token_order = cs.exact_token_order;
  rq.stream_window = cs.stream != 0; rq.any_final = cs.stream != 1;
  rq.f_end = cs.f_end;
  const SearchCall c = PlanSearchCall(g, l, rq, num_cu, ReadSearchSwitches());
  CheckLds(g, l, c, what);
  CHECK(c.windows == (cs.stream != 0 && StreamSearchIncremental(l) && !(cs.stream == 2 && c.want_lattice)), "%s: windows", what);
  if (cs.stream == 1 && !c.windows) std::snprintf(line, sizeof(line), "no launch");
  else if (cs.stream != 1 && c.error) std::snprintf(line, sizeof(line), "error=%s", c.error);
  else {
    DescribeSearchCall(c, line, sizeof(line));
    if (cs.stream == 1) {      // an advance has no capacities
      std::string s(line);
      const size_t a = s.find(" | cap_pf="), b = s.find(" opts=");
      CHECK(a != std::string::npos && b != std::string::npos && a < b, "%s: %s", what, line);
      std::snprintf(line, sizeof(line), "%s |%s", s.substr(0, a).c_str(), s.substr(b).c_str());
    }
  }
#endif
  std::printf("%s | %s\n", what, line);
  g_cases++;
}

#ifndef SEARCH_PLAN_RECORD
// WalkSearchGraph on three small real graphs
static void CheckWalk() {
  {      // 0 -e-> 1 -x-> 2 -x-> 3, 1 -x-> 3, 3 -e-> 0, 3 -e-> 1
    const int src[] = {0, 1, 1, 2, 3, 3}, dst[] = {1, 2, 3, 3, 0, 1};
    const unsigned char em[] = {1, 0, 0, 0, 1, 1};
    SearchGraph g;
    g.states = 4;
    WalkSearchGraph(src, dst, em, 6, &g);
    CHECK(g.in_e == 3 && g.in_x == 3 && g.eps_dst == 2 && g.eps_depth == 2 && g.max_out_e == 2 && g.max_out_x == 2, "walk: %d %d %d %d %d %d", g.in_e, g.in_x, g.eps_dst,
          g.eps_depth, g.max_out_e, g.max_out_x);
  }
  {      // an epsilon cycle 1 -> 2 -> 1
    const int src[] = {0, 1, 2}, dst[] = {1, 2, 1};
    const unsigned char em[] = {1, 0, 0};
    SearchGraph g;
    g.states = 3;
    WalkSearchGraph(src, dst, em, 3, &g);
    CHECK(g.eps_depth == -1 && g.eps_dst == 2, "walk: cycle %d", g.eps_depth);
  }
  {      // no epsilon arcs
    const int src[] = {0, 0, 1}, dst[] = {1, 0, 0};
    const unsigned char em[] = {1, 1, 1};
    SearchGraph g;
    g.states = 2;
    WalkSearchGraph(src, dst, em, 3, &g);
    CHECK(g.eps_depth == 0 && g.in_x == 0 && g.eps_dst == 0 && g.max_out_e == 2, "walk: no epsilons");
  }
}
#endif

#ifndef SEARCH_PLAN_RECORD
static int GraphMode(int argc, char **argv) {
  CHECK(argc >= 7 && (argc - 4) % 3 == 0, "usage: --graph FILE CUS n_utts nbest exact [n_utts nbest exact ...]");
  FILE *f = std::fopen(argv[2], "r");
  CHECK(f, "cannot read %s", argv[2]);
  int S = 0, P = 0;
  long A = 0;
  CHECK(std::fscanf(f, "%d %d %ld", &S, &P, &A) == 3 && S > 0 && P >= 0 && A >= 0, "%s: header", argv[2]);
  std::vector<int> src(A), dst(A);
  std::vector<unsigned char> em(A);
  for (long a = 0; a < A; a++) {
    int e = 0;
    CHECK(std::fscanf(f, "%d %d %d", &src[a], &dst[a], &e) == 3, "%s: arc %ld", argv[2], a);
    CHECK(src[a] >= 0 && src[a] < S && dst[a] >= 0 && dst[a] < S && (a == 0 || src[a] >= src[a - 1]), "%s: arc %ld: %d -> %d", argv[2], a, src[a], dst[a]);
    em[a] = e != 0;
  }
  std::fclose(f);
  SearchGraph g;
  g.states = S; g.arcs = (int)A; g.pdfs = P; g.live_tables = true;
  WalkSearchGraph(src.data(), dst.data(), em.data(), (size_t)A, &g);
  const int num_cu = std::atoi(argv[3]);
  const SearchLoad l = PlanSearchLoad(g, ReadSearchSwitches());
  char line[600];
  std::printf("walk: states=%d in_e=%d in_x=%d eps_dst=%d eps_depth=%d max_out_e=%d max_out_x=%d\n", g.states, g.in_e, g.in_x, g.eps_dst, g.eps_depth, g.max_out_e, g.max_out_x);
  std::printf("search: %s\n", DescribeSearchLoad(g, l, num_cu, ReadSearchSwitches(), line, sizeof(line)));
  for (int i = 4; i + 2 < argc; i += 3) {
    SearchRequest rq;
    rq.n_utts = std::atoi(argv[i]); rq.maxT = 298; rq.nbest = std::atoi(argv[i + 1]); rq.exact_token_order = std::atoi(argv[i + 2]);
    rq.beam = 13.0f; rq.lattice_beam = 6.0f; rq.beam_delta = 0.5f; rq.max_active = 7000; rq.min_active = 200;
    const SearchCall c = PlanSearchCall(g, l, rq, num_cu, ReadSearchSwitches());
    char what[100];
    std::snprintf(what, sizeof(what), "call n%d nbest%d exact%d", rq.n_utts, rq.nbest, rq.exact_token_order);
    CheckLds(g, l, c, what);
    std::printf("%s | %s\n", what, DescribeSearchCall(c, line, sizeof(line)));
  }
  return 0;
}
#endif

int main(int argc, char **argv) {
#ifndef SEARCH_PLAN_RECORD
  if (argc > 1 && !std::strcmp(argv[1], "--graph")) return GraphMode(argc, argv);
#endif
  (void)argc; (void)argv;
  // every graph, every request kind: one utterance of 298 frames on 256 CUs
  for (const GraphSpec &g : kGraphs) {
    bool every_kind = false;
    for (const char *gn : {"grammar625", "reg_e8193", "dense_s11409", "arpa", "big_s100000", "exact_depth0"}) every_kind = every_kind || !std::strcmp(g.name, gn);
    if (every_kind) for (const CallSpec &c : kCalls) Case(g, c, 1, 298, 256, "-");
    else for (const char *cn : {"best", "nbest5", "window", "exact", "exact_nbest5", "token_lists"}) Case(g, Call(cn), 1, 298, 256, "-");
  }
  // batch sizes around the crowded threshold (4 n_utts >= 3 CUs) on two devices, for the graphs of the register shapes
  for (const char *gn : {"grammar625", "reg_e2049", "reg_e4097", "exact_s1000", "reg_e8193"})
    for (int cu : {256, 304})
      for (int n : {191, 192, 227, 228, 256, 512}) {
        if ((cu == 304) != (n == 227 || n == 228)) continue;
        for (const char *cn : {"best", "nbest5", "window", "finish", "exact"}) Case(Graph(gn), Call(cn), n, 298, cu, "-");
      }
  // utterance lengths: none, one frame, and one whose token lists cannot be indexed
  for (const char *gn : {"grammar625", "dense_s11408", "big_s100000", "arpa"})
    for (int T : {0, 1, 99, 100, 76693, 76694, 2000000})
      for (const char *cn : {"best", "nbest5", "token_lists", "slab"}) Case(Graph(gn), Call(cn), 4, T, 256, "-");
  // the switches the tests flip, alone and in the tests' combinations
  const char *const switch_sets[] = {"DECODER=reg", "DECODER=dense", "DECODER=sparse", "DECODER=hash", "DECODER=auto", "LATTICE_SEARCH=tokens", "LATTICE_KERNEL=tokens",
                                     "LATTICE_KERNEL=vote", "EXACT_ORDER=1", "EXACT_ORDER=0", "REG_NO_HIST=1", "REG_NO_HIST=0", "HASH_SLOT_LIMIT=64,HASH_LDS_LOG=6",
                                     "DECODER=hash,HASH_LDS_LOG=4"};
  for (const char *sw : switch_sets)
    for (const char *gn : {"grammar625", "exact_e33", "reg_e8193", "dl_s2049", "arpa"})
      for (const char *cn : {"best", "nbest5", "finish", "exact", "exact_nbest5"}) Case(Graph(gn), Call(cn), 4, 298, 256, sw);
#ifndef SEARCH_PLAN_RECORD
  CheckWalk();
  // the measurement switches (TuneEnv: a shipped build does not read them): coverage of the other workgroup sizes' shapes only
  SetSwitches("-");
  for (int dl_nt : {256, 1024})
    for (int dense_nt : {64, 1024})
      for (int reg_nt : {256, 512})
        for (const GraphSpec &gs : kGraphs) {
          SearchSwitches sw = ReadSearchSwitches();
          sw.dl_nt = dl_nt; sw.dense_nt = dense_nt; sw.reg_nt = reg_nt; sw.reg_nt_pinned = true; sw.stage_kb = 12;
          const SearchGraph g = Facts(gs);
          const SearchLoad l = PlanSearchLoad(g, sw);
          for (const char *cn : {"best", "nbest5", "exact"}) {
            const CallSpec &cs = Call(cn);
            SearchRequest rq;
            rq.n_utts = 512; rq.maxT = 298; rq.nbest = cs.nbest; rq.max_active = 7000; rq.exact_token_order = cs.exact_token_order;
            const SearchCall c = PlanSearchCall(g, l, rq, 256, sw);
            CheckLds(g, l, c, gs.name);
            CHECK(c.search != SearchCall::kReg || (c.reg.nt == reg_nt && c.reg.nt == l.nt), "%s: RS_REG_NT pins the shape", gs.name);
          }
        }
#endif
  return g_cases > 0 ? 0 : 1;
}

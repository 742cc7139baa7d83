// The search's policy (search_plan.h), top to bottom: the switches, what a graph's sizes allow, the launch shapes, the choice for
// one call.  Measurements behind the constants: DESIGN.md sections 4, 5 and 7, profiles/.
#include "search_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "env.h"

namespace rs {
namespace {

// ------------------------------------------------------------------------------------------ switches
const char *Env(const char *name) { return std::getenv(name); }
int IntOr(const char *e, int unset) { return e ? std::atoi(e) : unset; }
bool Is(const char *e, const char *value) { return e && std::strcmp(e, value) == 0; }

SearchSwitches ReadTuneSwitches() {
  SearchSwitches t;
  t.reg_nt = IntOr(TuneEnv("RS_REG_NT"), 0);
  t.reg_nt_pinned = TuneEnv("RS_REG_NT") != nullptr;
  t.dense_nt = IntOr(TuneEnv("RS_DENSE_NT"), 256);
  const int dl = IntOr(TuneEnv("RS_DL_NT"), 512);
  t.dl_nt = dl == 256 || dl == 1024 ? dl : 512;
  t.stage_kb = IntOr(TuneEnv("RS_DECODE_STAGE_KB"), 32);
  return t;
}

// the instantiations; RegDecodeConfig picks the first one the graph fits.  Workgroup size measured on MI355X (625-state
// grammar graph, 298 frames): 64 threads 7.5 us/frame, 256 -> 4.2, 512 -> 3.7, 1024 -> 5.1: the per-lane instruction count
// dominates until the barriers of 16 waves take over.
const int kRegConfigs[][3] = {{512, 4, 2}, {256, 8, 4}, {512, 8, 4}, {256, 16, 8}, {256, 32, 16}};

}  // namespace

SearchSwitches ReadSearchSwitches() {
  static const SearchSwitches tuned = ReadTuneSwitches();      // once per process
  SearchSwitches s = tuned;
  if (const char *e = TuneEnv("RS_FORCE_SPARSE_DECODER")) s.force_sparse = e[0] == '1';
  // reg / dense: the LDS-resident searches of small graphs; sparse: DecodeKernel alone (dense per-state tables in HBM); hash: the
  // token-list search with the live-state table, which is what "auto" runs on graphs the first two cannot hold
  const char *d = Env("RS_DECODER");
  s.decoder = Is(d, "reg") ? 1 : Is(d, "dense") ? 2 : Is(d, "sparse") ? 3 : Is(d, "hash") ? 4 : 0;
  if (s.decoder >= 3) s.force_sparse = true;
  s.lattice_search_tokens = Is(Env("RS_LATTICE_SEARCH"), "tokens");
  s.lattice_kernel_tokens = Is(Env("RS_LATTICE_KERNEL"), "tokens");
  s.lattice_kernel_vote = Is(Env("RS_LATTICE_KERNEL"), "vote");
  s.exact_order = Env("RS_EXACT_ORDER") ? (std::atoi(Env("RS_EXACT_ORDER")) != 0 ? 1 : 0) : -1;
  s.hash_slot_limit = IntOr(Env("RS_HASH_SLOT_LIMIT"), kLiveSlotCap);
  s.hash_lds_log = IntOr(Env("RS_HASH_LDS_LOG"), 0);
  s.reg_no_hist = IntOr(Env("RS_REG_NO_HIST"), 0) != 0;
  return s;
}

// ------------------------------------------------------------------------------------------ the graph
void WalkSearchGraph(const int *src, const int *dst, const unsigned char *emitting, size_t num_arcs, SearchGraph *g) {
  const int S = g->states;
  std::vector<int> out_e(S, 0), out_x(S, 0), in_x(S, 0);
  g->in_e = g->in_x = 0;
  for (size_t a = 0; a < num_arcs; a++) {
    if (emitting[a]) { out_e[src[a]]++; g->in_e++; }
    else { out_x[src[a]]++; in_x[dst[a]]++; g->in_x++; }
  }
  g->eps_dst = g->max_out_e = g->max_out_x = 0;
  for (int s = 0; s < S; s++) {
    g->eps_dst += in_x[s] > 0;
    g->max_out_e = std::max(g->max_out_e, out_e[s]);
    g->max_out_x = std::max(g->max_out_x, out_x[s]);
  }
  // longest path of the epsilon subgraph = number of closure rounds (only the register-resident kernels ask)
  g->eps_depth = 0;
  if (S > kRegMaxStates) return;
  std::vector<int> first(S + 1, 0), to(g->in_x), len(S, 0), order;
  for (int s = 0; s < S; s++) first[s + 1] = first[s] + out_x[s];
  std::vector<int> fill(first.begin(), first.end() - 1);
  for (size_t a = 0; a < num_arcs; a++) if (!emitting[a]) to[fill[src[a]]++] = dst[a];
  for (int s = 0; s < S; s++) if (in_x[s] == 0) order.push_back(s);
  for (size_t i = 0; i < order.size(); i++)
    for (int k = first[order[i]]; k < first[order[i] + 1]; k++) {
      const int d = to[k];
      len[d] = std::max(len[d], len[order[i]] + 1);
      if (--in_x[d] == 0) order.push_back(d);
    }
  if ((int)order.size() < S) { g->eps_depth = -1; return; }
  for (int s = 0; s < S; s++) g->eps_depth = std::max(g->eps_depth, len[s]);
}

// ------------------------------------------------------------------------------------------ what the sizes allow
bool RegDecodeConfig(int num_states, int num_emitting, int num_eps, const SearchSwitches &sw, int *nt, int *ke, int *kx) {
  if (num_states > kRegMaxStates) return false;
  for (const auto &c : kRegConfigs) {
    if (sw.reg_nt && c[0] != sw.reg_nt) continue;
    if ((long long)c[0] * c[1] >= num_emitting && (long long)c[0] * c[2] >= num_eps) { *nt = c[0]; *ke = c[1]; *kx = c[2]; return true; }
  }
  return false;
}

// cost_cur (f32) + key_next (u64) per state, one log-likelihood row, beside the kernel's static LDS and 1 KB to spare
bool DenseDecodeFits(int S, int P) { return lds::DenseGraph(S, P) + kDenseRedBytes + 1024 <= kDenseSmemBudget; }

SearchLoad PlanSearchLoad(const SearchGraph &g, const SearchSwitches &sw) {
  SearchLoad l;
  l.decoder = sw.decoder;
  l.force_sparse = sw.force_sparse;
  l.dense_ok = DenseDecodeFits(g.states, g.pdfs);
  if (!l.dense_ok || g.pdfs <= 0 || !RegDecodeConfig(g.states, g.in_e, g.in_x, sw, &l.nt, &l.ke, &l.kx)) return l;
  l.key_base = (int)lds::RegKeyBase(g.states);
  // cyclic or deep -> the kernel votes instead of counting rounds
  l.eps_rounds = g.eps_depth > 6 ? -1 : g.eps_depth;
  // the reference's token order can be followed exactly where its hash table cannot collide (it starts with 1000 buckets),
  // the closure is one round, and a state's arcs fit one 32-bit mask (decode_reg.hip: RegDecodeExactKernel)
  l.exact_ok = g.states <= 1000 && l.eps_rounds >= 0 && l.eps_rounds <= 1 && g.max_out_e <= 32 && g.max_out_x <= 32;
  return l;
}

static bool RegRoute(const SearchLoad &l) { return l.nt != 0 && !l.force_sparse && (l.decoder == 0 || l.decoder == 1); }
bool StreamSearchIncremental(const SearchLoad &l) { return RegRoute(l); }

// ------------------------------------------------------------------------------------------ launch shapes
RegLaunch PlanRegLaunch(const SearchGraph &g, const SearchLoad &l, int n_utts, bool window, bool any_final, int f_end, int maxT, bool exact_order,
                        int num_cu, const SearchSwitches &sw) {
  RegLaunch p;
  p.nt = l.nt; p.ke = l.ke; p.kx = l.kx;
  // A batch that puts a search workgroup on (nearly) every CU shares those CUs with the GEMM workgroups of the next call: with
  // half the waves and twice the arcs per thread the search alone is 8 % slower (1.12 -> 1.21 ms for 256 x 3 s) and the step with
  // calls in flight 2.5 % faster (2.51 -> 2.45 ms together with the smaller traceback staging below).  The tables are the same --
  // arc i sits in slot i of e_tab / x_tab whatever the shape.  RS_REG_NT pins the shape chosen at load.
  const bool crowded = !sw.reg_nt_pinned && !window && 4 * (long)n_utts >= 3 * (long)num_cu;
  if (crowded && p.nt == 512 && p.ke == 4 && p.kx == 2) { p.nt = 256; p.ke = 8; p.kx = 4; }
  else if (crowded && p.nt == 512 && p.ke == 8 && p.kx == 4) { p.nt = 256; p.ke = 16; p.kx = 8; }
  p.lds_bytes = lds::RegBytes(l.key_base, g.states);
  // room to stage back-pointer rows for the traceback.  48 KB, not more: with 128 KB a search workgroup left no room for
  // the GEMM workgroups (33 KB each) of the next decode call on its CU, and the overlap of calls in flight was limited to
  // the feature / iVector stages (3.7 ms per headline batch against 3.35 with 48 KB; the search itself takes the same
  // time).  A slab that finishes no utterance does not trace back and keeps its LDS footprint minimal.
  // (12 KB since the calls' stages are chained, engine.cc: 2.51 -> 2.47-2.49 ms per headline step; 4-16 KB are within 1 % of each other.
  // Round 4: 32 KB -- the 16-bit arc -> source table now sits in front of the rows, and the layer GEMM's 72 KB leave one of its
  // workgroups room beside a search whatever this is; 12 / 20 / 32 / 44 KB: search 1.26 / 1.23 / 1.20 / 1.20 ms, profiles/micro/stage_kb.sh)
  p.stage_bytes = (window ? !any_final : f_end <= maxT) ? 0 : (size_t)sw.stage_kb * 1024;
  p.lds_bytes = std::max(p.lds_bytes, p.stage_bytes);
  p.exact = exact_order && l.exact_ok && g.states <= 4 * p.nt;
  // the order's arrays behind the keys: list positions, insertion keys, per-position minima / sums, masks, per-arc values
  if (p.exact) p.lds_bytes = std::max(p.lds_bytes, lds::RegExactBytes(l.key_base, g.states, p.nt * p.ke));
  return p;
}

namespace {

DenseLaunch PlanDenseLaunch(const SearchGraph &g, const SearchSwitches &sw) {
  DenseLaunch p;
  p.lds_bytes = lds::DenseGraph(g.states, g.pdfs);
  // the reverse graph is cached in LDS when it fits (every frame re-reads it several times), else read through L1 / L2
  const size_t with_graph = lds::DenseGraphBytes(g.states, g.pdfs, g.in_e, g.in_x, g.eps_dst);
  p.graph_in_lds = with_graph + kDenseRedBytes + 1024 <= kDenseSmemBudget;
  if (p.graph_in_lds) p.lds_bytes = with_graph;
  // RS_DENSE_NT selects the workgroup size per utterance (64 / 256 / 1024); measured on MI355X (625-state grammar graph,
  // 298 frames): 64 -> 18 us/frame, 256 -> 10 us/frame: the frame is a chain of dependent LDS reads, more lanes hide more.
  const bool one_wave = sw.dense_nt == 64 && g.states <= 4096 && g.pdfs <= 2048;
  p.nt = one_wave ? 64 : sw.dense_nt == 1024 ? 1024 : 256;
  p.lds_bytes = std::max<size_t>(p.lds_bytes, one_wave ? 40 * 1024 : 64 * 1024);      // room to stage back-pointer rows for the traceback
  return p;
}

bool DenseLatticeFits(const SearchGraph &g) { return g.states <= kDLMaxStates && g.arcs <= kDLMaxArcs; }

DenseLatticeLaunch PlanDenseLattice(const SearchGraph &g, const SearchLoad &l, const SearchSwitches &sw) {
  DenseLatticeLaunch p;
  // 512 threads: a wave alone on its SIMD issues an instruction every ~10 cycles whatever it is, and a frame is per-arc instructions
  // (256 / 512 / 1024 threads: 1.9 / 1.3 / 1.3 ms per 256 x 298 frames, profiles/micro/dl_nt.sh; RS_DL_NT in a -DRS_TUNING build)
  p.nt = sw.dl_nt;
  // arcs per thread: the instantiations of each workgroup size (the last one holds kDLMaxArcs)
  static const int kLadder[3][6] = {{4, 8, 12, 16, 24, 32}, {2, 4, 6, 8, 12, 16}, {1, 2, 3, 4, 6, 8}};
  const int *rungs = kLadder[p.nt == 256 ? 0 : p.nt == 512 ? 1 : 2];
  const int ka = (g.arcs + p.nt - 1) / p.nt;
  p.ka = rungs[5];
  for (int i = 5; i >= 0; i--) if (ka <= rungs[i]) p.ka = rungs[i];
  p.lds_bytes = lds::DenseLatticeBytes(g.states);
  p.eps_rounds = g.in_x > 0 ? l.eps_rounds : 0;
  if (sw.lattice_kernel_vote && p.eps_rounds != 0) p.eps_rounds = -1;      // (tests: closure rounds until nothing changes)
  return p;
}

}  // namespace

// ------------------------------------------------------------------------------------------ one call
SearchCall PlanSearchCall(const SearchGraph &g, const SearchLoad &l, const SearchRequest &rq, int num_cu, const SearchSwitches &sw) {
  SearchCall c;
  const int S = g.states;
  c.S = S; c.n_utts = rq.n_utts; c.maxT = rq.maxT;
  c.opts.beam = rq.beam; c.opts.lattice_beam = rq.lattice_beam; c.opts.beam_delta = rq.beam_delta;
  c.opts.max_active = rq.max_active; c.opts.min_active = rq.min_active;
  c.opts.exact_order = ExactOrderAsked(sw, rq.exact_token_order) ? 1 : 0;
  // The reference un-scales the lattice's acoustic costs before lattice-to-nbest ranks its paths (online2-wav-nnet3-latgen-
  // faster.cc:290-293), so with a decodable --acoustic-scale other than 1 even the 1-best is chosen on the lattice.
  c.unscale = rq.acoustic_scale != 1.0f && rq.acoustic_scale != 0.0f;
  c.want_lattice = !rq.best_path_only && (rq.nbest > 1 || rq.lat_scale != 1.0f || rq.emit_lattice != 0 || c.unscale);
  c.windows = rq.stream_window && StreamSearchIncremental(l) && !(rq.any_final && c.want_lattice);
  // A lattice needs every token of every frame, which the token-list searches keep and the register-resident one does not (5.8 ms
  // against 1.1 for the headline batch): it leaves the costs of all (frame, state) pairs beside its back-pointer rows instead and
  // either DenseLatticeKernel reads those or a compaction kernel writes the token lists LatticeKernel reads (RS_LATTICE_SEARCH=tokens:
  // the token-list search, as before round 4).  Not with the exact token order, whose search keeps no cost rows.
  const bool rows_lattice = c.want_lattice && !c.windows && RegRoute(l) && !(c.opts.exact_order && l.exact_ok) && !sw.lattice_search_tokens;
  const bool lattice = c.want_lattice && !c.windows;
  const bool best_path = !lattice && !(rq.token_lists && !c.windows);      // a search that keeps no token lists will do
  const bool use_reg = rows_lattice || (best_path && RegRoute(l));
  const bool use_dense = use_reg || (best_path && l.dense_ok && !l.force_sparse && l.decoder != 3);
  if (use_reg) {
    c.reg = PlanRegLaunch(g, l, rq.n_utts, c.windows, rq.any_final, rq.f_end < 0 ? rq.maxT + 1 : rq.f_end, rq.maxT, c.opts.exact_order != 0, num_cu, sw);
    c.search = c.reg.exact ? SearchCall::kRegExact : SearchCall::kReg;
    c.opts.no_commit_hist = sw.reg_no_hist ? 1 : 0;
  } else if (use_dense) {
    c.dense = PlanDenseLaunch(g, sw);
    c.search = SearchCall::kDense;
  } else {
    const bool live = l.decoder != 3 && g.states > 0 && g.live_tables && g.arcs < (1 << 30);
    c.search = live ? SearchCall::kLive : SearchCall::kTokens;
    c.live_slot_limit = sw.hash_slot_limit;
    c.live_lds_log = sw.hash_lds_log;
  }
  if (!lattice) c.lattice = SearchCall::kNoLattice;
  else if (!rows_lattice) c.lattice = SearchCall::kTokenLists;
  else if (DenseLatticeFits(g) && !sw.lattice_kernel_tokens) { c.lattice = SearchCall::kDenseRows; c.dl = PlanDenseLattice(g, l, sw); }
  else c.lattice = SearchCall::kRowsToTokens;
  if (rq.stream_window && !rq.any_final) return c;      // (an advance keeps no tokens and collects nothing)
  // ---- capacities
  int cap_pf = rq.max_tokens_per_frame > 0 ? rq.max_tokens_per_frame : (int)std::min<long long>(std::max(4ll * rq.max_active, 8192ll), 0x7fffffffll);
  cap_pf = std::min(cap_pf, S);
  // (the register-resident search behind an n-best / lattice call keeps every live state of every frame -- it has no per-frame token
  // limit -- and DenseToTokensKernel writes them all: the utterance's slice of the token array holds S per frame whatever
  // max_tokens_per_frame says)
  if (rows_lattice) cap_pf = S;
  c.cap_pf = cap_pf;
  const long long tok_cap = (long long)(rq.maxT + 2) * cap_pf;
  if (tok_cap > 0x7fffffffLL) c.error = "decoder token capacity overflows; lower max_tokens_per_frame";
  else c.tok_cap = (int)tok_cap;
  if (c.rows()) c.path_cap = 4 * (rq.maxT + 2);
  return c;
}

const char *DescribeSearchCall(const SearchCall &c, char *buf, size_t size) {
  char search[160] = "", lattice[160] = "";
  switch (c.search) {
    case SearchCall::kReg:
    case SearchCall::kRegExact:
      std::snprintf(search, sizeof(search), "%s %s<%d,%d,%d> grid=%d threads=%d lds=%zu stage=%zu%s", c.reg.exact ? "reg-exact" : "reg",
                    c.reg.exact ? "RegDecodeExact" : "RegDecode", c.reg.nt, c.reg.ke, c.reg.kx, c.n_utts, c.reg.nt, c.reg.lds_bytes, c.reg.stage_bytes,
                    c.windows ? " windows" : "");
      break;
    case SearchCall::kDense:
      std::snprintf(search, sizeof(search), "dense DenseDecode<%d,%d> grid=%d threads=%d lds=%zu", c.dense.nt, (int)c.dense.graph_in_lds, c.n_utts, c.dense.nt,
                    c.dense.lds_bytes);
      break;
    case SearchCall::kLive:
      std::snprintf(search, sizeof(search), "live LiveDecode<1024> grid=%d threads=1024 lds=0 tab=%d slot_limit=%d lds_log=%d + Decode", c.n_utts, c.live_tab, c.live_slot_limit,
                    c.live_lds_log);
      break;
    case SearchCall::kTokens: std::snprintf(search, sizeof(search), "tokens Decode"); break;
  }
  switch (c.lattice) {
    case SearchCall::kNoLattice: std::snprintf(lattice, sizeof(lattice), "none"); break;
    case SearchCall::kDenseRows:
      std::snprintf(lattice, sizeof(lattice), "dense-rows DenseLattice<%d,%d> grid=%d threads=%d lds=%zu eps_rounds=%d", c.dl.nt, c.dl.ka, c.n_utts, c.dl.nt,
                    c.dl.lds_bytes, c.dl.eps_rounds);
      break;
    case SearchCall::kRowsToTokens: std::snprintf(lattice, sizeof(lattice), "rows-to-tokens"); break;
    case SearchCall::kTokenLists: std::snprintf(lattice, sizeof(lattice), "tokens"); break;
  }
  std::snprintf(buf, size, "%s | lattice=%s | cap_pf=%d tok_cap=%d max_words=%d path_cap=%d opts=%d,%d%s%s", search, lattice, c.cap_pf, c.tok_cap, c.max_words,
                c.path_cap, c.opts.exact_order, c.opts.no_commit_hist, c.error ? " error=" : "", c.error ? c.error : "");
  return buf;
}

const char *DescribeSearchLoad(const SearchGraph &g, const SearchLoad &l, int num_cu, const SearchSwitches &sw, char *buf, size_t size) {
  char reg[48] = "none", dl[48] = "none";
  if (l.nt != 0) std::snprintf(reg, sizeof(reg), "<%d,%d,%d>", l.nt, l.ke, l.kx);
  if (DenseLatticeFits(g)) {
    const DenseLatticeLaunch p = PlanDenseLattice(g, l, sw);
    std::snprintf(dl, sizeof(dl), "<%d,%d>", p.nt, p.ka);
  }
  std::snprintf(buf, size, "states=%d arcs_e=%d arcs_x=%d eps_depth=%d max_out=%d,%d reg=%s eps_rounds=%d exact_ok=%d dense_ok=%d dense_lattice=%s crowded_at=%ld",
                g.states, g.in_e, g.in_x, g.eps_depth, g.max_out_e, g.max_out_x, reg, l.eps_rounds, (int)l.exact_ok, (int)l.dense_ok, dl, (3 * (long)num_cu + 3) / 4);
  return buf;
}

}  // namespace rs

// Host-only policy of the search: which of the five searches a call runs, what its lattice pass reads, the template shape, grid and
// LDS bytes of every launch, the token and table capacities, and the options the kernels get.  Plain arithmetic on the graph's sizes,
// the call's sizes, the device's CU count and the RS_* switches: nothing here includes a HIP header, launches or allocates, so every
// decision can be checked on a machine without a GPU (tests/host/search_plan_check.cc, tests/test_search_plan_cpu.py).  The .hip
// files keep the kernels and one function each that maps a planned shape to the matching instantiation; engine.cc and stream.cc
// switch on SearchCall::search / SearchCall::lattice and size their arena requests from its capacities.
#pragma once
#include <cstddef>

#include "search_dev.h"

namespace rs {

// ---------------------------------------------------------------- the graph, taken once at load
struct SearchGraph {
  int states = 0, arcs = 0, pdfs = 0;
  int in_e = 0, in_x = 0;            // emitting / epsilon in-arcs in total (= arcs of each kind)
  int eps_dst = 0;                   // states with at least one epsilon in-arc
  int eps_depth = 0;                 // longest path of the epsilon subgraph; 0 = no epsilon arcs, -1 = cyclic (kRegMaxStates states at most: else 0)
  int max_out_e = 0, max_out_x = 0;  // largest emitting / epsilon out-degree
  bool live_tables = false;          // the flagged arcs and node records of the live-state table exist (HclgDev::arcs_f, nodes)
};
// in_e .. max_out_x from the arcs in forward order: arc a runs src[a] -> dst[a], emitting[a] != 0 unless it is an epsilon arc
void WalkSearchGraph(const int *src, const int *dst, const unsigned char *emitting, size_t num_arcs, SearchGraph *g);

// ---------------------------------------------------------------- switches (env.h)
struct SearchSwitches {
  // read by Model's constructor, fixed for the model from then on (PlanSearchLoad copies them into SearchLoad)
  int decoder = 0;                   // RS_DECODER=reg|dense|sparse|hash: 1..4, forces a search (tests); 0 = automatic
  bool force_sparse = false;         // RS_FORCE_SPARSE_DECODER=1 (TuneEnv): always a token-list search
  // product and test switches: std::getenv on every ReadSearchSwitches() -- tests flip them inside one process
  bool lattice_search_tokens = false;      // RS_LATTICE_SEARCH=tokens: n-best / lattice calls run a token-list search
  bool lattice_kernel_tokens = false;      // RS_LATTICE_KERNEL=tokens: the lattice pass reads token lists, never the dense rows
  bool lattice_kernel_vote = false;        // RS_LATTICE_KERNEL=vote: DenseLatticeKernel's closure runs until nothing changes
  int exact_order = -1;              // RS_EXACT_ORDER: overrides rs_decode_opts.exact_token_order; -1 = unset
  int hash_slot_limit = kLiveSlotCap;      // RS_HASH_SLOT_LIMIT: live states a frame may hold before DecodeKernel takes the utterance
  int hash_lds_log = 0;              // RS_HASH_LDS_LOG: > 1 uses only 2^n entries of the table's LDS part
  bool reg_no_hist = false;          // RS_REG_NO_HIST=1: DecodeOptsDev::no_commit_hist
  // measurement switches (TuneEnv: unset unless the build has -DRS_TUNING), read once per process
  int reg_nt = 0;                    // RS_REG_NT: only register shapes of that workgroup size; pins the shape chosen at load
  bool reg_nt_pinned = false;        //   ... set at all
  int dense_nt = 256;                // RS_DENSE_NT: 64 | 256 | 1024
  int dl_nt = 512;                   // RS_DL_NT: 256 | 512 | 1024
  int stage_kb = 32;                 // RS_DECODE_STAGE_KB: traceback staging of the register-resident search
};
SearchSwitches ReadSearchSwitches();
// rs_decode_opts.exact_token_order, RS_EXACT_ORDER overriding
inline bool ExactOrderAsked(const SearchSwitches &sw, int exact_token_order) { return sw.exact_order >= 0 ? sw.exact_order != 0 : exact_token_order != 0; }

// ---------------------------------------------------------------- what is decided at load
struct SearchLoad {
  int decoder = 0;                   // SearchSwitches::decoder / force_sparse as the constructor read them
  bool force_sparse = false;
  bool dense_ok = false;             // the per-state tables fit in LDS (DenseDecodeKernel; the reverse graph is built)
  int nt = 0, ke = 0, kx = 0;        // register shape the arc tables are laid out for; nt = 0: the graph fits none
  int key_base = 0;                  // lds::RegKeyBase, baked into the arc tables
  int eps_rounds = 0;                // closure rounds: the epsilon depth; 0 = no epsilon arcs; -1 = cyclic or deeper than 6 -> vote
  bool exact_ok = false;             // RegDecodeExactKernel can follow the reference's token order on this graph
};
// the first register shape the graph fits (sw.reg_nt: only shapes of that workgroup size)
bool RegDecodeConfig(int num_states, int num_emitting, int num_eps, const SearchSwitches &sw, int *nt, int *ke, int *kx);
bool DenseDecodeFits(int num_states, int num_pdfs);
SearchLoad PlanSearchLoad(const SearchGraph &g, const SearchSwitches &at_construction);
// the model's streams are searched as their audio arrives (register-resident windows); else the search is deferred to the finish
bool StreamSearchIncremental(const SearchLoad &l);

// ---------------------------------------------------------------- one call
struct SearchRequest {
  int n_utts = 0, maxT = 0;
  int nbest = 1;
  float lat_scale = 1.0f;
  bool best_path_only = false;       // partial results: never a lattice
  bool token_lists = false;          // the caller reads the token lists (endpoint queries of deferred streams): a token-list search
  // rs_decode_opts
  float beam = 0.f, lattice_beam = 0.f, beam_delta = 0.f, acoustic_scale = 1.0f;
  int max_active = 0, min_active = 0, max_tokens_per_frame = 0, emit_lattice = 0, exact_token_order = 0;
  // a launch on the streams of the pool; any_final: some stream ends in it
  bool stream_window = false, any_final = true;
  // the register-resident launch covers frames [f_begin, f_end) (-1 starts the utterances; f_end < 0: to the end, maxT + 1)
  int f_begin = -1, f_end = -1;
};

struct RegLaunch {                   // RegDecodeKernel<nt, ke, kx> / RegDecodeExactKernel<nt, ke, kx>
  int nt = 0, ke = 0, kx = 0;        // the shape launched (after the crowded rule); nt = 0: none
  bool exact = false;
  size_t lds_bytes = 0, stage_bytes = 0;      // dynamic LDS; the traceback staging it has to hold
};
struct DenseLaunch {                 // DenseDecodeKernel<nt, graph_in_lds>
  int nt = 0;
  bool graph_in_lds = false;
  size_t lds_bytes = 0;
};
struct DenseLatticeLaunch {          // DenseLatticeKernel<nt, ka>
  int nt = 0, ka = 0;
  size_t lds_bytes = 0;
  int eps_rounds = 0;                // SearchLoad::eps_rounds, -1 under RS_LATTICE_KERNEL=vote
};

struct SearchCall {
  enum Search {
    kReg,            // RegDecodeKernel: arcs in registers, state tables in LDS
    kRegExact,       // RegDecodeExactKernel: the same in the reference's token order
    kDense,          // DenseDecodeKernel: LDS-resident pull search
    kLive,           // LiveDecodeKernel (live-state table) with DecodeKernel behind it for the utterances that outgrow the table
    kTokens,         // DecodeKernel alone (dense per-state tables in HBM)
  } search = kTokens;
  enum Lattice {
    kNoLattice,
    kDenseRows,      // DenseLatticeKernel on the cost / back-pointer rows of a register-resident search
    kRowsToTokens,   // those rows turned into token lists (DenseWriteKernel), then LatticeKernel
    kTokenLists,     // LatticeKernel on the token lists of a token-list search
  } lattice = kNoLattice;
  bool unscale = false, want_lattice = false;
  bool windows = false;              // stream launch on the pool's windows (else, on streams: a finishing call over the retained rows)
  bool rows() const { return search == kReg || search == kRegExact || search == kDense; }      // DenseWork is in use
  bool rows_lattice() const { return lattice == kDenseRows || lattice == kRowsToTokens; }
  RegLaunch reg;
  DenseLaunch dense;
  DenseLatticeLaunch dl;
  int S = 0, n_utts = 0, maxT = 0;
  int cap_pf = 0, tok_cap = 0;       // tokens per frame the lists are sized for; token capacity per utterance (all frames)
  int max_words = 1024, path_cap = 0;
  int live_tab = kLiveTableSize, live_slot_limit = kLiveSlotCap, live_lds_log = 0;      // DecodeWork::h_tab, h_slot_limit, h_lds_log
  DecodeOptsDev opts{};
  const char *error = nullptr;       // the call cannot run (a static string): the caller fails with it
};

// Does not allocate or throw; every graph and request is valid input.
SearchCall PlanSearchCall(const SearchGraph &g, const SearchLoad &l, const SearchRequest &rq, int num_cu, const SearchSwitches &sw);
// One launch of the register-resident search: the slabs of a pipelined batch call plan theirs one by one.  window: a stream launch
RegLaunch PlanRegLaunch(const SearchGraph &g, const SearchLoad &l, int n_utts, bool window, bool any_final, int f_end, int maxT, bool exact_order,
                        int num_cu, const SearchSwitches &sw);

// "reg RegDecode<512,4,2> grid=191 threads=512 lds=32768 stage=32768 | lattice=none | cap_pf=625 tok_cap=188125 max_words=1024
// path_cap=1204 opts=0,0": the search and its kernel's template arguments in their order, grid, threads, LDS bytes; the
// lattice route (and DenseLatticeKernel's launch); the capacities (error messages, the CPU check's fixture).  Returns buf.
const char *DescribeSearchCall(const SearchCall &c, char *buf, size_t size);
// "states=625 arcs_e=1040 arcs_x=208 eps_depth=1 max_out=12,4 reg=<512,4,2> eps_rounds=1 exact_ok=1 dense_ok=1 dense_lattice=<512,4>
// crowded_at=192": what WalkSearchGraph found and PlanSearchLoad decided (reg=none: no register shape fits), the DenseLatticeKernel
// instantiation of an n-best call (none: beyond kDLMaxStates / kDLMaxArcs) and the smallest batch the crowded rule applies to on a
// device of num_cu CUs (the `search:` line of rs_model_describe).  Returns buf.
const char *DescribeSearchLoad(const SearchGraph &g, const SearchLoad &l, int num_cu, const SearchSwitches &sw, char *buf, size_t size);

}  // namespace rs

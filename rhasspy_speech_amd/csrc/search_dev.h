// What the search kernels and their host-only planner (search_plan.h) share: the options a search kernel takes, the size limits of
// the kernels, and where every kernel that receives dynamic LDS puts its arrays in it.  No HIP header: search_plan.cc and its CPU
// check include this file too, and the kernels carve their LDS with the same constexpr functions the planner sizes it with.
#pragma once
#include <cstddef>

namespace rs {

struct DecodeOptsDev {
  float beam, lattice_beam, beam_delta;
  int max_active, min_active;
  int exact_order;            // rs_decode_opts.exact_token_order: the reference's order-dependent token creation (decode_reg.hip), where the graph allows it
  int no_commit_hist = 0;     // RS_REG_NO_HIST=1 (tests): RegDecodeKernel's GetCutoff always selects the slow way (KthFromHist)
  int no_final = 0;           // partial results of streams (rs_streams_partial): the final stage ignores final costs -- the
                              // "not reached" branch every search kernel already has (GetBestPath(use_final_probs = false))
};

// ---- size limits
constexpr int kRegMaxStates = 5000;      // register-resident search: 16-bit LDS byte addresses, key_base + 8 * (S + 1) < 65536
constexpr int kDLMaxStates = 2048, kDLMaxArcs = 8192;      // DenseLatticeKernel: states and arcs named in 16 bits, rows in LDS
// live-state table (decode_live.hip): a slot is the position of a state's entry in the utterance's table (LDS part, then global part)
constexpr int kHashCandCap = 65536;      // candidate records per utterance and frame (the ARPA workload's largest frame: 24 k)
constexpr int kLiveQueueCap = 65536;     // closure work-list entries per round
constexpr int kLiveGlobalLog = 15;       // second-level table: 32768 entries (tag + key) per utterance in global memory
constexpr int kLiveGlobalSize = 1 << kLiveGlobalLog;
constexpr int kLiveSlotCap = 24576;      // live states / tokens per frame (records name a token of a frame in 16 bits)
constexpr int kLiveTableSize = 65536;    // length of the slot-indexed arrays
// sizeof(dd::Red<4>), the static LDS of DenseDecodeKernel<256, .> beside its dynamic region (decode_dense.hip asserts the equality)
constexpr size_t kDenseRedBytes = 1520;
constexpr size_t kDenseSmemBudget = 144 * 1024;

// ---- dynamic LDS carve-ups: byte offsets from the start of the region
namespace lds {
constexpr size_t Al16(size_t x) { return (x + 15) & ~(size_t)15; }

// RegDecodeKernel / RegDecodeExactKernel: cost_cur f32 [S + 1] at 0, key_next u64 [S + 1] at key_base (baked into the arc tables)
constexpr size_t RegKeyBase(int S) { return Al16((size_t)(S + 1) * 4); }
constexpr size_t RegBytes(size_t key_base, int S) { return key_base + (size_t)(S + 1) * 8; }
// RegDecodeExactKernel, behind the keys: rank16 u16 [S]; fkey, ordm, maskE u32 [S] each; arcv f32 [E] (maskX u32 [S] in the same place)
constexpr size_t RegOrderRank(size_t key_base, int S) { return Al16(RegBytes(key_base, S)); }
constexpr size_t RegOrderKeys(size_t key_base, int S) { return RegOrderRank(key_base, S) + Al16((size_t)2 * S); }
constexpr size_t RegOrderArcs(size_t key_base, int S) { return RegOrderKeys(key_base, S) + (size_t)12 * S; }
constexpr size_t RegExactBytes(size_t key_base, int S, int E) { return RegOrderArcs(key_base, S) + (size_t)4 * (E > S ? E : S); }

// DenseDecodeKernel: key_next u64 [S] at 0, cost_cur f32 [S], one log-likelihood row f32 [P]; with the reverse graph in LDS behind
// them in_begin_e, in_begin_x u32 [S + 1], in_e int4 [n_e], in_x int4 [n_x], eps_dst i32 [n_eps_dst]
constexpr size_t DenseCost(int S) { return Al16((size_t)S * 8); }
constexpr size_t DenseLoglikes(int S) { return DenseCost(S) + Al16((size_t)S * 4); }
constexpr size_t DenseGraph(int S, int P) { return DenseLoglikes(S) + Al16((size_t)P * 4); }      // = the bytes without the graph
constexpr size_t DenseGraphBeginX(int S, int P) { return DenseGraph(S, P) + Al16((size_t)(S + 1) * 4); }
constexpr size_t DenseGraphInE(int S, int P) { return DenseGraph(S, P) + 2 * Al16((size_t)(S + 1) * 4); }
constexpr size_t DenseGraphInX(int S, int P, int n_e) { return DenseGraphInE(S, P) + Al16((size_t)n_e * 16); }
constexpr size_t DenseGraphEpsDst(int S, int P, int n_e, int n_x) { return DenseGraphInX(S, P, n_e) + Al16((size_t)n_x * 16); }
constexpr size_t DenseGraphBytes(int S, int P, int n_e, int n_x, int n_eps_dst) { return DenseGraphEpsDst(S, P, n_e, n_x) + Al16((size_t)n_eps_dst * 4); }

// DenseLatticeKernel: three cost rows f32 [S] at 0, two extra-cost rows u32 [S], two token-number rows u16 [S]
constexpr size_t DenseLatticeExtra(int S) { return (size_t)S * 12; }
constexpr size_t DenseLatticeRank(int S) { return (size_t)S * 20; }
constexpr size_t DenseLatticeBytes(int S) { return (size_t)S * 24 + 16; }
}  // namespace lds

}  // namespace rs

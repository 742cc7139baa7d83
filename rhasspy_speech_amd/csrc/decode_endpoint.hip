// Endpoint queries of streams (rs_streams_endpoint): the two quantities the reference's endpointing rules are evaluated on.
// Reference: EndpointDetected(config, tmodel, frame_shift, decoder) (online2/online-endpoint.cc:109-126) =
//   decoder.FinalRelativeCost()   -> ComputeFinalCosts (decoder/lattice-faster-decoder.cc:536-569): min over the last frame's tokens
//                                    of cost + Final(state), minus the min of cost; +inf when no token is in a final state;
//   TrailingSilenceLength()       -> online-endpoint.cc:74-107: from BestPathEnd(use_final_probs = false) backwards through
//                                    TraceBackBestPath, input-epsilon arcs skipped, one frame per emitting arc whose transition-id
//                                    belongs to a silence phone, stop at the first emitting arc that does not.
// The five rules themselves are host arithmetic on these two numbers and the frame count (engine.cc: EndpointRuleFired).
//
// One workgroup per listed stream.  EndpointRegKernel reads what the incremental search (decode_reg.hip) has left in the pool, like
// PartialRegKernel: the frontier's parked costs and the back-pointer rows.
//   1. two reductions over the frontier in one pass: arg-min of cost (ties: the lowest state -- the token rs_streams_partial starts
//      from) and min of cost + final weight;
//   2. one lane walks the best token's back-pointer chain and tests each arc in the "silence" bitmap (one bit per HCLG arc: emitting,
//      and its transition-id's phone is in the silence list; built on the host, engine side).  The walk ends at the first emitting
//      arc outside the bitmap, so it reads the rows of the trailing silence plus the one it stops in -- not the stream's length.
// EndpointTokensKernel does the same on the token lists of the token-list searches (streams whose search is deferred to finish).
// Both write one 16-byte record per stream and nothing else: (silence frames, rows read, flags, relative cost).  Flags: 2 = the search
// itself has failed (the host reports it like a partial does), 8 = a broken chain; 0 with +inf = a healthy frontier without final state.
#include "decode_common.h"

#include <climits>

namespace rs {
using namespace dd;

namespace {

constexpr int kEndpointNT = 256;

__device__ __forceinline__ bool SilArc(const unsigned *bm, int arc) { return (bm[arc >> 5] >> (arc & 31)) & 1u; }

__device__ __forceinline__ float RelativeCost(float with_final, float best) {
  return (with_final < INFINITY && best < INFINITY) ? with_final - best : INFINITY;
}

template <int NT>
__global__ __launch_bounds__(NT) void EndpointRegKernel(HclgDev h, EndpointWork w) {
  constexpr int NW = NT / 64;
  __shared__ Red<NW> red;
  const int u = blockIdx.x, tid = threadIdx.x, S = h.num_states;
  const float INF = INFINITY;
  const int T = w.num_frames[u];
  if (T <= 0) {      // nothing searched yet (online-endpoint.cc:115)
    if (tid == 0) w.out[u] = make_int4(0, 0, 0, __float_as_int(INF));
    return;
  }
  const size_t slot = (size_t)w.slot[u], row0 = (size_t)w.pool_row[u];
  const float *cost = w.state_cost + slot * (2 * (size_t)S + 4);
  const int *bp = w.bp + row0 * S;
  // (the register-resident search has one error and stores 1 for it: a frame left no token, decode_reg.hip "N == 0".  Token capacity
  // and epsilon cycles are errors of the token-list searches only, so flag 2 needs no detail bits here and the host's default message,
  // "no surviving tokens", is the partial's.)
  const int error = (int)cost[S + 1];
  // ---- 1. the frontier: best token without final costs, best cost with them
  float lv = INF, lf = INF;
  int li = INT_MAX;
  if (!error)
    for (int s = tid; s < S; s += NT) {
      const float c = cost[s];
      if (!(c < INF)) continue;
      if (c < lv || (c == lv && s < li)) { lv = c; li = s; }
      lf = fminf(lf, c + h.final_cost[s]);
    }
  float best_cost, best_final;
  int best, unused;
  BlockMinArg<NT>(red, lv, li, &best_cost, &best);
  BlockMinArg<NT>(red, lf, 0, &best_final, &unused);
  if (tid != 0) return;
  // (a search that reported an error is flagged, like by a partial; a frontier that is merely empty has no silence and no final cost)
  const bool ok = !error && best_cost < INF;
  // ---- 2. trailing silence along the best chain
  int sil = 0, low = T + 1, flags = error ? 2 : 0;
  if (ok) {
    int f = T, s = best;
    const int hop_cap = 4 * (T + 2);      // (longer than any path of the search: a broken chain is reported, not followed)
    for (int hops = 0;; hops++) {
      if (hops > hop_cap || f < 0 || s < 0 || s >= S) { flags = 8; break; }
      const int arc = bp[(size_t)f * S + s];
      low = min(low, f);
      if (arc < 0) { if (f != 0) flags = 8; break; }      // (only the start state's token has none, in row 0)
      if (arc >= h.num_arcs) { flags = 8; break; }
      const int sx = h.arc_srcx[arc];
      const int eps = (int)((unsigned)sx >> 31);
      if (!eps) {
        if (!SilArc(w.sil_arc, arc)) break;               // the first non-silence frame from the end
        sil++;
      }
      s = sx & 0x7fffffff;
      f -= 1 - eps;
    }
  }
  const bool good = flags == 0;
  w.out[u] = make_int4(good ? sil : 0, low <= T ? T - low + 1 : 0, flags, __float_as_int(good ? RelativeCost(best_final, best_cost) : INF));
}

template <int NT>
__global__ __launch_bounds__(NT) void EndpointTokensKernel(HclgDev h, EndpointWork w) {
  constexpr int NW = NT / 64;
  __shared__ Red<NW> red;
  const int u = blockIdx.x, tid = threadIdx.x, S = h.num_states;
  const float INF = INFINITY;
  const int T = w.num_frames[u];
  if (T <= 0) {
    if (tid == 0) w.out[u] = make_int4(0, 0, 0, __float_as_int(INF));
    return;
  }
  const int4 *tokens = w.tokens + (size_t)u * w.tok_cap;
  const int *frame_off = w.frame_tok_off + (size_t)u * (w.max_frames + 2);
  const int search_flags = (int)(w.counters[(size_t)u * 8 + 7] & 7);      // (workgroup-uniform: the search lost every token, ran out of room or met an epsilon cycle)
  const int error = search_flags != 0;
  const int off_cur = error ? 0 : frame_off[T], n_cur = error ? 0 : frame_off[T + 1] - off_cur;
  const bool lists_ok = off_cur >= 0 && n_cur >= 0 && (long long)off_cur + n_cur <= (long long)w.tok_cap;
  float lv = INF, lf = INF;
  int li = INT_MAX;
  if (lists_ok)
    for (int i = tid; i < n_cur; i += NT) {
      const int4 tk = tokens[off_cur + i];
      const float c = __int_as_float(tk.y);
      if (!(c < INF) || tk.x < 0 || tk.x >= S) continue;
      if (c < lv || (c == lv && i < li)) { lv = c; li = i; }
      lf = fminf(lf, c + h.final_cost[tk.x]);
    }
  float best_cost, best_final;
  int best, unused;
  BlockMinArg<NT>(red, lv, li, &best_cost, &best);
  BlockMinArg<NT>(red, lf, 0, &best_final, &unused);
  if (tid != 0) return;
  const bool ok = !error && lists_ok && best_cost < INF;
  int sil = 0, low = T + 1, flags = error ? (2 | (search_flags << 4)) : (lists_ok ? 0 : 8);      // (bits 4..6: the search's own flags)
  if (ok) {
    int F = T, idx = best;
    const int hop_cap = 4 * (T + 2);
    for (int hops = 0;; hops++) {
      if (hops > hop_cap || F < 0) { flags = 8; break; }
      const int fo = frame_off[F], fn = frame_off[F + 1] - fo;
      if (fo < 0 || idx < 0 || idx >= fn || (long long)fo + idx >= (long long)w.tok_cap) { flags = 8; break; }
      const int4 tk = tokens[fo + idx];
      low = min(low, F);
      if (tk.w < 0) break;                                // the start state's token
      if (tk.w >= h.num_arcs) { flags = 8; break; }
      const int eps = (int)((unsigned)h.arc_srcx[tk.w] >> 31);
      if (!eps) {
        if (!SilArc(w.sil_arc, tk.w)) break;
        sil++;
        F -= 1;
      }
      idx = tk.z;
    }
  }
  const bool good = flags == 0;
  w.out[u] = make_int4(good ? sil : 0, low <= T ? T - low + 1 : 0, flags, __float_as_int(good ? RelativeCost(best_final, best_cost) : INF));
}

}  // namespace

void LaunchEndpointReg(const HclgDev &h, const EndpointWork &w, int n_streams, hipStream_t s) {
  if (n_streams <= 0) return;
  hipLaunchKernelGGL(EndpointRegKernel<kEndpointNT>, dim3(n_streams), dim3(kEndpointNT), 0, s, h, w);
}

void LaunchEndpointTokens(const HclgDev &h, const EndpointWork &w, int n_streams, hipStream_t s) {
  if (n_streams <= 0) return;
  hipLaunchKernelGGL(EndpointTokensKernel<kEndpointNT>, dim3(n_streams), dim3(kEndpointNT), 0, s, h, w);
}

}  // namespace rs

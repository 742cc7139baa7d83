// Partial results of register-resident streams: the best path over the decoder frames searched so far, without final
// costs (rs_streams_partial).  Reference: SingleUtteranceNnet3Decoder::GetBestPath(end_of_utterance = false)
// (online2/online-nnet3-decoding.cc:82-85) -> LatticeFasterOnlineDecoder::BestPathEnd(use_final_probs = false) /
// TraceBackBestPath (decoder/lattice-faster-online-decoder.cc:56-160).
//
// One workgroup per listed stream reads what the incremental search (decode_reg.hip) has left in the pool: the frontier's parked
// costs, the back-pointer rows, the per-frame cost offsets and the log-likelihood rows.  It writes its result record and the
// stream's path cache (kernels.h: PartialRow / PartialAnchor), nothing an advance or a finish reads.
//   1. arg-min over the frontier, no final cost (ties: the lowest state -- FinishUtterance's lv2 / i2 branch);
//   2. the best token's back-pointer chain is walked down until it arrives in a row at the state the previous call's best path left
//      that row from.  Back-pointer rows never change, so the rest of the chain IS that path: its words and cost sums come from
//      the cache.  Without such a row (no previous call, RS_PARTIAL_FULL_WALK=1, another hypothesis since the start) the walk
//      goes down to the start state;
//   3. words and costs: the cached prefix, then the walked arcs first frame first.  The costs are double sums in path order, so a
//      sum resumed from the cache is bit for bit the sum over the whole path; the terms are gathered by all lanes a block of arcs
//      at a time and added by one, which also writes the cache rows of the new path.
// Per call, the rows read are those between the frontier and the point where the best path joins the previous one -- the frames
// since the previous call while the best hypothesis holds -- not the stream's length (rs_result_counters out[0] reports them).
// (A cache point every frontier chain passes through -- the chains' meeting point -- would be shared by every later best path, but
// on grammar graphs the frontier holds tokens of other sentences whose chains meet only at the start state: measured, DESIGN.md.)
#include "decode_common.h"
#include "env.h"

#include <climits>

namespace rs {
using namespace dd;

namespace {

constexpr int kPartialNT = 256;
constexpr int kTermBlock = 512;      // path arcs whose cost terms are gathered together before they are added up

template <int NT>
__global__ __launch_bounds__(NT) void PartialRegKernel(HclgDev h, PartialWork w) {
  constexpr int NW = NT / 64;
  __shared__ Red<NW> red;
  __shared__ int sh_plen, sh_join, sh_bad, sh_low;
  __shared__ float t_g[kTermBlock], t_a[kTermBlock];
  __shared__ int t_w[kTermBlock], t_s[kTermBlock], t_f[kTermBlock];
  const int u = blockIdx.x, tid = threadIdx.x, S = h.num_states;
  const float INF = INFINITY;
  const int T = w.num_frames[u];
  int *words = w.out_words + (size_t)u * w.max_words;
  float *oc = w.out_costs + (size_t)u * 4;
  long long *ctr = w.counters + (size_t)u * 8;
  if (T <= 0) {      // nothing searched yet: no words, cost 0 (the reference asserts here; its callers guard against it)
    if (tid == 0) {
      w.out_nwords[u] = 0;
      for (int i = 0; i < 4; i++) oc[i] = 0.f;
      for (int i = 0; i < 8; i++) ctr[i] = 0;
    }
    return;
  }
  const size_t slot = (size_t)w.slot[u], row0 = (size_t)w.pool_row[u];
  const float *cost = w.state_cost + slot * (2 * (size_t)S + 4);
  const int *bp = w.bp + row0 * S;
  const float *finfo = w.frame_info + row0 * 4;
  PartialRow *prow = w.rows + row0;
  PartialAnchor *anc = w.anchor + slot;
  int *anc_words = w.anchor_words + slot * (size_t)w.max_words;
  int *path = w.path + (size_t)u * w.path_cap * 2;
  const int Tc = w.full_walk ? -1 : anc->frames1 - 1;      // the cached path covers rows [0, Tc]
  const int error = (int)cost[S + 1];
  // ---- 1. the frontier's best token
  float lv = INF;
  int li = INT_MAX;
  if (!error)
    for (int s = tid; s < S; s += NT) {
      const float c = cost[s];
      if (c < lv || (c == lv && s < li)) { lv = c; li = s; }      // (+inf never wins: lv starts there)
    }
  float best_cost;
  int best;
  BlockMinArg<NT>(red, lv, li, &best_cost, &best);
  const bool ok = !error && best_cost < INF;
  // ---- 2. the best chain, down to the cached path or the start
  if (tid == 0) {
    int f = T, s = best, pos = 0, join = -1, low = T + 1;
    bool bad = !ok;
    while (!bad) {
      if (f <= Tc && prow[f].exit_state == s) { join = f; break; }
      if (pos > w.path_cap) { bad = true; break; }      // (a walk longer than any path of the search: give up, do not loop)
      const int arc = bp[(size_t)f * S + s];
      low = min(low, f);
      if (arc < 0) { bad = f != 0; break; }             // (only the start state's token has none, in row 0)
      const int sx = h.arc_srcx[arc];
      const int eps = (int)((unsigned)sx >> 31);
      if (pos < w.path_cap) { path[2 * pos] = arc; path[2 * pos + 1] = f - 1 + eps; }
      pos++;
      s = sx & 0x7fffffff;
      f -= 1 - eps;
    }
    sh_plen = pos; sh_join = join; sh_bad = bad || pos > w.path_cap; sh_low = low;
  }
  __syncthreads();
  const bool bad = sh_bad != 0;
  const int P = bad ? 0 : sh_plen, join = sh_join;
  const bool resume = !bad && join >= 0, keep = !bad && !w.full_walk;
  // ---- 3. words and costs: the cached prefix, then the walked arcs first frame first (cache rows of the new path on the way)
  int nw = resume ? prow[join].nwords : 0;
  const int nw_join = nw;
  if (resume)
    for (int i = tid; i < nw && i < w.max_words; i += NT) words[i] = anc_words[i];
  double g = resume ? prow[join].graph : 0.0, ac = resume ? prow[join].acoustic : 0.0;
  for (int base = P - 1; base >= 0; base -= kTermBlock) {
    const int cnt = min(kTermBlock, base + 1);
    __syncthreads();                                     // (the previous block has been added up)
    for (int j = tid; j < cnt; j += NT) {
      const int i = base - j, arc = path[2 * i], Fs = path[2 * i + 1];
      const int4 a = h.arcs[arc];
      t_g[j] = __int_as_float(a.z);
      t_w[j] = a.y;
      t_s[j] = h.arc_src[arc];
      t_f[j] = a.x != 0 ? Fs : -1;                       // -1: epsilon arc (no acoustic term, the row is not left)
      float at = 0.f;
      if (a.x != 0) {
        const float off = finfo[Fs * 4 + 0];
        const float lk = w.loglikes[(row0 + Fs) * w.ld + (a.x - 1)];
        const float link_ac = off - lk;                  // ForwardLink::acoustic_cost
        at = link_ac - off;                              // TraceBackBestPath: minus the frame's cost offset
      }
      t_a[j] = at;
    }
    __syncthreads();
    if (tid == 0) {
      for (int j = 0; j < cnt; j++) {
        if (t_f[j] >= 0 && keep) prow[t_f[j]] = PartialRow{t_s[j], nw, g, ac};      // the path leaves row t_f[j] here
        g += (double)t_g[j];
        if (t_f[j] >= 0) ac += (double)t_a[j];
        if (t_w[j] != 0) { if (nw < w.max_words) words[nw] = t_w[j]; nw++; }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    const bool truncated = nw > w.max_words;
    w.out_nwords[u] = (bad || truncated) ? -1 : nw;
    oc[0] = (float)g;
    oc[1] = (float)ac;
    oc[2] = ok ? best_cost : INF;
    oc[3] = 0.f;                                         // (no final cost was reached: none was asked for)
    ctr[0] = sh_low <= T ? T - sh_low + 1 : 0;
    for (int i = 1; i < 7; i++) ctr[i] = 0;
    ctr[7] = !ok ? 2 : (bad ? 8 : 0);                    // 8: the walk did not end at the start state (cannot happen; reported)
    if (keep) {
      if (truncated) {
        anc->frames1 = 0;                                // (the rows above the join point were rewritten: the cache is gone)
      } else {
        for (int i = nw_join; i < nw; i++) anc_words[i] = words[i];
        prow[T] = PartialRow{best, nw, g, ac};
        anc->frames1 = T + 1;
      }
    }
  }
}

}  // namespace

void LaunchPartialReg(const HclgDev &h, const PartialWork &w, int n_streams, hipStream_t s) {
  if (n_streams <= 0) return;
  hipLaunchKernelGGL(PartialRegKernel<kPartialNT>, dim3(n_streams), dim3(kPartialNT), 0, s, h, w);
}

}  // namespace rs

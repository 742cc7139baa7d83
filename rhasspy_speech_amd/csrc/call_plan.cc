// Host-only planning of a decode call (call_plan.h).  No HIP here: this file builds with a plain C++17 compiler.
#include "call_plan.h"

#include <algorithm>
#include <array>
#include <cstring>

namespace rs {

void ScheduleChunks(const PlanConfig &c, long ns, bool flush, ChunkCursor *cur, ChunkList *out) {
  // ticks completed by the samples so far; the partial last read counts at EOF
  const long ticks = flush ? (ns + kTickSamples - 1) / kTickSamples : ns / kTickSamples;
  const int avail = c.Frames(ns), nch_final = (avail + c.chunk - 1) / c.chunk;
  for (long j = cur->ticks_done; j < ticks; j++) {
    const int fr = c.Frames(std::min<long>(kTickSamples * (j + 1), ns));
    const int ready = std::max(0, fr - c.Rm) / c.chunk;
    while (cur->chunks_sched < ready && (!flush || cur->chunks_sched < nch_final)) out->push_back({cur->chunks_sched++, std::min(fr - 1, fr - c.sr - 1)});
  }
  cur->ticks_done = ticks;
  if (flush) while (cur->chunks_sched < nch_final) out->push_back({cur->chunks_sched++, avail - 1});
}

void FillIvecRows(const PlanConfig &c, int t_first, int nr, int kmax, int ivrow0, int *out) {
  const int chunk = c.chunk;
  int q = t_first >= 0 ? t_first / chunk : -((-t_first + chunk - 1) / chunk), rem = t_first - q * chunk;      // t = q * chunk + rem, 0 <= rem < chunk
  auto k_of = [&](int qq) { const int d = qq * chunk - c.Rm; const int k = d >= 0 ? d / chunk : 0; return ivrow0 + (k > kmax ? kmax : k); };
  int kv = k_of(q);
  for (int r = 0; r < nr; r++) {
    out[r] = kv;
    if (++rem == chunk) { rem = 0; kv = k_of(++q); }
  }
}

void FillStepTables(const ChunkList &chunks, int stats_done, int ivrow0, int unit, int n_units, StepTables *t) {
  int done = stats_done;
  for (size_t k = 0; k < chunks.size(); k++) {
    const size_t o = k * n_units + unit;
    const int end = chunks[k].second + 1;
    t->orow[o] = ivrow0 + chunks[k].first;
    if (end > done) { t->fb[o] = done - stats_done; t->fe[o] = end - stats_done; t->act[o] = 1; done = end; }
  }
}

void PlanBatchSchedule(const PlanConfig &c, const long *n_samples, const int *T, const int *row_base, int n, int *row_ivec, BatchSchedule *out) {
  std::vector<ChunkList> chunks(n);
  out->ivrow_base.assign(n + 1, 0);
  out->max_chunks = 1;
  for (int u = 0; u < n; u++) {
    ChunkCursor fresh;
    ScheduleChunks(c, n_samples[u], /*flush=*/true, &fresh, &chunks[u]);
    const int nch = (int)chunks[u].size();
    out->max_chunks = std::max(out->max_chunks, nch);
    out->ivrow_base[u + 1] = out->ivrow_base[u] + std::max(nch, 1);
    FillIvecRows(c, -c.L, T[u] + c.L + c.R, std::max(nch - 1, 0), out->ivrow_base[u], row_ivec + row_base[u]);
  }
  out->steps.Reset(out->max_chunks, n);
  for (int u = 0; u < n; u++) FillStepTables(chunks[u], 0, out->ivrow_base[u], u, n, &out->steps);
}

int SpanOfRuns(const std::vector<std::pair<int, int>> &runs, int window) {
  long worst = 0;
  size_t b = 0;
  long inner = 0;                             // entries of the runs strictly between a and b
  for (size_t a = 0; a + 1 < runs.size(); a++) {
    if (b <= a) { b = a + 1; inner = 0; }
    while (b + 1 < runs.size() && inner + runs[b].second <= window - 2) { inner += runs[b].second; b++; }
    const long gaps = (long)runs[b].first - (runs[a].first + runs[a].second) - inner;
    worst = std::max(worst, gaps);
    if (b > a + 1) inner -= runs[a + 1].second;
  }
  return (int)(window + worst);
}

RowListStatus PlanRowLists(const int *T, const int *row_base, int n_utts, int maxT, int L, int R, const std::vector<BufExtent> &op_out, int n_slabs,
                           int slab_len, int max_lists, bool trim_halo, RowListPlan *out) {
  std::vector<RowList> &lists = out->lists;
  std::vector<int> &segs = out->segs;
  lists.clear();
  segs.clear();
  out->slab_off.assign(n_slabs + 1, 0);
  int total_frames = 0;
  for (int u = 0; u < n_utts; u++) total_frames += T[u];
  if (total_frames == 0) return RowListStatus::kOk;
  std::vector<std::pair<int, int>> runs;
  auto span = [&](int lext, int rext, int window) {
    runs.clear();
    for (int u = 0; u < n_utts; u++) if (T[u] > 0) runs.emplace_back(row_base[u] + L - lext, T[u] + lext + rext);
    return SpanOfRuns(runs, window);
  };
  RowList lp;
  lp.n_segs = n_slabs * n_utts; lp.total = total_frames; lp.L_eff = L; lp.slab_len = slab_len; lp.seg_at = segs.size();
  int acc_rows = 0;
  for (int k = 0; k < n_slabs; k++) {
    out->slab_off[k] = acc_rows;
    for (int u = 0; u < n_utts; u++) { segs.push_back(acc_rows); acc_rows += std::min(std::max(T[u] - k * slab_len, 0), slab_len); }
  }
  segs.push_back(acc_rows);
  out->slab_off[n_slabs] = acc_rows;
  // (one slab: the list runs through the utterances in order, so a GEMM tile of 128 rows reaches over its rows + the halos it skips)
  lp.span128 = n_slabs == 1 ? span(0, 0, 128) : 0;
  lp.span160 = n_slabs == 1 ? span(0, 0, 160) : 0;
  lists.push_back(lp);
  // Trimmed halos are all or nothing: an op evaluated through its list leaves the other rows of its buffer as the arena held them, so
  // everything that reads the buffer must go through a list as narrow or narrower.  Count the distinct lists first; a network with
  // more of them than a call carries evaluates every layer on all rows (of the full halo: always valid) instead.
  bool trim = trim_halo;
  {
    std::vector<std::array<int, 3>> distinct;
    for (const BufExtent &ob : op_out) {
      if (ob.stride == 1 && ((ob.lext == 0 && ob.rext == 0) || (ob.lext >= L && ob.rext >= R) || !trim_halo)) continue;
      const std::array<int, 3> key{ob.lext, ob.rext, ob.stride};
      if (std::find(distinct.begin(), distinct.end(), key) == distinct.end()) distinct.push_back(key);
    }
    if ((int)distinct.size() + 1 > max_lists) trim = false;
  }
  // (two passes: the lists of the strided buffers first -- a buffer evaluated on every f-th row MUST have its list, its consumers
  // read nothing else and its own sources may hold nothing else -- then, while there is room, the trimmed halos, which only save work)
  for (size_t pi = 0; pi < 2 * op_out.size(); pi++) {
    const bool strided_pass = pi < op_out.size();
    const BufExtent &ob = op_out[pi % op_out.size()];
    const int st = ob.stride;
    if ((st > 1) != strided_pass || (st == 1 && !trim)) continue;
    if (ob.lext > L || ob.rext > R) continue;
    if (st == 1 && ((ob.lext == 0 && ob.rext == 0) || (ob.lext >= L && ob.rext >= R))) continue;
    if (st > 1 && n_slabs != 1) return RowListStatus::kStridedInSlabs;
    bool have = false;
    for (auto &l : lists) have = have || (l.lext == ob.lext && l.rext == ob.rext && l.stride == st);
    if (have) continue;
    if ((int)lists.size() >= max_lists) {
      if (st > 1) return RowListStatus::kTooManyStrided;
      continue;
    }
    RowList l2;
    l2.lext = ob.lext; l2.rext = ob.rext; l2.n_segs = n_utts; l2.L_eff = L - ob.lext; l2.slab_len = std::max(maxT + ob.lext + ob.rext, 1); l2.seg_at = segs.size();
    l2.stride = st;
    l2.first = ob.lext % st;             // t = -lext + first is the first row with t = 0 mod stride
    int acc = 0;
    // (rows t = 0 mod stride of [-lext, T + rext): (T + rext - 1) / stride + lext / stride + 1 of them)
    for (int u = 0; u < n_utts; u++) { segs.push_back(acc); acc += T[u] > 0 ? (st == 1 ? T[u] + ob.lext + ob.rext : (T[u] + ob.rext - 1) / st + ob.lext / st + 1) : 0; }
    segs.push_back(acc);
    if (acc == 0) { segs.resize(l2.seg_at); continue; }
    l2.total = acc;
    // 128 consecutive rows of the list cross at most (126 / shortest run) + 1 utterance boundaries, each skipping the halo rows
    // nobody reads: the physical rows a GEMM tile reaches over (a strided list: not bounded here, the strip form is not used)
    l2.span128 = st == 1 ? span(ob.lext, ob.rext, 128) : 0;
    l2.span160 = st == 1 ? span(ob.lext, ob.rext, 160) : 0;
    lists.push_back(l2);
  }
  return RowListStatus::kOk;
}

// ---------------------------------------------------------------------------------------------------------- one stream advance
void PlanAdvanceSchedule(const PlanConfig &c, const StreamView *views, int n, bool flush, AdvancePlan *plan) {
  plan->n = n;
  plan->pl.resize(n);
  plan->max_new_chunks = 0;
  for (int i = 0; i < n; i++) {
    const StreamView &st = views[i];
    StreamAdvance &a = plan->pl[i];
    a.avail = c.Frames(st.n_samples);
    a.mf0 = st.frames_mfcc;
    a.chunks.clear();
    a.sched = st.sched;
    ScheduleChunks(c, st.n_samples, flush, &a.sched, &a.chunks);
    plan->max_new_chunks = std::max(plan->max_new_chunks, (int)a.chunks.size());
    a.sa = a.sb = st.stats_done;
    for (auto &ch : a.chunks) a.sb = std::max(a.sb, ch.second + 1);
    a.t0 = st.ll_done;
    a.t1 = flush ? a.avail : std::min(c.chunk * a.sched.chunks_sched, a.avail);
  }
}

namespace {
// pool rows of the frames t_first, t_first + 1, ... of a stream, clamped to its frames [0, avail) (the reference's edge clamping)
void AppendClampedRows(std::vector<int> *v, int row0, int t_first, int nr, int avail) {
  const int hi = std::max(avail - 1, 0);
  const size_t b0 = v->size();
  v->resize(b0 + nr);
  int *ps = v->data() + b0;
  for (int r = 0; r < nr; r++) { const int t = t_first + r; ps[r] = row0 + (t < 0 ? 0 : (t > hi ? hi : t)); }
}

size_t Stage(std::vector<int> *h, const std::vector<int> &v) {
  const size_t o = h->size();
  h->insert(h->end(), v.begin(), v.end());
  while (h->size() & 3) h->push_back(0);
  return o;
}
size_t Stage64(std::vector<int> *h, const std::vector<int64_t> &v) {
  const size_t o = h->size();
  h->resize(o + 2 * v.size());
  if (!v.empty()) std::memcpy(&(*h)[o], v.data(), 8 * v.size());
  while (h->size() & 3) h->push_back(0);
  return o;
}
}  // namespace

void PlanAdvanceRows(const PlanConfig &c, const StreamView *views, int n, bool flush, bool final, AdvancePlan *plan) {
  AdvancePlan &p = *plan;
  const std::vector<StreamAdvance> &pl = p.pl;
  const int chunk = c.chunk, fsf = c.fsf;
  // stages 1 and 2: the streams with new frames
  p.m_T.clear(); p.m_out.clear(); p.m_f0.clear(); p.m_rb.assign(1, 0); p.m_so.assign(1, 0);
  p.c_T.clear(); p.c_rb.clear(); p.c_tb.clear(); p.c_slot.clear(); p.c_spk_iv.clear(); p.c_spk_nn.clear();
  p.pcm_total = 0;
  p.any_spk_iv = p.any_spk_nn = false;
  for (int i = 0; i < n; i++) {
    const int tn = pl[i].avail - pl[i].mf0;
    if (tn <= 0) continue;
    const StreamView &st = views[i];
    const long cnt = st.n_samples - (long)pl[i].mf0 * c.shift;
    p.m_T.push_back(tn);
    p.m_f0.push_back(pl[i].mf0);
    p.m_rb.push_back(p.m_rb.back() + tn);
    p.m_so.push_back(p.m_so.back() + cnt);
    { const size_t b0 = p.m_out.size(); p.m_out.resize(b0 + tn); int *po = p.m_out.data() + b0; const int r0 = st.row0 + pl[i].mf0; for (int t = 0; t < tn; t++) po[t] = r0 + t; }
    p.pcm_total += (size_t)cnt;
    p.c_T.push_back(pl[i].avail); p.c_rb.push_back(st.row0); p.c_tb.push_back(pl[i].mf0); p.c_slot.push_back(st.slot);
    p.c_spk_iv.push_back(st.spk_iv ? st.slot : -1); p.c_spk_nn.push_back(st.spk_nn ? st.slot : -1);
    p.any_spk_iv = p.any_spk_iv || st.spk_iv; p.any_spk_nn = p.any_spk_nn || st.spk_nn;
  }
  p.nM = (int)p.m_T.size(); p.rowsM = p.m_rb.back();
  p.m_T.push_back(0);
  p.m_f0.push_back(0);
  p.c_rb.push_back(0);
  // stage 3: iVector segments
  p.I_idx.clear();
  for (int i = 0; i < n; i++) if (c.has_iv && !pl[i].chunks.empty()) p.I_idx.push_back(i);
  const int nI = p.nI = (int)p.I_idx.size();
  p.i_T.assign(nI + 1, 0); p.i_rb.assign(nI + 1, 0); p.i_slot.assign(nI, 0); p.i_src.clear();
  p.steps.Reset(p.max_new_chunks, std::max(nI, 1));
  for (int u = 0; u < nI; u++) {
    const StreamAdvance &a = pl[p.I_idx[u]];
    const StreamView &st = views[p.I_idx[u]];
    p.i_T[u] = a.sb - a.sa;
    p.i_rb[u + 1] = p.i_rb[u] + p.i_T[u] + c.sl + c.sr;
    p.i_slot[u] = st.slot;
    AppendClampedRows(&p.i_src, st.row0, a.sa - c.sl, p.i_T[u] + c.sl + c.sr, a.avail);
    FillStepTables(a.chunks, a.sa, st.row0 / chunk, u, nI, &p.steps);
  }
  p.rowsI = p.i_rb[nI];
  // stage 4: nnet segments
  p.N_idx.clear();
  for (int i = 0; i < n; i++) if (pl[i].t1 > pl[i].t0) p.N_idx.push_back(i);
  const int nN = p.nN = (int)p.N_idx.size();
  p.n_T.assign(nN + 1, 0); p.n_rb.assign(nN + 1, 0); p.n_fb.assign(nN + 1, 0);
  p.n_src.clear(); p.n_riv.clear(); p.n_lldst.clear(); p.n_llsrc.clear();
  p.maxTn = 0;
  for (int u = 0; u < nN; u++) {
    const StreamAdvance &a = pl[p.N_idx[u]];
    const StreamView &st = views[p.N_idx[u]];
    const int Tn = p.n_T[u] = a.t1 - a.t0, nr = Tn + c.L + c.R;
    p.maxTn = std::max(p.maxTn, Tn);
    p.n_rb[u + 1] = p.n_rb[u] + nr;
    p.n_fb[u + 1] = p.n_fb[u] + Tn;
    AppendClampedRows(&p.n_src, st.row0, a.t0 - c.L, nr, a.avail);
    p.n_riv.resize(p.n_src.size());
    FillIvecRows(c, a.t0 - c.L, nr, std::max(a.sched.chunks_sched - 1, 0), st.row0 / chunk, p.n_riv.data() + p.n_riv.size() - nr);
    if (fsf == 1) {
      const size_t l0 = p.n_lldst.size();
      p.n_lldst.resize(l0 + Tn);
      int *pd = p.n_lldst.data() + l0;
      for (int t = 0; t < Tn; t++) pd[t] = st.row0 + a.t0 + t;
    } else {
      // --frame-subsampling-factor: the decoder's frame t / fsf is the output row of t = 0, fsf, 2 fsf, ...; only those go to the pool
      for (int t = (a.t0 + fsf - 1) / fsf * fsf; t < a.t1; t += fsf) { p.n_llsrc.push_back(p.n_rb[u] + c.L + (t - a.t0)); p.n_lldst.push_back(st.row0 + t / fsf); }
    }
  }
  p.rowsN = p.n_rb[nN]; p.framesN = p.n_fb[nN];
  // stage 5: search windows
  p.maxT = p.max_feat_frames = 0;
  p.d_T.assign(n + 1, 0); p.d_rb.assign(n + 1, 0); p.w_b.resize(n); p.w_e.resize(n); p.w_f.assign(n, final ? 1 : 0);
  p.slots.resize(n); p.row0s.resize(n); p.avails.resize(n);
  for (int i = 0; i < n; i++) {
    const StreamView &st = views[i];
    p.maxT = std::max(p.maxT, c.DecFrames(pl[i].avail));
    p.max_feat_frames = std::max(p.max_feat_frames, pl[i].avail);
    p.slots[i] = st.slot; p.row0s[i] = st.row0;
    p.avails[i] = c.DecFrames(flush ? pl[i].avail : pl[i].t1);
    p.d_T[i] = c.DecFrames(pl[i].t1); p.d_rb[i] = st.row0;
    p.w_b[i] = st.dec_started ? st.frames_decoded : -1;
    p.w_e[i] = c.DecFrames(pl[i].t1);
  }
  // the staging block
  std::vector<int> &h = p.stage;
  AdvancePlan::Offsets &o = p.o;
  h.clear();
  o.mT = Stage(&h, p.m_T); o.mrb = Stage(&h, p.m_rb); o.mout = Stage(&h, p.m_out); o.mf0 = Stage(&h, p.m_f0); o.mso = Stage64(&h, p.m_so);
  o.cT = Stage(&h, p.c_T); o.crb = Stage(&h, p.c_rb); o.ctb = Stage(&h, p.c_tb); o.cslot = Stage(&h, p.c_slot);
  o.cspki = p.any_spk_iv ? Stage(&h, p.c_spk_iv) : 0; o.cspkn = p.any_spk_nn ? Stage(&h, p.c_spk_nn) : 0;
  o.iT = Stage(&h, p.i_T); o.irb = Stage(&h, p.i_rb); o.isrc = Stage(&h, p.i_src); o.islot = Stage(&h, p.i_slot);
  o.sfb = Stage(&h, p.steps.fb); o.sfe = Stage(&h, p.steps.fe); o.sor = Stage(&h, p.steps.orow); o.sac = Stage(&h, p.steps.act);
  o.nT = Stage(&h, p.n_T); o.nrb = Stage(&h, p.n_rb); o.nfb = Stage(&h, p.n_fb); o.nsrc = Stage(&h, p.n_src); o.nriv = Stage(&h, p.n_riv);
  o.nll = Stage(&h, p.n_lldst); o.nlls = Stage(&h, p.n_llsrc);
  o.dT = Stage(&h, p.d_T); o.drb = Stage(&h, p.d_rb); o.wb = Stage(&h, p.w_b); o.we = Stage(&h, p.w_e); o.wf = Stage(&h, p.w_f);
  o.slots = Stage(&h, p.slots); o.row0 = Stage(&h, p.row0s);
}

}  // namespace rs

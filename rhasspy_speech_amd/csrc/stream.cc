// Incremental streaming decode: rs_stream_accept / rs_streams_advance / rs_streams_finish.
//
// Reference: online2-cli-nnet3-decode-faster.cc:129-170 reads stdin in 1024-sample ticks and, per tick, AcceptWaveform +
// AdvanceDecoding: MFCC frames are produced as their samples arrive (online-feature.cc:131-204), a nnet chunk of 24 frames
// is computed on the first tick at which 24 (k + 1) + R feature frames exist (decodable-online-looped.cc:56-84), with the
// iVector estimated from the frames available on that tick (online-ivector-feature.cc:248-275; CG warm-started from the
// previous estimate), and the search consumes the new log-likelihood rows.  After stdin closes, the last frames are flushed
// (right context = copies of the last frame) and the lattice is finalised.
//
// Here the same work is done per rs_streams_advance call, BATCHED over the streams of the call: which chunk becomes
// computable on which tick -- and therefore which frames its iVector has seen -- is a pure function of the number of samples
// accepted so far, so it does not matter how many ticks' worth of audio one advance covers: the results are those of the
// tick-by-tick reference (and equal, bit for bit, to the batch replay of DecodeGroup(streaming = true), which the tests use as
// a cross-check).  What persists between advances lives in a per-model POOL in HBM:
//   rows (one per frame; a stream owns a contiguous range):  raw MFCCs, CMVN'd MFCCs, log-likelihoods, and -- for graphs the
//       register-resident search handles -- back-pointer rows and per-frame cutoffs;
//   slots (one per stream): iVector estimator state (linear / quadratic terms, frame count, CG solution), CMVN running sums,
//       the search's parked token costs and counters;  per-chunk iVectors.
// Everything else is transient and comes from the arena of the advance.  One advance =
//   1. new samples -> device; MFCC of the frames they complete, straight into the stream's pool rows;
//   2. CMVN resumed from the parked sums (iVector branch; nnet branch if the model has one);
//   3. for the streams that got new chunks: splice + LDA + UBM posteriors over the not-yet-accumulated frames (context gathered
//      from the pool with the reference's edge clamping), then chunk by chunk accumulate -> derived terms -> CG solve;
//   4. the acoustic model over [first new frame - left context, last new frame + right context) of every such stream, gathered
//      into the batch layout of kernels.h, output rows scattered into the pool;
//   5. the search resumed over the new rows (RegDecodeKernel windows); graphs it cannot hold are searched at finish.
// rs_streams_finish = one last advance with end-of-input semantics, then traceback / lattice / result records: its device
// work is one chunk's worth when the streams were advanced as the audio came in.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <thread>
#include "env.h"

#include "engine.h"
#include <cstdio>

namespace rs {

// A second host thread for the second half of an advance.  Issuing an advance's ~35 launches is the host's largest share of a
// streams step (profiles/micro/streams_trace.sh: 7 ms of 21.5 per 64 x 30 s, beside 2.6 ms accepting samples, 1.5 planning, 1.3
// uploading, 2.7 finishing); the acoustic model's and the search's launches (stage B / C: queues q and qc) need nothing the caller's
// thread computes afterwards, so they are handed to this thread as a closure and the caller goes on to its bookkeeping and the next
// advance's plan and stage A (queues qa, qi).  Jobs run in submission order (the order on q / qc is the advances' order); whoever
// is about to wait for an advance's events, to queue work on q / qc itself, or to tear the pool down drains the thread first; an
// exception of a job surfaces at that drain.
struct StreamIssuer {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv, cv_done;
  std::deque<std::function<void()>> jobs;
  long submitted = 0, completed = 0;
  bool stop = false, started = false;
  std::exception_ptr err;
  int device = 0;
  void Loop() {
    (void)hipSetDevice(device);
    for (;;) {
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !jobs.empty(); });
        if (jobs.empty()) return;
        job = std::move(jobs.front());
        jobs.pop_front();
      }
      std::exception_ptr e;
      try { job(); } catch (...) { e = std::current_exception(); }
      {
        std::lock_guard<std::mutex> lk(mu);
        if (e && !err) err = e;
        completed++;
      }
      cv_done.notify_all();
    }
  }
  void Submit(std::function<void()> f) {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!started) { started = true; th = std::thread([this] { Loop(); }); }
      jobs.push_back(std::move(f));
      submitted++;
    }
    cv.notify_one();
  }
  // everything submitted has been issued; a job's exception is rethrown here (once)
  void Drain(bool rethrow = true) {
    std::exception_ptr e;
    {
      std::unique_lock<std::mutex> lk(mu);
      cv_done.wait(lk, [&] { return completed == submitted; });
      e = err;
      err = nullptr;
    }
    if (e && rethrow) std::rethrow_exception(e);
  }
  ~StreamIssuer() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
};

struct StreamPool {
  StreamIssuer issuer;
  bool use_issuer = true;        // RS_STREAM_ISSUER=0: the caller's thread issues everything (A/B: profiles/micro)
  int min_ticks = 16;            // an advance call with fewer new 1024-sample ticks than this on every stream is coalesced into the next (rs_decode_opts.stream_min_ticks; RS_STREAM_MIN_TICKS overrides)
  // Queues, so that consecutive advances overlap on the device: `qa` runs an advance's features and UBM posteriors, `qi` (below)
  // its iVector steps, `q` its acoustic model (behind events of both), `qc` its search.  Stage A of advance n + 1 touches rows and slots stage B of advance n
  // does not (new frames / new chunks vs. the ones already scheduled), so the only ordering between them is per queue.
  hipStream_t q = nullptr, qa = nullptr, qc = nullptr;      // qc: the search of an advance (behind q's event), under the next advance's acoustic model
#ifndef RS_STREAM_DEPTH
#define RS_STREAM_DEPTH 4      // (2 / 3 / 4: 35.2 / 27.3 / 24.5 ms per 64 x 30 s step, profiles/micro/stream_depth.sh; at 4 the host no longer waits for the device)
#endif
  static constexpr int kDepth = RS_STREAM_DEPTH;                               // advances in flight at most <= arena / staging sets (DecodeContext::kSets)
  hipEvent_t ev_a[kDepth] = {}, ev_b[kDepth] = {}, ev_done[kDepth] = {};       // per set: stage A issued / log-likelihoods issued / the advance finished
  // qi: the iVector steps of an advance (estimator state in, one accumulate / products / solve per new chunk, state out), behind
  // qa's event at the UBM posteriors.  The chain is the longest sequential piece of an advance (~300 us of dependent small kernels);
  // on its own queue the next advance's features and posteriors run beside it instead of behind it.
  hipStream_t qi = nullptr;
  hipEvent_t ev_f[kDepth] = {}, ev_i[kDepth] = {};                             // per set: posteriors issued (qa) / iVectors issued (qi)
  std::unique_ptr<Timer> tm_i[kDepth];
  bool pending[kDepth] = {};                                                   // an advance that used this set may still run
  std::vector<rs_stream *> open_streams;                                       // every stream that holds a slot (a device failure nobody can attribute poisons them all)
  std::unique_ptr<Timer> tm_a[kDepth], tm_b[kDepth], tm_c[kDepth];
  // device time of set `par`'s advance into the pool's totals (its done event has been waited for)
  // (device time is SAMPLED: ten event records per advance were a fifth of an advance's issue time on the host, so only every
  // kTimedEvery-th advance -- and every finishing one -- carries them and counts kTimedEvery-fold)
  static constexpr int kTimedEvery = 4;
  float time_weight[kDepth] = {};
  void Account(int par, float *extra) {
    if (time_weight[par] == 0.f) return;
    const float ms[4] = {tm_a[par]->Ms(0, 1), tm_a[par]->Ms(1, 2) + tm_i[par]->Ms(0, 1), tm_b[par]->Ms(0, 1), tm_c[par]->Ms(0, 1)};
    for (int j = 0; j < 4; j++) { stage_ms[j + 1] += ms[j] * time_weight[par]; if (extra) extra[j] += ms[j]; }
  }
  long n_adv = 0;
  bool sync_each = false;        // RS_STREAM_SYNC=1: wait for every advance before returning (the behaviour before the two queues)
  void *cx = nullptr;            // Model::DecodeContext with the arenas / staging of the advances (never handed to batch calls)
  int rows = 0;                  // capacity in frame rows
  int chunk = 24, ld_c = 0, ld_ll = 0, ld_i = 0, S = 0;
  bool reg = false;              // the register-resident search runs incrementally
  float *raw = nullptr, *cm = nullptr, *nn_in = nullptr, *ll = nullptr, *finfo = nullptr, *ivec = nullptr, *dec_state = nullptr;
  int *bp = nullptr;
  int max_slots = 0;
  double *lin = nullptr, *quad = nullptr, *numf = nullptr, *x = nullptr, *cmvn_iv = nullptr, *cmvn_nn = nullptr;
  // Speaker adaptation (rs_stream_open_adapted / rs_streams_adaptation): the speaker CMVN sums + count a stream was opened with,
  // (C + 1) doubles per slot and CMVN object (read only by streams that have them: rs_stream::spk_iv / spk_nn)
  double *spk_iv = nullptr, *spk_nn = nullptr;
  // ... a pinned buffer the carried state of one open is staged in, and the event behind the copies out of it
  double *seed_h = nullptr;
  size_t seed_cap = 0;
  hipEvent_t seed_ev = nullptr;
  bool seed_pending = false;
  // Streams that have ended (finish / finalize) but are not freed: they keep their slot and rows, so that their adaptation state can
  // still be taken, until they are freed or an open / a growing stream needs the room (oldest first)
  std::vector<rs_stream *> ended;
  long long *dec_ctr = nullptr;
  // Recurrent blocks: per kLstm / kGru op (indexed like the network's ops, null elsewhere) and slot, the `delay` state rows [s_c | s_r] the
  // stream's next advance re-enters the block behind -- row (t mod delay) holds the state of the one t in
  // [ll_done - need_lext - delay, ll_done - need_lext) of that class (recurrent_walk.h: RecWalk::ring).  Written by the advance that
  // computes those rows, read by the next one; a stream's first advance reads nothing (it starts from zeros), so opening, growing,
  // reclaiming and ending a stream have nothing to do here: the state goes with the slot.
  std::vector<float *> lstm_ring;
  // rs_streams_partial on register-resident streams (decode_partial.hip): the previous call's best path per row, its length and
  // words per slot
  static constexpr int kPartialWords = 1024;          // = SearchPlan::max_words: a partial result holds as many words as a final one
  PartialRow *prow = nullptr;
  PartialAnchor *anchor = nullptr;
  int *anchor_words = nullptr;
  std::vector<int> free_slots;
  std::map<int, int> free_rows;  // start -> length
  std::vector<void *> owned;
  float host_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // host time of the sections of an advance (RS_STREAMS_TRACE)
  AdvancePlan plans[kDepth];      // the plan of the advance on each arena set: reused, so that its vectors keep their capacity (call_plan.h)
  std::vector<StreamView> views;  // ... and what it reads of the call's streams
  float stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // device time of the stages, summed over the advances since the last finish

  int AllocRows(int n) {
    for (auto it = free_rows.begin(); it != free_rows.end(); ++it)
      if (it->second >= n) {
        const int start = it->first, len = it->second;
        free_rows.erase(it);
        if (len > n) free_rows[start + n] = len - n;
        return start;
      }
    return -1;
  }
  void FreeRows(int start, int n) {
    if (n <= 0) return;
    auto it = free_rows.emplace(start, n).first;
    auto nx = std::next(it);
    if (nx != free_rows.end() && it->first + it->second == nx->first) { it->second += nx->second; free_rows.erase(nx); }
    if (it != free_rows.begin()) {
      auto pv = std::prev(it);
      if (pv->first + pv->second == it->first) { pv->second += it->second; free_rows.erase(it); }
    }
  }
};

void StreamPoolDeleter::operator()(StreamPool *p) const {
  if (!p) return;
  p->issuer.Drain(false);
  if (p->qa) (void)hipStreamSynchronize(p->qa);
  if (p->qi) (void)hipStreamSynchronize(p->qi);
  if (p->q) (void)hipStreamSynchronize(p->q);
  if (p->qc) (void)hipStreamSynchronize(p->qc);
  for (int k = 0; k < StreamPool::kDepth; k++) {
    p->tm_a[k].reset(); p->tm_b[k].reset(); p->tm_c[k].reset(); p->tm_i[k].reset();
    for (hipEvent_t e : {p->ev_a[k], p->ev_b[k], p->ev_done[k], p->ev_f[k], p->ev_i[k]}) if (e) (void)hipEventDestroy(e);
  }
  for (void *d : p->owned) (void)hipFree(d);
  if (p->seed_h) (void)hipHostFree(p->seed_h);
  if (p->seed_ev) (void)hipEventDestroy(p->seed_ev);
  for (rs_stream *st : p->ended) { st->ended = false; st->reclaimed = true; }      // (freed after their model: nothing left to release)
  if (p->q) (void)hipStreamDestroy(p->q);
  if (p->qa) (void)hipStreamDestroy(p->qa);
  if (p->qc) (void)hipStreamDestroy(p->qc);
  if (p->qi) (void)hipStreamDestroy(p->qi);
  delete p;
}

namespace {
int RoundUp(int x, int m) { return (x + m - 1) / m * m; }
int EnvInt(const char *name, int dflt) { const char *e = std::getenv(name); return e ? std::atoi(e) : dflt; }

}  // namespace

StreamPool *Model::Pool() {
  if (pool_) return pool_.get();
  ToDevice();
  RS_HIP(hipSetDevice(opts_.device_id));
  std::unique_ptr<StreamPool, StreamPoolDeleter> p(new StreamPool());
  const Nnet &nn = am_.nnet;
  const int C = fc_.mfcc.nceps, P = nn.output_dim;
  p->chunk = opts_.frames_per_chunk;
  p->rows = RoundUp(std::max(EnvInt("RS_STREAM_POOL_ROWS", 1 << 19), 4 * p->chunk), p->chunk);      // 2^19 frames = 87 min of live audio; ~10 KB per row for a 2000-pdf model
  p->max_slots = std::max(EnvInt("RS_STREAM_SLOTS", 512), 1);
  p->ld_c = RoundUp(C, 4);
  p->ld_ll = RoundUp(P, 4);
  p->S = hclg_.num_states();
  p->reg = StreamSearchIncremental(search_load_);
  RS_HIP(hipStreamCreateWithFlags(&p->q, hipStreamNonBlocking));
  RS_HIP(hipStreamCreateWithFlags(&p->qa, hipStreamNonBlocking));
  RS_HIP(hipStreamCreateWithFlags(&p->qc, hipStreamNonBlocking));
  RS_HIP(hipStreamCreateWithFlags(&p->qi, hipStreamNonBlocking));
  for (int k = 0; k < StreamPool::kDepth; k++) {
    RS_HIP(hipEventCreateWithFlags(&p->ev_f[k], hipEventDisableTiming));
    RS_HIP(hipEventCreateWithFlags(&p->ev_i[k], hipEventDisableTiming));
    p->tm_i[k].reset(new Timer(p->qi));
    RS_HIP(hipEventCreateWithFlags(&p->ev_a[k], hipEventDisableTiming));
    RS_HIP(hipEventCreateWithFlags(&p->ev_b[k], hipEventDisableTiming));
    RS_HIP(hipEventCreateWithFlags(&p->ev_done[k], hipEventDisableTiming));
    p->tm_a[k].reset(new Timer(p->qa));
    p->tm_b[k].reset(new Timer(p->q));
    p->tm_c[k].reset(new Timer(p->qc));
  }
  { const char *e = TuneEnv("RS_STREAM_SYNC"); p->sync_each = e && std::atoi(e) != 0; }
  { const char *e = std::getenv("RS_STREAM_ISSUER"); p->use_issuer = !(e && std::atoi(e) == 0); }
  if (opts_.stream_min_ticks >= 1) p->min_ticks = opts_.stream_min_ticks;      // rs_decode_opts (0: the default above)
  { const char *e = std::getenv("RS_STREAM_MIN_TICKS"); if (e && std::atoi(e) >= 1) p->min_ticks = std::atoi(e); }
  p->issuer.device = opts_.device_id;
  auto dalloc = [&](size_t bytes) {
    void *d = nullptr;
    RS_HIP(hipMalloc(&d, std::max<size_t>(bytes, 256)));
    RS_HIP(hipMemsetAsync(d, 0, std::max<size_t>(bytes, 256), p->q));
    p->owned.push_back(d);
    return d;
  };
  const size_t R = (size_t)p->rows + 8;
  p->raw = static_cast<float *>(dalloc(R * p->ld_c * 4));
  if (fc_.ie.present) p->cm = static_cast<float *>(dalloc(R * p->ld_c * 4));
  if (fc_.use_cmvn) p->nn_in = static_cast<float *>(dalloc(R * p->ld_c * 4));
  p->ll = static_cast<float *>(dalloc(R * p->ld_ll * 4));
  if (p->reg) {
    p->bp = static_cast<int *>(dalloc(R * p->S * 4));
    p->finfo = static_cast<float *>(dalloc(R * 16));
    p->dec_state = static_cast<float *>(dalloc((size_t)p->max_slots * (2 * (size_t)p->S + 4) * 4));
    p->prow = static_cast<PartialRow *>(dalloc(R * sizeof(PartialRow)));
    p->anchor = static_cast<PartialAnchor *>(dalloc((size_t)p->max_slots * sizeof(PartialAnchor)));
    p->anchor_words = static_cast<int *>(dalloc((size_t)p->max_slots * StreamPool::kPartialWords * 4));
  }
  p->dec_ctr = static_cast<long long *>(dalloc((size_t)p->max_slots * 64));
  p->lstm_ring.assign(nn.ops.size(), nullptr);
  // a recurrent block's ring: [slot][delay][StateDim()], the row width its kernel is given as RecWalk::state_w (Model::RunNnet)
  for (size_t i = 0; i < nn.ops.size(); i++) {
    const LayerOp &op = nn.ops[i];
    size_t row_floats = 0;
    if (op.kind == LayerOp::kLstm || op.kind == LayerOp::kLstmp || op.kind == LayerOp::kLstmb) row_floats = (size_t)op.lstm.delay * op.lstm.StateDim();
    else if (op.kind == LayerOp::kGru) row_floats = (size_t)op.gru.delay * op.gru.StateDim();
    else if (op.kind == LayerOp::kPgru) row_floats = (size_t)op.pgru.delay * op.pgru.StateDim();
    if (row_floats > 0) p->lstm_ring[i] = static_cast<float *>(dalloc((size_t)p->max_slots * row_floats * 4));
  }
  if (fc_.ie.present) {
    const int Di = fc_.ie.ivector_dim(), usz = Di * (Di + 1) / 2;
    p->ld_i = RoundUp(Di, 4);
    p->ivec = static_cast<float *>(dalloc(((size_t)p->rows / p->chunk + 8) * p->ld_i * 4 + 1024));
    p->lin = static_cast<double *>(dalloc((size_t)p->max_slots * Di * 8));
    p->quad = static_cast<double *>(dalloc((size_t)p->max_slots * usz * 8));
    p->numf = static_cast<double *>(dalloc((size_t)p->max_slots * 8));
    p->x = static_cast<double *>(dalloc((size_t)p->max_slots * Di * 8));
    p->cmvn_iv = static_cast<double *>(dalloc((size_t)p->max_slots * (C + 1) * 8));
    p->spk_iv = static_cast<double *>(dalloc((size_t)p->max_slots * (C + 1) * 8));
  }
  if (fc_.use_cmvn) {
    p->cmvn_nn = static_cast<double *>(dalloc((size_t)p->max_slots * (C + 1) * 8));
    p->spk_nn = static_cast<double *>(dalloc((size_t)p->max_slots * (C + 1) * 8));
  }
  RS_HIP(hipEventCreateWithFlags(&p->seed_ev, hipEventDisableTiming));
  for (int s = p->max_slots - 1; s >= 0; s--) p->free_slots.push_back(s);
  p->free_rows[0] = p->rows;
  std::unique_ptr<DecodeContext> c(new DecodeContext());
  c->stream = p->q;
  RS_HIP(hipHostMalloc((void **)&c->gemm_ovf, 64, hipHostMallocMapped));
  c->gemm_ovf[0] = c->gemm_ovf[1] = 0;
  RS_HIP(hipHostGetDevicePointer((void **)&c->gemm_ovf_dev, c->gemm_ovf, 0));
  stream_ctx_ = std::move(c);
  p->cx = stream_ctx_.get();
  RS_HIP(hipStreamSynchronize(p->q));
  RS_HIP(hipStreamSynchronize(p->qa));
  RS_HIP(hipStreamSynchronize(p->qi));
  pool_ = std::move(p);
  return pool_.get();
}

// Waits for the advances still in flight and adds their stage times to the pool's totals (and to `extra`, if given: the finishing
// call's own share).  Device errors of those advances surface here.
// A closure the issuing thread ran for an advance (its acoustic-model and search launches) threw: the advance's rows were never
// computed, its done event never recorded -- and the exception comes out in whichever later call waits for the thread, possibly one
// that has nothing to do with the streams concerned (rs_stream_open).  So wherever it is collected, every open stream of the pool is
// poisoned with its message first (the streams used to carry on with missing rows behind a stale event).
void Model::IssuerSync(StreamPool *p) {
  try {
    p->issuer.Drain();
  } catch (const std::exception &e) {
    StreamsPoisonAll(e.what());
    throw;
  } catch (...) {
    StreamsPoisonAll("an advance's deferred work failed");
    throw;
  }
}

void Model::StreamsDrain(StreamPool *p, float *extra) {
  IssuerSync(p);
  for (int k = 0; k < StreamPool::kDepth; k++) {
    const int par = (int)((p->n_adv + k) % StreamPool::kDepth);      // the oldest advance first
    if (!p->pending[par]) continue;
    RS_HIP(hipEventSynchronize(p->ev_done[par]));
    p->pending[par] = false;
    p->Account(par, extra);
  }
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) Fail(std::string("a kernel launch failed: ") + hipGetErrorString(le));
  StreamsCheckRange();
}

// An advance cannot be repeated (its rows are written, the chunk schedule has moved on): when a layer GEMM met an activation
// the fp16 split cannot carry, the model changes to the exact-FP32 kernels for everything that follows and this call fails.
void Model::StreamsCheckRange() {
  DecodeContext *cx = stream_ctx_.get();
  // (only the split-fp16 kernels raise the word, so a raised word means an advance issued on them overflowed -- whether or not a
  // batch call has moved the model to the exact kernels in the meantime)
  if (!cx || !cx->gemm_ovf) return;
  volatile int *w = static_cast<volatile int *>(cx->gemm_ovf);
  const int over = w[0], under = w[1];
  if (over != 0 || under != 0) {
    w[0] = w[1] = 0;
    exact_gemm_.store(true);
    range_retries_.fetch_add(1);
    if (under != 0) precision_retries_.fetch_add(1);
    StreamsPoisonAll();        // (any of the advances in flight may be the one: their log-likelihood rows are not numbers / not the FP32 result)
    if (over != 0)
      Fail("an activation exceeded the range of the split-fp16 layer GEMMs (|x| >= 65520) during a stream advance; the model now uses the "
           "exact-FP32 kernels (RS_GEMM_B3=0 selects them from the start)");
    Fail("an activation row below the precision range of the split-fp16 layer GEMMs (largest |x| < 2^-3) was met during a stream advance; the model "
         "now uses the exact-FP32 kernels (RS_GEMM_B3=0 selects them from the start)");
  }
}

// An ended stream gives its slot and rows back: nothing is in flight on them (the call that ended it waited for everything)
static void ReleaseEnded(StreamPool *p, rs_stream *st, bool reclaimed) {
  p->FreeRows(st->row0, st->cap);
  p->free_slots.push_back(st->slot);
  st->ended = false;
  st->reclaimed = reclaimed;
  p->ended.erase(std::remove(p->ended.begin(), p->ended.end(), st), p->ended.end());
}

// rows for a stream; ended streams that still hold theirs make room, oldest first
static int AllocRowsReclaiming(StreamPool *p, int want) {
  int row0 = p->AllocRows(want);
  while (row0 < 0 && !p->ended.empty()) { ReleaseEnded(p, p->ended.front(), true); row0 = p->AllocRows(want); }
  return row0;
}

void Model::AdaptationFresh(rs_adaptation *a) const {
  const int C = fc_.mfcc.nceps;
  *a = rs_adaptation();
  a->feat_dim = C;
  a->has_iv = fc_.ie.present;
  a->has_nn = fc_.use_cmvn;
  if (a->has_iv) {
    // the estimator as its constructor leaves it (ivector-extractor.cc: quadratic = I, linear = [prior_offset, 0, ...], no frames)
    const int Di = fc_.ie.ivector_dim();
    a->ivec_dim = Di;
    a->lin.assign(Di, 0.0);
    a->lin[0] = fc_.ie.prior_offset;
    a->quad.assign((size_t)Di * (Di + 1) / 2, 0.0);
    for (int r = 0; r < Di; r++) a->quad[(size_t)r * (r + 1) / 2 + r] = 1.0;
    a->cmvn_iv.assign(2 * (size_t)(C + 1), 0.0);
  }
  if (a->has_nn) a->cmvn_nn.assign(2 * (size_t)(C + 1), 0.0);
}

std::string Model::AdaptationMismatch(const rs_adaptation &a) const {
  const int C = fc_.mfcc.nceps, Di = fc_.ie.present ? fc_.ie.ivector_dim() : 0;
  if (a.has_iv != fc_.ie.present || a.ivec_dim != Di) return "the state's iVector dimension (" + std::to_string(a.ivec_dim) + ") is not the model's (" + std::to_string(Di) + ")";
  if (a.has_nn != fc_.use_cmvn) return std::string("the state ") + (a.has_nn ? "has" : "lacks") + " nnet-input CMVN statistics and the model " + (fc_.use_cmvn ? "has" : "lacks") + " that CMVN";
  if ((a.has_iv || a.has_nn) && a.feat_dim != C) return "the state's feature dimension (" + std::to_string(a.feat_dim) + ") is not the model's (" + std::to_string(C) + ")";
  if (a.lin.size() != (size_t)Di || a.quad.size() != (size_t)Di * (Di + 1) / 2 || a.cmvn_iv.size() != (a.has_iv ? 2 * (size_t)(C + 1) : 0) ||
      a.cmvn_nn.size() != (a.has_nn ? 2 * (size_t)(C + 1) : 0))
    return "the state's arrays do not have the model's sizes";
  return std::string();
}

void Model::StreamOpen(rs_stream *st, const rs_adaptation *state) {
  std::lock_guard<std::mutex> lk(pool_mu_);
  StreamPool *p = Pool();
  RS_HIP(hipSetDevice(opts_.device_id));
  // (this call queues on qi / qc itself.  A failure of an earlier advance's deferred work belongs to the streams that are open, not to
  // the one being opened: they are poisoned with its message and refuse their next call; the open goes ahead on the drained pool)
  try { IssuerSync(p); } catch (...) {}
  if (p->free_slots.empty() && !p->ended.empty()) ReleaseEnded(p, p->ended.front(), true);
  if (p->free_slots.empty()) Fail("too many live streams on this model (RS_STREAM_SLOTS=" + std::to_string(p->max_slots) + ")");
  const int want = RoundUp(std::max(EnvInt("RS_STREAM_INIT_FRAMES", 4096), 2 * p->chunk), p->chunk);
  const int row0 = AllocRowsReclaiming(p, want);
  if (row0 < 0) Fail("stream pool exhausted (RS_STREAM_POOL_ROWS=" + std::to_string(p->rows) + " frame rows of live audio)");
  st->slot = p->free_slots.back();
  p->free_slots.pop_back();
  st->row0 = row0;
  st->cap = want;
  // fresh estimator / search state in the slot -- or the carried one (SetAdaptationState, online-ivector-feature.cc:445-453:
  // the statistics are replaced, the CG solution keeps its constructor value [prior_offset, 0, ...]; SetCmvnState)
  if (state) {
    const int C = fc_.mfcc.nceps, C1 = C + 1, Di = state->ivec_dim, usz = Di * (Di + 1) / 2;
    const size_t need = (size_t)2 * Di + usz + 1 + 2 * (size_t)C1;
    if (p->seed_pending) { RS_HIP(hipEventSynchronize(p->seed_ev)); p->seed_pending = false; }      // (the previous open's copies have left the buffer)
    if (p->seed_cap < need) {
      if (p->seed_h) RS_HIP(hipHostFree(p->seed_h));
      p->seed_h = nullptr; p->seed_cap = 0;
      RS_HIP(hipHostMalloc((void **)&p->seed_h, need * 8, hipHostMallocDefault));
      p->seed_cap = need;
    }
    double *h_lin = p->seed_h, *h_quad = h_lin + Di, *h_numf = h_quad + usz, *h_x = h_numf + 1, *h_iv = h_x + Di, *h_nn = h_iv + C1;
    st->spk0.assign(4 * (size_t)C1, 0.0);
    if (state->has_iv) {
      std::memcpy(h_lin, state->lin.data(), 8 * (size_t)Di);
      std::memcpy(h_quad, state->quad.data(), 8 * (size_t)usz);
      *h_numf = state->num_frames;
      for (int i = 0; i < Di; i++) h_x[i] = i == 0 ? fc_.ie.prior_offset : 0.0;
      std::memcpy(h_iv, state->cmvn_iv.data(), 8 * (size_t)C1);
      std::memcpy(st->spk0.data(), state->cmvn_iv.data(), 8 * 2 * (size_t)C1);
      st->spk_iv = state->cmvn_iv[C] > 0.0;
      // (the estimator's state on the iVector steps' queue, the speaker sums on the features' queue: the queues that read them)
      RS_HIP(hipMemcpyAsync(p->lin + (size_t)st->slot * Di, h_lin, 8 * (size_t)Di, hipMemcpyHostToDevice, p->qi));
      RS_HIP(hipMemcpyAsync(p->quad + (size_t)st->slot * usz, h_quad, 8 * (size_t)usz, hipMemcpyHostToDevice, p->qi));
      RS_HIP(hipMemcpyAsync(p->numf + st->slot, h_numf, 8, hipMemcpyHostToDevice, p->qi));
      RS_HIP(hipMemcpyAsync(p->x + (size_t)st->slot * Di, h_x, 8 * (size_t)Di, hipMemcpyHostToDevice, p->qi));
      if (st->spk_iv) RS_HIP(hipMemcpyAsync(p->spk_iv + (size_t)st->slot * C1, h_iv, 8 * (size_t)C1, hipMemcpyHostToDevice, p->qa));
    }
    if (state->has_nn) {
      std::memcpy(h_nn, state->cmvn_nn.data(), 8 * (size_t)C1);
      std::memcpy(st->spk0.data() + 2 * C1, state->cmvn_nn.data(), 8 * 2 * (size_t)C1);
      st->spk_nn = state->cmvn_nn[C] > 0.0;
      if (st->spk_nn) RS_HIP(hipMemcpyAsync(p->spk_nn + (size_t)st->slot * C1, h_nn, 8 * (size_t)C1, hipMemcpyHostToDevice, p->qa));
    }
    // one event behind both queues' copies: qa waits for qi's, the event is recorded on qa
    if (state->has_iv || state->has_nn) {
      RS_HIP(hipEventRecord(p->seed_ev, p->qi));
      RS_HIP(hipStreamWaitEvent(p->qa, p->seed_ev, 0));
      RS_HIP(hipEventRecord(p->seed_ev, p->qa));
      p->seed_pending = true;
    }
  } else if (fc_.ie.present) {
    const int Di = fc_.ie.ivector_dim(), usz = Di * (Di + 1) / 2;
    LaunchIvecInit(ivec_dev_, 1, p->lin + (size_t)st->slot * Di, p->quad + (size_t)st->slot * usz, p->x + (size_t)st->slot * Di, p->numf + st->slot, p->qi);      // (the iVector steps' queue: the estimator state is its)
  }
  RS_HIP(hipMemsetAsync(p->dec_ctr + (size_t)st->slot * 8, 0, 64, p->qc));      // (the search's queue)
  if (p->anchor) RS_HIP(hipMemsetAsync(p->anchor + st->slot, 0, sizeof(PartialAnchor), p->qc));      // no cached path yet (partials run on qc too)
  st->open = true;
  p->open_streams.push_back(st);
}

// The stream ended through a finish or a finalize that succeeded.  It keeps its slot and rows (see StreamPool::ended): nothing of
// the pool reads or writes them any more, and no later advance can fail on its behalf.
void Model::StreamEnd(rs_stream *st, bool flushed) {
  if (!st->open) return;
  std::lock_guard<std::mutex> lk(pool_mu_);
  if (!pool_) return;
  // the frames GetState covers: all of them after a finish; after a finalize those of the complete ticks (what lies beyond the last
  // complete tick is ignored, as by the results)
  st->adapt_frames = flushed ? st->frames_mfcc : std::min(st->frames_mfcc, NumFrames(kTickSamples * st->sched.ticks_done, fc_.mfcc.opts));
  st->open = false;
  st->ended = true;
  auto &os = pool_->open_streams;
  os.erase(std::remove(os.begin(), os.end(), st), os.end());
  pool_->ended.push_back(st);
}

void Model::StreamClose(rs_stream *st) {
  if (!st->open && !st->ended) return;
  std::lock_guard<std::mutex> lk(pool_mu_);
  if (!pool_) return;
  if (st->ended) { ReleaseEnded(pool_.get(), st, false); return; }
  // an advance that still uses the stream's rows / slot finishes first (a device error of it is the other streams' to report:
  // this one is going away either way)
  try { StreamsDrain(pool_.get(), nullptr); } catch (...) { pool_->issuer.Drain(false); (void)hipStreamSynchronize(pool_->qa); (void)hipStreamSynchronize(pool_->qi); (void)hipStreamSynchronize(pool_->q); (void)hipStreamSynchronize(pool_->qc); }
  pool_->FreeRows(st->row0, st->cap);
  pool_->free_slots.push_back(st->slot);
  st->open = false;
  auto &os = pool_->open_streams;
  os.erase(std::remove(os.begin(), os.end(), st), os.end());
}

// A failure that cannot be pinned on one advance's streams -- a device error that surfaced at a wait, up to three advances
// after the one that caused it; a layer GEMM that left its range in any of the advances in flight: no stream of the pool can
// trust its rows.  Everything queued is waited for, every set is free again, every open stream refuses further calls.
void Model::StreamsPoisonAll(const std::string &why) {
  StreamPool *p = pool_.get();
  if (!p) return;
  p->issuer.Drain(false);
  (void)hipStreamSynchronize(p->qa); (void)hipStreamSynchronize(p->qi); (void)hipStreamSynchronize(p->q); (void)hipStreamSynchronize(p->qc);
  (void)hipGetLastError();
  for (int k = 0; k < StreamPool::kDepth; k++) p->pending[k] = false;
  for (rs_stream *st : p->open_streams) {
    if (!st->failed && !why.empty()) st->fail_why = why;
    st->failed = true;
  }
}

// A stream outgrew its row range: move it to a range twice as long (device-to-device copies on the pool's stream).
void Model::StreamGrow(rs_stream *st, int need_frames) {
  StreamPool *p = pool_.get();
  StreamsDrain(p, nullptr);                 // both queues idle: the rows move under nobody's feet
  int want = st->cap;
  while (want < need_frames) want *= 2;
  const int row0 = AllocRowsReclaiming(p, want);
  if (row0 < 0) Fail("stream pool exhausted (RS_STREAM_POOL_ROWS=" + std::to_string(p->rows) + " frame rows of live audio)");
  const size_t n = (size_t)st->cap;
  auto mv = [&](void *base, size_t row_bytes) {
    if (base) RS_HIP(hipMemcpyAsync(static_cast<char *>(base) + (size_t)row0 * row_bytes, static_cast<char *>(base) + (size_t)st->row0 * row_bytes, n * row_bytes,
                                    hipMemcpyDeviceToDevice, p->q));
  };
  mv(p->raw, (size_t)p->ld_c * 4); mv(p->cm, (size_t)p->ld_c * 4); mv(p->nn_in, (size_t)p->ld_c * 4); mv(p->ll, (size_t)p->ld_ll * 4);
  mv(p->bp, (size_t)p->S * 4); mv(p->finfo, 16); mv(p->prow, sizeof(PartialRow));
  if (p->ivec)
    RS_HIP(hipMemcpyAsync(p->ivec + (size_t)(row0 / p->chunk) * p->ld_i, p->ivec + (size_t)(st->row0 / p->chunk) * p->ld_i,
                          (size_t)(st->cap / p->chunk) * p->ld_i * 4, hipMemcpyDeviceToDevice, p->q));
  RS_HIP(hipStreamSynchronize(p->q));       // ... and stage A of the next advance (other queue) finds them in place
  p->FreeRows(st->row0, st->cap);
  st->row0 = row0;
  st->cap = want;
}

// One advance over `n` streams of this model.  final: end of input for all of them; results go to `res` (n utterances).
void Model::StreamsAdvance(rs_stream *const *streams, int n, bool final, int nbest, float lat_scale, Result *res) {
  std::lock_guard<std::mutex> lk(pool_mu_);
  try {
    StreamsAdvanceLocked(streams, n, final, nbest, lat_scale, res);
  } catch (const DeviceError &) {
    StreamsPoisonAll();        // a HIP error: which advance, which streams -- unknown
    throw;
  } catch (...) {
    // The advance may have queued part of its work on a set it never marked pending: whatever is queued finishes before the set
    // can be handed out again (the call's own streams are poisoned by the caller, api.cc).
    if (pool_) { pool_->issuer.Drain(false); (void)hipStreamSynchronize(pool_->qa); (void)hipStreamSynchronize(pool_->qi); (void)hipStreamSynchronize(pool_->q); (void)hipStreamSynchronize(pool_->qc); }
    throw;
  }
}

// ---------------------------------------------------------------------------------------------------------- one advance, stage by stage
namespace {
// The host's time per section of an advance, into StreamPool::host_ms (RS_STREAMS_TRACE: plan | arena + uploads | issue of stage A | B | C)
struct HostClock {
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  void Mark(float *ms) {
    const auto now = std::chrono::steady_clock::now();
    *ms += std::chrono::duration<float, std::milli>(now - last).count();
    last = now;
  }
};
float MsSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
void MarkIf(bool timed, Timer *t) { if (timed) t->Mark(); }
float *AllocGuarded(DeviceArena &arena, int rows, int ld, int guard) { return arena.AllocT<float>(((size_t)rows + 2 * guard) * ld) + (size_t)guard * ld; }
}  // namespace

// The arena / staging set an advance runs on and what its upload left there
struct AdvanceSet {
  int par = 0;
  DeviceArena *arena = nullptr;
  HostArena *harena = nullptr;
  int *d_is = nullptr;           // AdvancePlan::stage on the device
  int16_t *d_pcm = nullptr;      // the new samples of the streams with new frames, back to back
  bool timed = false;            // this advance carries the stage timers' events (StreamPool::kTimedEvery)
  int guard = 0;
};

// Stages B and C of an advance -- the acoustic model and the scatter into the pool on q, the search windows on qc -- as the values
// they need: everything queues on q / qc and needs nothing the caller's thread computes later.  A finishing call runs it itself
// (Model::IssueStagesBC); everyone else hands it to the pool's issuing thread.  Its buffers came out of the arena in the caller's thread.
struct StagesBC {
  StreamPool *p = nullptr;
  DeviceArena *arena = nullptr;
  int par = 0;
  bool final = false, timed = false, reg_windows = false, exact = false;
  int *ovf_dev = nullptr;
  uint64_t gemm_rec_gen = 0;      // (keep_intermediates: the advance's generation of recorded layer GEMM launches)
  int nI = 0, nN = 0, rowsN = 0, framesN = 0, maxTn = 1, n = 0, n_sub = 0;
  bool have_sub = false;
  const int *d_nsrc = nullptr, *d_nfb = nullptr, *d_nrb = nullptr, *d_nriv = nullptr, *d_nll = nullptr, *d_nlls = nullptr, *d_slots = nullptr;
  // recurrent networks: per nnet segment its frames; the stream's frames before it and its slot (h_lstm: both, staged on the host)
  const int *d_nT = nullptr, *h_lstm = nullptr;
  int *d_lstm_t0 = nullptr, *d_lstm_slot = nullptr;
  std::vector<float *> bufp;
  std::vector<int> buf_ld;
  std::vector<ActImage> imgs;
  int *frame_rows = nullptr;
  BatchGeom gd;
  DenseWork dw;
  DecodeOptsDev dopts;
  RegLaunch reg;                 // the window launch (reg_windows)
  SearchPlan *sp = nullptr;      // (a finishing call only)
};

// Coalescing: nothing but the end of a stream reads what an advance computes, and an advance is chains of small dependent launches
// (the iVector estimator's per-chunk chain is the longest queue of a step: ~300 us per advance whatever the number of chunks) -- so
// a call that brings less than min_ticks ticks of new audio on every stream leaves it to the next one.  The chunk / iVector
// schedule is a function of the sample counts, not of the calls (ScheduleChunks): same rows, same results as with one
// advance per tick or one at the end (the three delivery patterns of the stream tests).  RS_STREAM_MIN_TICKS=1: every call works.
static bool LeftToTheNextCall(const StreamPool *p, rs_stream *const *streams, int n) {
  if (p->min_ticks <= 1) return false;
  long most = 0;
  for (int i = 0; i < n; i++) most = std::max(most, (long)(streams[i]->n_samples / kTickSamples) - streams[i]->sched.ticks_done);
  return most < p->min_ticks;
}

PlanConfig Model::PlanCfg() const {
  PlanConfig c;
  c.window = fc_.mfcc.win; c.shift = fc_.mfcc.shift;
  c.chunk = opts_.frames_per_chunk;
  c.L = L_; c.R = R_; c.Rm = am_.nnet.right_context;
  c.has_iv = fc_.ie.present;
  c.sl = c.has_iv ? fc_.ie.splice_left : 0; c.sr = c.has_iv ? fc_.ie.splice_right : 0;
  c.fsf = opts_.frame_subsampling_factor;
  return c;
}

// Consecutive advances rotate over kDepth arena / staging sets, so the host plans and issues the next advances while earlier ones
// still run: the advance kDepth calls ago used this set and has to be over (it normally is)
int Model::AdvanceTakeSet(StreamPool *p, bool final) {
  const int par = (int)(p->n_adv % StreamPool::kDepth);
  if (final) IssuerSync(p);      // a finishing call issues everything itself, behind what the issuing thread still holds
  if (p->pending[par]) {
    const auto w0 = std::chrono::steady_clock::now();
    IssuerSync(p);         // (its done event has been recorded)
    RS_HIP(hipEventSynchronize(p->ev_done[par]));
    p->stage_ms[7] += MsSince(w0);
    p->pending[par] = false;
    p->Account(par, nullptr);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) Fail(std::string("a kernel launch failed: ") + hipGetErrorString(le));
    StreamsCheckRange();
  }
  return par;
}

// The plan of the advance (call_plan.h), in its two steps around the move of the streams that outgrew their rows
void Model::AdvancePlanStreams(StreamPool *p, rs_stream *const *streams, int n, bool flush, bool final, AdvancePlan *plan) {
  const PlanConfig cfg = PlanCfg();
  std::vector<StreamView> &views = p->views;
  views.resize(n);
  for (int i = 0; i < n; i++) {
    const rs_stream &st = *streams[i];
    StreamView &v = views[i];
    v.n_samples = st.n_samples; v.sched = st.sched;
    v.frames_mfcc = st.frames_mfcc; v.stats_done = st.stats_done; v.ll_done = st.ll_done; v.frames_decoded = st.frames_decoded; v.dec_started = st.dec_started;
    v.slot = st.slot; v.spk_iv = st.spk_iv; v.spk_nn = st.spk_nn;
  }
  PlanAdvanceSchedule(cfg, views.data(), n, flush, plan);
  for (int i = 0; i < n; i++) {
    if (plan->pl[i].avail + 2 > streams[i]->cap) StreamGrow(streams[i], plan->pl[i].avail + 2);
    views[i].row0 = streams[i]->row0;
  }
  PlanAdvanceRows(cfg, views.data(), n, flush, final, plan);
}

// The set's arenas handed back, then the uploads on qa: the index arrays in one copy, the new samples in another
void Model::AdvanceUpload(StreamPool *p, rs_stream *const *streams, const AdvancePlan &plan, bool final, AdvanceSet *set) {
  const int n = plan.n;
  DeviceArena &arena = *set->arena;
  HostArena &harena = *set->harena;
  hipStream_t qa = p->qa;
  set->guard = L_ + R_ + 8;
  arena.Reset(qa);
  harena.Reset(qa);
  const size_t n_is = plan.stage.size(), pcm_total = plan.pcm_total;
  set->d_is = arena.AllocT<int>(n_is + 16);
  {
    int *hp = harena.AllocT<int>(n_is + 16);
    std::memcpy(hp, plan.stage.data(), n_is * 4);
    RS_HIP(hipMemcpyAsync(set->d_is, hp, n_is * 4, hipMemcpyHostToDevice, qa));
  }
  set->d_pcm = arena.AllocT<int16_t>(pcm_total + 512);
  if (pcm_total) {
    int16_t *hp = harena.AllocT<int16_t>(pcm_total + 512);
    const int shift = fc_.mfcc.shift;
    size_t o = 0;
    for (int i = 0; i < n; i++) {
      const rs_stream &st = *streams[i];
      if (plan.pl[i].avail <= plan.pl[i].mf0) continue;
      const long first = (long)plan.pl[i].mf0 * shift, cnt = st.n_samples - first;
      std::memcpy(hp + o, st.pcm.data() + (first - st.pcm_start), sizeof(int16_t) * (size_t)cnt);
      o += (size_t)cnt;
    }
    RS_HIP(hipMemcpyAsync(set->d_pcm, hp, sizeof(int16_t) * pcm_total, hipMemcpyHostToDevice, qa));
  }
  const int par = set->par;
  p->tm_a[par]->Reset(); p->tm_b[par]->Reset(); p->tm_c[par]->Reset(); p->tm_i[par]->Reset();
  set->timed = final || p->n_adv % StreamPool::kTimedEvery == 0;
  p->time_weight[par] = final ? 1.f : (set->timed ? (float)StreamPool::kTimedEvery : 0.f);
  MarkIf(set->timed, p->tm_a[par].get());
}

// Stage A on qa: 1. MFCC of the new frames, straight into the pool; 2. CMVN resumed from the parked sums; 3. for the streams with
// new chunks splice + LDA + UBM posteriors over the not-yet-accumulated frames -- and on qi, behind them, the estimator's steps
void Model::AdvanceStageA(StreamPool *p, const AdvancePlan &plan, const AdvanceSet &set) {
  const AdvancePlan::Offsets &o = plan.o;
  const int par = set.par, ld_c = p->ld_c, nM = plan.nM, rowsM = plan.rowsM;
  const bool timed = set.timed;
  DeviceArena &arena = *set.arena;
  hipStream_t qa = p->qa;
  Timer *tma = p->tm_a[par].get();
  auto D = [&](size_t off) { return set.d_is + off; };
  if (nM > 0) {
    BatchGeom g;
    g.n_utts = nM; g.total_rows = rowsM; g.total_frames = rowsM;
    g.d_sample_off = reinterpret_cast<const int64_t *>(D(o.mso)); g.d_num_frames = D(o.mT); g.d_row_base = D(o.mrb);
    g.d_frame0 = D(o.mf0);
    int *ru = arena.AllocT<int>(rowsM), *rt = arena.AllocT<int>(rowsM);
    LaunchRowGeometry(nM, rowsM, 0, D(o.mrb), nullptr, ru, rt, nullptr, qa);
    g.d_row_utt = ru; g.d_row_t = rt;
    LaunchBaseFeatures(plan.max_feat_frames, g, set.d_pcm, p->raw, ld_c, qa, false, D(o.mout));
    BatchGeom gc;
    gc.n_utts = nM; gc.d_num_frames = D(o.cT); gc.d_row_base = D(o.crb);
    const bool spk_iv = plan.any_spk_iv, spk_nn = plan.any_spk_nn;
    if (fc_.ie.present) LaunchOnlineCmvn(cmvn_iv_dev_, gc, p->raw, p->cm, ld_c, qa, D(o.ctb), p->cmvn_iv, D(o.cslot), spk_iv ? p->spk_iv : nullptr, spk_iv ? D(o.cspki) : nullptr);
    if (fc_.use_cmvn)
      LaunchOnlineCmvn(cmvn_nnet_dev_, gc, p->raw, p->nn_in, ld_c, qa, D(o.ctb), p->cmvn_nn, D(o.cslot), spk_nn ? p->spk_nn : nullptr, spk_nn ? D(o.cspkn) : nullptr);
  }
  MarkIf(timed, tma);
  if (plan.nI > 0) AdvanceIvectors(p, plan, set);
  MarkIf(timed, tma);
  // the acoustic model waits for both: the features (qa) and, where there is an extractor, the iVectors (qi, itself behind qa)
  RS_HIP(hipEventRecord(p->ev_a[par], qa));
  if (plan.nI > 0) RS_HIP(hipEventRecord(p->ev_i[par], p->qi));
}

// 3. iVectors of the new chunks
void Model::AdvanceIvectors(StreamPool *p, const AdvancePlan &plan, const AdvanceSet &set) {
  const AdvancePlan::Offsets &o = plan.o;
  const int C = fc_.mfcc.nceps, sl = fc_.ie.splice_left, sr = fc_.ie.splice_right;
  const int Dl = fc_.ie.feat_dim(), Di = fc_.ie.ivector_dim(), G = fc_.ie.num_gauss(), nsel = fc_.ie.num_gselect, usz = Di * (Di + 1) / 2;
  const int ld_c = p->ld_c, ld_l = RoundUp(std::max(Dl, 1), 4), ld_i = p->ld_i;
  const int par = set.par, guard = set.guard, nI = plan.nI, rowsI = plan.rowsI, max_new_chunks = plan.max_new_chunks;
  DeviceArena &arena = *set.arena;
  hipStream_t qa = p->qa, qi = p->qi;
  Timer *tmi = p->tm_i[par].get();
  auto D = [&](size_t off) { return set.d_is + off; };
  float *seg_raw = AllocGuarded(arena, rowsI, ld_c, guard), *seg_cm = AllocGuarded(arena, rowsI, ld_c, guard);
  float *lda_raw = AllocGuarded(arena, rowsI, ld_l, guard), *lda_norm = AllocGuarded(arena, rowsI, ld_l, guard);
  LaunchCopyRows(p->raw, ld_c, D(o.isrc), seg_raw, ld_c, nullptr, rowsI, C, qa);
  LaunchCopyRows(p->cm, ld_c, D(o.isrc), seg_cm, ld_c, nullptr, rowsI, C, qa);
  BatchGeom g;
  g.n_utts = nI; g.L = sl; g.R = sr; g.total_rows = rowsI; g.guard = guard;
  g.d_num_frames = D(o.iT); g.d_row_base = D(o.irb);
  int *ru = arena.AllocT<int>(rowsI + 8), *rt = arena.AllocT<int>(rowsI + 8);
  LaunchRowGeometry(nI, rowsI, sl, D(o.irb), nullptr, ru, rt, nullptr, qa);
  g.d_row_utt = ru; g.d_row_t = rt;
  LaunchGemmRecorded(LdaPlan(ld_c).op->name, MakeGemm(LdaPlan(ld_c), {seg_raw}, {ld_c}, nullptr, 0, lda_raw, ld_l, 1), rowsI, ru, qa);
  LaunchGemmRecorded(LdaPlan(ld_c).op->name, MakeGemm(LdaPlan(ld_c), {seg_cm}, {ld_c}, nullptr, 0, lda_norm, ld_l, 1), rowsI, ru, qa);
  int *post_idx = arena.AllocT<int>((size_t)rowsI * nsel + 64);
  float *post_w = arena.AllocT<float>((size_t)rowsI * nsel + 64);
  LaunchUbmPosteriors(ivec_dev_, g, lda_norm, ld_l, post_idx, post_w, qa);
  // the estimator's steps on their own queue, behind the posteriors
  RS_HIP(hipEventRecord(p->ev_f[par], qa));
  RS_HIP(hipStreamWaitEvent(qi, p->ev_f[par], 0));
  MarkIf(set.timed, tmi);
  const float *stats_feats = fc_.ie.online_cmvn_iextractor ? lda_norm : lda_raw;
  if (Di <= 128) {
    // the new chunks of all streams: statistics side by side, then one launch that walks every stream's chunks in order on its
    // estimator state in place (round 4: state rows gathered, a five-launch chain per chunk, state rows scattered)
    IvecChunkChain(arena, g, nI, max_new_chunks, stats_feats, ld_l, post_idx, post_w, D(o.sfb), D(o.sfe), D(o.sor), D(o.sac), p->lin, p->quad, p->numf,
                   p->x, D(o.islot), p->ivec, ld_i, qi);
  } else {
    double *gamma = arena.AllocT<double>((size_t)nI * G), *wfeats = arena.AllocT<double>((size_t)nI * G * Dl);
    double *linear = arena.AllocT<double>((size_t)nI * Di), *quad = arena.AllocT<double>((size_t)nI * usz);
    double *numf = arena.AllocT<double>(nI), *x = arena.AllocT<double>((size_t)nI * Di);
    double *scratch = arena.AllocT<double>(IvecStatsScratchDoubles(ivec_dev_, nI));
    // estimator state: slots -> dense, the steps, dense -> slots (one launch each way for the four arrays)
    CopyRowsSet in_set{{{p->lin, linear, 2L * Di, 2 * Di}, {p->quad, quad, 2L * usz, 2 * usz}, {p->numf, numf, 2, 2}, {p->x, x, 2L * Di, 2 * Di}}, 4};
    LaunchCopyRowsMulti(in_set, D(o.islot), nullptr, nI, qi);
    for (int k = 0; k < max_new_chunks; k++) {
      const size_t at = (size_t)k * nI;
      LaunchIvecAccumulate(ivec_dev_, g, stats_feats, ld_l, post_idx, post_w, D(o.sfb) + at, D(o.sfe) + at, gamma, wfeats, true, qi);
      LaunchIvecStats(ivec_dev_, nI, gamma, wfeats, linear, quad, numf, scratch, qi);
      LaunchIvecSolve(ivec_dev_, nI, linear, quad, numf, x, p->ivec, ld_i, D(o.sor) + at, D(o.sac) + at, qi);
    }
    CopyRowsSet out_set{{{linear, p->lin, 2L * Di, 2 * Di}, {quad, p->quad, 2L * usz, 2 * usz}, {numf, p->numf, 2, 2}, {x, p->x, 2L * Di, 2 * Di}}, 4};
    LaunchCopyRowsMulti(out_set, nullptr, D(o.islot), nI, qi);
  }
  MarkIf(set.timed, tmi);
}

// What the search of an advance (and the collection of a finish) sees: every stream of the call, its decoder frames in the pool
static BatchGeom SearchGeom(const AdvancePlan &plan, const int *d_is) {
  BatchGeom gd;
  gd.n_utts = plan.n; gd.max_frames = plan.maxT; gd.d_num_frames = d_is + plan.o.dT; gd.d_row_base = d_is + plan.o.drb;
  return gd;
}

// 4. the acoustic model over the new chunks (+ context), 5. the search: buffers out of the arena here, the launches as a StagesBC
void Model::AdvanceStagesBC(StreamPool *p, const AdvancePlan &plan, const AdvanceSet &set, bool final, SearchPlan *sp) {
  const Nnet &nn = am_.nnet;
  const AdvancePlan::Offsets &o = plan.o;
  DeviceArena &arena = *set.arena;
  auto D = [&](size_t off) { return set.d_is + off; };
  StagesBC job;
  job.p = p; job.arena = &arena; job.par = set.par;
  job.final = final; job.timed = set.timed; job.reg_windows = sp->call.windows; job.exact = exact_gemm_.load();
  job.ovf_dev = static_cast<DecodeContext *>(p->cx)->gemm_ovf_dev;
  job.gemm_rec_gen = GemmRecordJoined();
  job.nI = plan.nI; job.nN = plan.nN; job.rowsN = plan.rowsN; job.framesN = plan.framesN; job.maxTn = std::max(plan.maxTn, 1); job.n = plan.n;
  job.n_sub = (int)plan.n_lldst.size(); job.have_sub = !plan.n_llsrc.empty();
  job.d_nsrc = D(o.nsrc); job.d_nfb = D(o.nfb); job.d_nrb = D(o.nrb); job.d_nriv = D(o.nriv); job.d_nll = D(o.nll); job.d_nlls = D(o.nlls); job.d_slots = D(o.slots);
  job.bufp.assign(nn.bufs.size(), nullptr);
  job.buf_ld.resize(nn.bufs.size());
  for (size_t b = 0; b < nn.bufs.size(); b++) job.buf_ld[b] = RoundUp(nn.bufs[b].dim, 4);
  if (plan.nN > 0) {
    for (size_t b = 0; b < nn.bufs.size(); b++) job.bufp[b] = AllocGuarded(arena, plan.rowsN, job.buf_ld[b], set.guard);
    job.imgs = AllocImages(arena, plan.rowsN);
    job.frame_rows = arena.AllocT<int>(plan.framesN + 8);
    if (nn.recurrent) {
      // where each segment's stream stands (its log-likelihood frames so far: the segment covers [t0, t1)) and its slot
      const int nN = plan.nN;
      int *h = set.harena->AllocT<int>(2 * (size_t)nN + 8), *dv = arena.AllocT<int>(2 * (size_t)nN + 8);
      for (int k = 0; k < nN; k++) { h[k] = plan.pl[plan.N_idx[k]].t0; h[nN + k] = plan.slots[plan.N_idx[k]]; }
      job.d_nT = D(o.nT); job.h_lstm = h; job.d_lstm_t0 = dv; job.d_lstm_slot = dv + nN;      // (copied on q, in front of the acoustic model)
    }
  }
  job.gd = SearchGeom(plan, set.d_is);
  DenseWork &dw = job.dw;
  std::memset(&dw, 0, sizeof(dw));
  dw.bp = p->bp; dw.frame_info = p->finfo; dw.state_cost = p->dec_state; dw.counters = p->dec_ctr;
  dw.win_begin = D(o.wb); dw.win_end = D(o.we); dw.win_final = D(o.wf); dw.pool_row = D(o.row0); dw.slot = D(o.slots);
  job.dopts = sp->dopts;
  job.reg = sp->call.reg;
  job.sp = sp;
  if (final || !p->use_issuer) IssueStagesBC(job);
  else p->issuer.Submit([this, job = std::move(job)] { IssueStagesBC(job); });
}

void Model::IssueStagesBC(const StagesBC &j) {
  StreamPool *p = j.p;
  const Nnet &nn = am_.nnet;
  const int C = fc_.mfcc.nceps, P = nn.output_dim, fsf = opts_.frame_subsampling_factor, par = j.par;
  hipStream_t q = p->q, qc = p->qc;
  Timer *tb = p->tm_b[par].get(), *tc = p->tm_c[par].get();
  SampleGemmMode(j.exact, j.ovf_dev);      // (thread-local: the issuing thread's launches run in the mode this advance was planned in)
  GemmRecordJoin(j.gemm_rec_gen);
  RS_HIP(hipStreamWaitEvent(q, p->ev_a[par], 0));
  if (j.nI > 0) RS_HIP(hipStreamWaitEvent(q, p->ev_i[par], 0));
  MarkIf(j.timed, tb);
  if (j.nN > 0) {
    const float *nn_src = fc_.use_cmvn ? p->nn_in : p->raw;
    LaunchCopyRows(nn_src, p->ld_c, j.d_nsrc, j.bufp[nn.input_buf], j.buf_ld[nn.input_buf], nullptr, j.rowsN, C, q);
    LaunchFrameRows(j.nN, j.nN, j.framesN, L_, j.maxTn, j.d_nfb, j.d_nrb, j.frame_rows, q);
    RowMaps row_maps;
    row_maps.maps.push_back({0, 0, j.frame_rows, j.framesN});
    if (fsf > 1 && j.have_sub) row_maps.maps.push_back({0, 0, j.d_nlls, j.n_sub, 0, fsf});      // the layers only the decoder's frames read
    LstmCall lstm_call;
    if (j.h_lstm) RS_HIP(hipMemcpyAsync(j.d_lstm_t0, j.h_lstm, sizeof(int) * 2 * (size_t)j.nN, hipMemcpyHostToDevice, q));
    lstm_call.n_utts = j.nN; lstm_call.num_frames = j.d_nT; lstm_call.row_base = j.d_nrb;
    lstm_call.t0 = j.d_lstm_t0; lstm_call.slot = j.d_lstm_slot; lstm_call.rings = &p->lstm_ring;
    RunNnet(j.bufp, j.buf_ld, p->ivec, p->ld_i, j.d_nriv, j.rowsN, row_maps, 1, 0, nn.ops.size(), q, &j.imgs, &lstm_call);
    if (fsf == 1) LaunchCopyRows(j.bufp[nn.output_buf], j.buf_ld[nn.output_buf], j.frame_rows, p->ll, p->ld_ll, j.d_nll, j.framesN, P, q);
    else if (j.n_sub > 0) LaunchCopyRows(j.bufp[nn.output_buf], j.buf_ld[nn.output_buf], j.d_nlls, p->ll, p->ld_ll, j.d_nll, j.n_sub, P, q);
  }
  MarkIf(j.timed, tb);
  // the search on its own queue: the next advance's acoustic model does not wait for it
  RS_HIP(hipEventRecord(p->ev_b[par], q));
  RS_HIP(hipStreamWaitEvent(qc, p->ev_b[par], 0));
  MarkIf(j.timed, tc);
  if (j.final) AllocSearch(j.sp, *j.arena, qc);
  if (j.reg_windows && (j.final || j.nN > 0)) {      // (an advance without new log-likelihood rows has nothing to search)
    DenseWork dw2 = j.dw;
    if (j.final) { dw2 = j.sp->dw; dw2.bp = j.dw.bp; dw2.frame_info = j.dw.frame_info; dw2.state_cost = j.dw.state_cost; dw2.counters = j.dw.counters;
                   dw2.win_begin = j.dw.win_begin; dw2.win_end = j.dw.win_end; dw2.win_final = j.dw.win_final; dw2.pool_row = j.dw.pool_row; dw2.slot = j.dw.slot; }
    LaunchDecodeReg(hclg_dev_, reg_dev_, j.dopts, j.gd, p->ll, p->ld_ll, dw2, j.reg, 0, 0, qc);
    if (j.final) LaunchCopyRows(p->dec_ctr, 16, j.d_slots, j.sp->w.counters, 16, nullptr, j.n, 16, qc);
  } else if (j.final) {
    LaunchSearch(j.sp, j.gd, p->ll, p->ld_ll, qc);
  }
  MarkIf(j.timed, tc);
  RS_HIP(hipEventRecord(p->ev_done[par], qc));
  const hipError_t le = hipGetLastError();      // (per thread: a failed launch of this job is seen here)
  if (le != hipSuccess) Fail(std::string("a kernel launch failed: ") + hipGetErrorString(le));
}

// What the advance did, into the streams: the schedule's cursor, the frames done per stage; samples no longer needed go
void Model::AdvanceBookkeeping(StreamPool *p, rs_stream *const *streams, const AdvancePlan &plan, int par, bool searched) {
  const int shift = fc_.mfcc.shift, fsf = opts_.frame_subsampling_factor;
  for (int i = 0; i < plan.n; i++) {
    rs_stream &st = *streams[i];
    const StreamAdvance &a = plan.pl[i];
    st.sched = a.sched;
    st.frames_mfcc = a.avail;
    st.stats_done = a.sb;
    st.ll_done = a.t1;
    if (searched) { st.frames_decoded = (a.t1 + fsf - 1) / fsf; st.dec_started = true; }
    // samples before the first frame that is not complete yet are not needed again (online-feature.cc:186-203)
    const long keep_from = (long)a.avail * shift;
    if (!st.keep_pcm && keep_from > st.pcm_start) {
      st.pcm.erase(st.pcm.begin(), st.pcm.begin() + std::min<long>(keep_from - st.pcm_start, (long)st.pcm.size()));
      st.pcm_start = keep_from;
    }
  }
  p->pending[par] = true;         // (its done event is recorded by the StagesBC)
  p->n_adv++;
}

// The end of a finishing call: every advance in flight waited for, results, intermediates, timings
void Model::AdvanceFinish(StreamPool *p, rs_stream *const *streams, const AdvancePlan &plan, const AdvanceSet &set, SearchPlan &sp, bool flush, int nbest,
                          float lat_scale, std::chrono::steady_clock::time_point wall0, Result *res) {
  const Nnet &nn = am_.nnet;
  const bool has_iv = fc_.ie.present;
  const int C = fc_.mfcc.nceps, P = nn.output_dim, chunk = p->chunk, fsf = opts_.frame_subsampling_factor, Di = has_iv ? fc_.ie.ivector_dim() : 0;
  const int n = plan.n, par = set.par, ld_c = p->ld_c, ld_i = p->ld_i;
  hipStream_t qc = p->qc;
  float own[4] = {0.f, 0.f, 0.f, 0.f};
  // every earlier advance first (their time is the stream's, not this call's), then this one
  for (int k = 1; k <= StreamPool::kDepth; k++) {
    const int other = (par + k) % StreamPool::kDepth;       // oldest first; k = kDepth: this call's own
    if (!p->pending[other]) continue;
    RS_HIP(hipEventSynchronize(p->ev_done[other]));
    p->pending[other] = false;
    p->Account(other, other == par ? own : nullptr);
  }
  StreamsCheckRange();
  res->utts.resize(n);
  for (int i = 0; i < n; i++) res->utts[i].num_frames = plan.avails[i];
  Timer tmr(qc);
  tmr.Mark();
  CollectResults(sp, *static_cast<DecodeContext *>(p->cx), par, SearchGeom(plan, set.d_is), plan.avails.data(), p->ll, p->ld_ll, nbest, lat_scale, qc, res->utts.data(),
                 res->timings);
  tmr.Mark();
  if (opts_.keep_intermediates) {
    const float *fin = fc_.use_cmvn ? p->nn_in : p->raw;
    for (int i = 0; i < n; i++) {
      UttResult &ur = res->utts[i];
      const rs_stream &st = *streams[i];
      const int T = flush ? plan.pl[i].avail : plan.pl[i].t1, nch = std::max((T + chunk - 1) / chunk, 1), T_dec = (T + fsf - 1) / fsf;
      ur.feat_dim = C; ur.num_pdfs = P; ur.ivec_dim = Di; ur.ivec_rows = has_iv ? nch : 0;
      if (T == 0) continue;
      ur.feats.resize((size_t)T * C);
      ur.loglikes.resize((size_t)T_dec * P);
      RS_HIP(hipMemcpy2D(ur.feats.data(), sizeof(float) * C, fin + (size_t)st.row0 * ld_c, sizeof(float) * ld_c, sizeof(float) * C, T, hipMemcpyDeviceToHost));
      RS_HIP(hipMemcpy2D(ur.loglikes.data(), sizeof(float) * P, p->ll + (size_t)st.row0 * p->ld_ll, sizeof(float) * p->ld_ll, sizeof(float) * P, T_dec, hipMemcpyDeviceToHost));
      if (has_iv) {
        ur.ivector.resize((size_t)nch * Di);
        RS_HIP(hipMemcpy2D(ur.ivector.data(), sizeof(float) * Di, p->ivec + (size_t)(st.row0 / chunk) * ld_i, sizeof(float) * ld_i, sizeof(float) * Di, nch,
                           hipMemcpyDeviceToHost));
      }
    }
  }
  { const hipError_t le = hipGetLastError(); if (le != hipSuccess) Fail(std::string("a kernel launch failed: ") + hipGetErrorString(le)); }
  // stage times of the whole stream(s): this call plus the advances since the previous finish on this model; [7] = this call alone
  res->timings[7] = MsSince(wall0);
  for (int k = 0; k < 4; k++) res->timings[k + 1] = p->stage_ms[k + 1];
  res->timings[5] = tmr.Ms(0, 1);
  res->timings[6] = p->stage_ms[6] + res->timings[7];
  // RS_STREAMS_TRACE=1: where the host's time went since the last finish -- inside the advance calls, and of that waiting for the
  // advance three calls back to leave its arena set (the device is the bottleneck when that is most of it)
  static const bool trace = [] { const char *e = TuneEnv("RS_STREAMS_TRACE"); return e && std::atoi(e) != 0; }();
  if (trace) {
    std::fprintf(stderr, "streams: %.2f ms in advance calls, %.2f ms of it waiting for the device; plan %.2f, arena + uploads %.2f, issue of stage A %.2f, B %.2f, C %.2f\n",
                 p->stage_ms[6], p->stage_ms[7], p->host_ms[0], p->host_ms[1], p->host_ms[2], p->host_ms[3], p->host_ms[4]);
    for (float &v : p->host_ms) v = 0.f;
  }
  for (float &v : p->stage_ms) v = 0.f;
}

// queues: qa = features + UBM posteriors, qi = the iVector steps (stage A); q = acoustic model, qc = search (stages B and C, behind
// stage A's events).  no_flush (rs_streams_finalize): the end of the streams as the reference reaches it after an endpoint --
// FinalizeDecoding() without InputFinished() (online2-wav-nnet3-latgen-faster.cc:270-278): the ticks completed are scheduled like by
// any advance, nothing is flushed, and the final stage runs over the decoder frames those ticks give
void Model::StreamsAdvanceLocked(rs_stream *const *streams, int n, bool final, int nbest, float lat_scale, Result *res, bool every_tick, bool no_flush) {
  const bool flush = final && !no_flush;
  StreamPool *p = Pool();
  RS_HIP(hipSetDevice(opts_.device_id));
  if (!final && !every_tick && LeftToTheNextCall(p, streams, n)) return;
  DecodeContext &cx = *static_cast<DecodeContext *>(p->cx);
  AdvanceSet set;
  set.par = AdvanceTakeSet(p, final);
  set.arena = &cx.arena[set.par];
  set.harena = &cx.host_arena[set.par];
  SampleGemmMode(exact_gemm_.load(), cx.gemm_ovf_dev);
  GemmRecordJoin(GemmRecordBegin());
  HostClock clock;
  const auto wall0 = clock.last;
  AdvancePlan &plan = p->plans[set.par];
  AdvancePlanStreams(p, streams, n, flush, final, &plan);
  // the search of this call: the streams' new windows (a finishing call that wants a lattice: the retained rows, like a batch)
  SearchPlan sp;
  SearchRequest rq = SearchRequestFor(n, plan.maxT, nbest, lat_scale);
  rq.stream_window = true; rq.any_final = final;
  PlanSearch(rq, &sp);
  sp.want_alignment = final && opts_.emit_alignment != 0;
  const bool reg_windows = sp.call.windows;
  clock.Mark(&p->host_ms[0]);
  AdvanceUpload(p, streams, plan, final, &set);
  clock.Mark(&p->host_ms[1]);
  AdvanceStageA(p, plan, set);
  clock.Mark(&p->host_ms[2]);
  AdvanceStagesBC(p, plan, set, final, &sp);
  clock.Mark(&p->host_ms[3]);
  clock.Mark(&p->host_ms[4]);
  AdvanceBookkeeping(p, streams, plan, set.par, /*searched=*/reg_windows && (final || plan.nN > 0));
  if (!final) {
    // No wait here: the next advance is planned and issued while this one runs.  What it did on the device is accounted for --
    // and a device error of it reported -- by whichever later call of this model waits for it.
    if (p->sync_each) StreamsDrain(p, nullptr);
    p->stage_ms[6] += MsSince(wall0);
    return;
  }
  AdvanceFinish(p, streams, plan, set, sp, flush, nbest, lat_scale, wall0, res);
}

// ---------------------------------------------------------------------------------------------------------- partial results
// rs_streams_partial: what rs_streams_advance does, for every tick the accepted samples complete (no coalescing: a caller that
// asks for a partial wants the frames its audio allows), then per stream the best path over the decoder frames searched so far
// without final costs (GetBestPath(end_of_utterance = false)).
//   * register-resident streams: PartialRegKernel (decode_partial.hip) over the parked frontier and the back-pointer rows in the
//     pool; the previous call's best path, cached per row, keeps each call's traceback to the frames since that path;
//   * streams whose search is deferred to finish (graphs the register-resident search cannot hold, RS_DECODER=dense|sparse|hash):
//     the finish-time search over the log-likelihood rows so far in a scratch arena, its final stage told to ignore final costs
//     (DecodeOptsDev::no_final).  O(frames so far) per call.
// Nothing an advance or a finish reads is written: a later rs_streams_finish gives what it gives without the partial calls.
void Model::StreamsPartial(rs_stream *const *streams, int n, Result *res) {
  std::lock_guard<std::mutex> lk(pool_mu_);
  try {
    StreamsPartialLocked(streams, n, res);
  } catch (const DeviceError &) {
    StreamsPoisonAll();
    throw;
  } catch (...) {
    if (pool_) { pool_->issuer.Drain(false); (void)hipStreamSynchronize(pool_->qa); (void)hipStreamSynchronize(pool_->qi); (void)hipStreamSynchronize(pool_->q); (void)hipStreamSynchronize(pool_->qc); }
    throw;
  }
}

void Model::StreamsPartialLocked(rs_stream *const *streams, int n, Result *res) {
  StreamPool *p = Pool();
  RS_HIP(hipSetDevice(opts_.device_id));
  bool more = false;
  for (int i = 0; i < n; i++) more = more || streams[i]->n_samples / kTickSamples > streams[i]->sched.ticks_done;
  if (more) StreamsAdvanceLocked(streams, n, /*final=*/false, 1, 1.0f, nullptr, /*every_tick=*/true);
  StreamsDrain(p, nullptr);        // every advance has finished: the arena sets are free, the frontier and rows are in place
  const int fsf = opts_.frame_subsampling_factor, S = p->S;
  std::vector<int> T(n), slots(n), row0s(n);
  int maxT = 0;
  for (int i = 0; i < n; i++) {
    const rs_stream &st = *streams[i];
    T[i] = (p->reg && !st.dec_started) ? 0 : (st.ll_done + fsf - 1) / fsf;      // NumFramesDecoded()
    slots[i] = st.slot;
    row0s[i] = st.row0;
    maxT = std::max(maxT, T[i]);
  }
  DecodeContext &cx = *static_cast<DecodeContext *>(p->cx);
  const int par = (int)(p->n_adv % StreamPool::kDepth);
  DeviceArena &arena = cx.arena[par];
  HostArena &harena = cx.host_arena[par];
  hipStream_t qc = p->qc;
  SearchPlan sp;
  if (p->reg) {
    sp.n_utts = n; sp.S = S; sp.maxT = maxT; sp.max_words = StreamPool::kPartialWords;
  } else {
    SearchRequest rq = SearchRequestFor(n, maxT, 1, 1.0f);
    rq.best_path_only = true;      // (never a lattice, whatever the model's options ask of a finish)
    PlanSearch(rq, &sp);
    sp.dopts.no_final = 1;
  }
  arena.Reset(qc);
  harena.Reset(qc);
  int *d_idx = arena.AllocT<int>((size_t)3 * n + 16);
  {
    int *h = harena.AllocT<int>((size_t)3 * n + 16);
    for (int i = 0; i < n; i++) { h[i] = T[i]; h[n + i] = slots[i]; h[2 * n + i] = row0s[i]; }
    RS_HIP(hipMemcpyAsync(d_idx, h, sizeof(int) * 3 * n, hipMemcpyHostToDevice, qc));
  }
  BatchGeom gd;
  gd.n_utts = n; gd.max_frames = maxT; gd.d_num_frames = d_idx; gd.d_row_base = d_idx + 2 * n;
  if (p->reg) {
    DecodeWork &w = sp.w;
    w.max_words = sp.max_words;
    w.out_words = arena.AllocT<int>((size_t)n * sp.max_words);
    w.out_nwords = arena.AllocT<int>(n);
    w.out_costs = arena.AllocT<float>((size_t)n * 4);
    w.counters = arena.AllocT<long long>((size_t)n * 8);
    PartialWork pw;
    std::memset(&pw, 0, sizeof(pw));
    pw.state_cost = p->dec_state; pw.bp = p->bp; pw.frame_info = p->finfo; pw.loglikes = p->ll; pw.ld = p->ld_ll;
    pw.num_frames = d_idx; pw.slot = d_idx + n; pw.pool_row = d_idx + 2 * n;
    pw.anchor = p->anchor; pw.rows = p->prow; pw.anchor_words = p->anchor_words;
    pw.out_words = w.out_words; pw.out_nwords = w.out_nwords; pw.out_costs = w.out_costs; pw.counters = w.counters;
    pw.max_words = sp.max_words;
    pw.path_cap = 4 * (maxT + 2);
    pw.path = arena.AllocT<int>((size_t)n * pw.path_cap * 2);
    { const char *e = std::getenv("RS_PARTIAL_FULL_WALK"); pw.full_walk = e && std::atoi(e) != 0 ? 1 : 0; }      // (read per call: tests compare)
    LaunchPartialReg(hclg_dev_, pw, n, qc);
  } else {
    AllocSearch(&sp, arena, qc);
    LaunchSearch(&sp, gd, p->ll, p->ld_ll, qc);
  }
  { const hipError_t le = hipGetLastError(); if (le != hipSuccess) Fail(std::string("a kernel launch failed: ") + hipGetErrorString(le)); }
  res->utts.assign(n, UttResult());
  for (int i = 0; i < n; i++) res->utts[i].num_frames = T[i];
  CollectResults(sp, cx, par, gd, T.data(), p->ll, p->ld_ll, 1, 1.0f, qc, res->utts.data(), res->timings);
  for (int i = 0; i < n; i++) {
    UttResult &ur = res->utts[i];
    if (T[i] == 0) {                 // nothing searched yet: an empty best path (the reference asserts; its callers guard)
      ur.status = RS_OK;
      ur.error.clear();
      ur.hyps.assign(1, Hypothesis());
      for (int64_t &c : ur.counters) c = 0;
      continue;
    }
    if (!p->reg) {                   // (the deferred search's traceback walks every frame)
      for (int k = 1; k < 7; k++) ur.counters[k] = 0;
      ur.counters[0] = T[i] + 1;
    }
    if (ur.status != RS_OK && (ur.counters[7] & 8)) ur.error = "partial result: a back-pointer chain missed the stream's traceback anchor";
  }
}


// ---------------------------------------------------------------------------------------------------------- endpointing
// "The arc's transition-id belongs to a silence phone", one bit per HCLG arc (the device arcs carry pdf ids, so TransitionIdToPhone
// is applied here, once per model and phone list).  Callers hold pool_mu_ and wait for their kernel before they return, so nothing
// reads the bitmap while a changed list rewrites it.
const unsigned *Model::SilenceArcBitmap(const std::vector<int32_t> &sil_phones, hipStream_t s) {
  if (d_sil_bitmap_ && sil_phones == sil_bitmap_phones_) return d_sil_bitmap_;
  const size_t A = hclg_.arcs.size(), words = A / 32 + 1;
  h_sil_bitmap_.assign(words, 0u);
  const std::vector<int32_t> &id2phone = am_.trans.id2phone;
  for (size_t a = 0; a < A; a++) {
    const int tid = hclg_.arcs[a].ilabel;
    if (tid <= 0 || tid >= (int)id2phone.size()) continue;
    if (std::binary_search(sil_phones.begin(), sil_phones.end(), id2phone[tid])) h_sil_bitmap_[a >> 5] |= 1u << (a & 31);
  }
  if (!d_sil_bitmap_) {
    void *d = nullptr;
    RS_HIP(hipMalloc(&d, words * 4));
    owned_.push_back(d);
    d_sil_bitmap_ = static_cast<unsigned *>(d);
  }
  RS_HIP(hipMemcpyAsync(d_sil_bitmap_, h_sil_bitmap_.data(), words * 4, hipMemcpyHostToDevice, s));
  RS_HIP(hipStreamSynchronize(s));      // (h_sil_bitmap_ is pageable and reused)
  sil_bitmap_phones_ = sil_phones;
  return d_sil_bitmap_;
}

// rs_streams_endpoint: the catch-up of a partial (every completed tick, batched), then per stream FinalRelativeCost() and
// TrailingSilenceLength() (online-endpoint.cc:109-126):
//   * register-resident streams: EndpointRegKernel (decode_endpoint.hip) over the parked frontier and the back-pointer rows of the
//     trailing silence;
//   * streams whose search is deferred to finish: the token-list search over the log-likelihood rows so far in a scratch arena, then
//     EndpointTokensKernel over its last token list and back pointers.  O(frames so far) per call.
// The rules are evaluated on the host (EndpointRuleFired) by the caller.  Nothing an advance, a partial or a finish reads is written.
// A stream whose search has failed (what a partial reports as that utterance's RS_ERR_DECODE) has no answer: *search_error names the
// first such stream with the partial's message, its record says "nothing detected", and the streams stay usable as after a partial.
void Model::StreamsEndpoint(rs_stream *const *streams, int n, const std::vector<int32_t> &sil_phones, rs_endpoint_status *out, std::string *search_error) {
  std::lock_guard<std::mutex> lk(pool_mu_);
  try {
    StreamsEndpointLocked(streams, n, sil_phones, out, search_error);
  } catch (const DeviceError &) {
    StreamsPoisonAll();
    throw;
  } catch (...) {
    if (pool_) { pool_->issuer.Drain(false); (void)hipStreamSynchronize(pool_->qa); (void)hipStreamSynchronize(pool_->qi); (void)hipStreamSynchronize(pool_->q); (void)hipStreamSynchronize(pool_->qc); }
    throw;
  }
}

void Model::StreamsEndpointLocked(rs_stream *const *streams, int n, const std::vector<int32_t> &sil_phones, rs_endpoint_status *out, std::string *search_error) {
  StreamPool *p = Pool();
  RS_HIP(hipSetDevice(opts_.device_id));
  bool more = false;
  for (int i = 0; i < n; i++) more = more || streams[i]->n_samples / kTickSamples > streams[i]->sched.ticks_done;
  if (more) StreamsAdvanceLocked(streams, n, /*final=*/false, 1, 1.0f, nullptr, /*every_tick=*/true);
  StreamsDrain(p, nullptr);        // every advance has finished: the arena sets are free, the frontier and rows are in place
  const int fsf = opts_.frame_subsampling_factor;
  std::vector<int> T(n);
  int maxT = 0;
  for (int i = 0; i < n; i++) {
    const rs_stream &st = *streams[i];
    T[i] = (p->reg && !st.dec_started) ? 0 : (st.ll_done + fsf - 1) / fsf;      // NumFramesDecoded()
    maxT = std::max(maxT, T[i]);
  }
  DecodeContext &cx = *static_cast<DecodeContext *>(p->cx);
  const int par = (int)(p->n_adv % StreamPool::kDepth);
  DeviceArena &arena = cx.arena[par];
  HostArena &harena = cx.host_arena[par];
  hipStream_t qc = p->qc;
  SearchPlan sp;
  if (!p->reg) {
    SearchRequest rq = SearchRequestFor(n, maxT, 1, 1.0f);
    rq.best_path_only = rq.token_lists = true;
    PlanSearch(rq, &sp);
  }
  arena.Reset(qc);
  harena.Reset(qc);
  EndpointWork ew;
  std::memset(&ew, 0, sizeof(ew));
  ew.sil_arc = SilenceArcBitmap(sil_phones, qc);
  int *d_idx = arena.AllocT<int>((size_t)3 * n + 16);
  {
    int *h = harena.AllocT<int>((size_t)3 * n + 16);
    for (int i = 0; i < n; i++) { h[i] = T[i]; h[n + i] = streams[i]->slot; h[2 * n + i] = streams[i]->row0; }
    RS_HIP(hipMemcpyAsync(d_idx, h, sizeof(int) * 3 * n, hipMemcpyHostToDevice, qc));
  }
  ew.num_frames = d_idx;
  ew.out = arena.AllocT<int4>(n);
  if (p->reg) {
    ew.state_cost = p->dec_state; ew.bp = p->bp; ew.slot = d_idx + n; ew.pool_row = d_idx + 2 * n;
    LaunchEndpointReg(hclg_dev_, ew, n, qc);
  } else {
    BatchGeom gd;
    gd.n_utts = n; gd.max_frames = maxT; gd.d_num_frames = d_idx; gd.d_row_base = d_idx + 2 * n;
    // (the search also adds final costs and traces its best path back into out_words / out_costs, which nobody reads here:
    // EndpointTokensKernel needs the best token without final costs and the first non-silence arc, so it reduces the last token list
    // and walks the back pointers itself.  The extra traceback is one walk of the path, small beside the search over all frames.)
    AllocSearch(&sp, arena, qc);
    LaunchSearch(&sp, gd, p->ll, p->ld_ll, qc);
    ew.tokens = sp.w.tokens; ew.frame_tok_off = sp.w.frame_tok_off; ew.counters = sp.w.counters;
    ew.tok_cap = sp.w.tok_cap; ew.max_frames = maxT;
    LaunchEndpointTokens(hclg_dev_, ew, n, qc);
  }
  { const hipError_t le = hipGetLastError(); if (le != hipSuccess) Fail(std::string("a kernel launch failed: ") + hipGetErrorString(le)); }
  int4 *h_out = harena.AllocT<int4>(n);
  RS_HIP(hipMemcpyAsync(h_out, ew.out, sizeof(int4) * n, hipMemcpyDeviceToHost, qc));
  RS_HIP(hipStreamSynchronize(qc));
  const float shift = EndpointFrameShift();
  for (int i = 0; i < n; i++) {
    rs_endpoint_status &o = out[i];
    const int fl = h_out[i].z;
    if (fl & 8) Fail("endpoint query: a back-pointer chain of the best token is broken");
    if ((fl & 2) && search_error && search_error->empty()) {      // the messages of a partial (CollectResults)
      const int sf = fl >> 4;
      *search_error = "stream " + std::to_string(i) + ": " +
                      (sf & 1 ? "decoder token capacity exceeded (raise rs_decode_opts.max_tokens_per_frame)"
                              : sf & 4 ? "epsilon cycle in the decoding graph" : "no surviving tokens (search error)");
    }
    o.detected = 0;
    o.num_frames_decoded = T[i];
    o.trailing_silence_frames = h_out[i].x;
    std::memcpy(&o.final_relative_cost, &h_out[i].w, 4);
    o.frame_shift_seconds = shift;
    o.rows_read = T[i] == 0 ? 0 : (p->reg ? h_out[i].y : T[i] + 1);      // (the deferred search itself reads every frame)
  }
}

// rs_streams_finalize: see StreamsAdvanceLocked(no_flush)
void Model::StreamsFinalize(rs_stream *const *streams, int n, int nbest, float lat_scale, Result *res) {
  std::lock_guard<std::mutex> lk(pool_mu_);
  try {
    StreamsAdvanceLocked(streams, n, /*final=*/true, nbest, lat_scale, res, /*every_tick=*/true, /*no_flush=*/true);
  } catch (const DeviceError &) {
    StreamsPoisonAll();
    throw;
  } catch (...) {
    if (pool_) { pool_->issuer.Drain(false); (void)hipStreamSynchronize(pool_->qa); (void)hipStreamSynchronize(pool_->qi); (void)hipStreamSynchronize(pool_->q); (void)hipStreamSynchronize(pool_->qc); }
    throw;
  }
}

// ---------------------------------------------------------------------------------------------------------- speaker adaptation
// rs_streams_adaptation: the reference's GetAdaptationState / GetCmvnState (online2-wav-nnet3-latgen-faster.cc:287-288) of streams
// that have ended, in one launch over the listed streams (adapt_kernels.hip) and one copy to the host.  The streams still hold
// their slots and rows (StreamEnd); everything that wrote them has been waited for by the call that ended them.
void Model::StreamsAdaptation(rs_stream *const *streams, int n, rs_adaptation **out) {
  std::lock_guard<std::mutex> lk(pool_mu_);
  try {
    StreamPool *p = Pool();
    RS_HIP(hipSetDevice(opts_.device_id));
    const bool has_iv = fc_.ie.present, has_nn = fc_.use_cmvn;
    const int C = fc_.mfcc.nceps, C1 = C + 1, Di = has_iv ? fc_.ie.ivector_dim() : 0, usz = Di * (Di + 1) / 2;
    const size_t stride = (has_iv ? (size_t)Di + usz + 1 + 2 * C1 : 0) + (has_nn ? 2 * (size_t)C1 : 0);
    if (stride == 0) {      // no extractor, no nnet-input CMVN: the state is empty
      for (int i = 0; i < n; i++) AdaptationFresh(out[i]);
      return;
    }
    StreamsDrain(p, nullptr);      // the arena sets are free (advances of other streams may have been in flight)
    DecodeContext &cx = *static_cast<DecodeContext *>(p->cx);
    const int par = (int)(p->n_adv % StreamPool::kDepth);
    DeviceArena &arena = cx.arena[par];
    HostArena &harena = cx.host_arena[par];
    hipStream_t qc = p->qc;
    arena.Reset(qc);
    harena.Reset(qc);
    int *d_idx = arena.AllocT<int>((size_t)3 * n + 16);
    double *d_car = arena.AllocT<double>((size_t)n * 4 * C1 + 8), *d_out = arena.AllocT<double>((size_t)n * stride + 8);
    {
      int *h = harena.AllocT<int>((size_t)3 * n + 16);
      double *hc = harena.AllocT<double>((size_t)n * 4 * C1 + 8);
      for (int i = 0; i < n; i++) {
        const rs_stream &st = *streams[i];
        h[i] = st.row0; h[n + i] = st.adapt_frames; h[2 * n + i] = st.slot;
        if (st.spk0.empty()) std::memset(hc + (size_t)i * 4 * C1, 0, 8 * 4 * (size_t)C1);
        else std::memcpy(hc + (size_t)i * 4 * C1, st.spk0.data(), 8 * 4 * (size_t)C1);
      }
      RS_HIP(hipMemcpyAsync(d_idx, h, sizeof(int) * 3 * n, hipMemcpyHostToDevice, qc));
      RS_HIP(hipMemcpyAsync(d_car, hc, 8 * (size_t)n * 4 * C1, hipMemcpyHostToDevice, qc));
    }
    AdaptWork w;
    std::memset(&w, 0, sizeof(w));
    w.n_streams = n; w.dim = C; w.ld = p->ld_c; w.ivec_dim = Di; w.has_iv = has_iv ? 1 : 0; w.has_nn = has_nn ? 1 : 0;
    w.raw = p->raw; w.row0 = d_idx; w.frames = d_idx + n; w.slot = d_idx + 2 * n;
    w.carried = d_car; w.lin = p->lin; w.quad = p->quad; w.numf = p->numf;
    // LimitFrames(max_remembered_frames, posterior_scale): the iVector statistics' target count is the FLOAT product, as there
    w.max_remembered = (double)fc_.ie.max_remembered_frames;
    w.max_remembered_scaled = (double)(float)(fc_.ie.max_remembered_frames * fc_.ie.posterior_scale);
    w.max_count = (double)fc_.ie.max_count; w.prior_offset = fc_.ie.prior_offset;
    w.out = d_out; w.out_stride = (long)stride;
    LaunchAdaptGet(w, qc);
    { const hipError_t le = hipGetLastError(); if (le != hipSuccess) Fail(std::string("a kernel launch failed: ") + hipGetErrorString(le)); }
    double *h_out = harena.AllocT<double>((size_t)n * stride + 8);
    RS_HIP(hipMemcpyAsync(h_out, d_out, 8 * (size_t)n * stride, hipMemcpyDeviceToHost, qc));
    RS_HIP(hipStreamSynchronize(qc));
    for (int i = 0; i < n; i++) {
      rs_adaptation &a = *out[i];
      AdaptationFresh(&a);
      const double *o = h_out + (size_t)i * stride;
      if (has_iv) {
        std::memcpy(a.lin.data(), o, 8 * (size_t)Di);
        std::memcpy(a.quad.data(), o + Di, 8 * (size_t)usz);
        a.num_frames = o[Di + usz];
        std::memcpy(a.cmvn_iv.data(), o + Di + usz + 1, 8 * 2 * (size_t)C1);
        o += (size_t)Di + usz + 1 + 2 * C1;
      }
      if (has_nn) std::memcpy(a.cmvn_nn.data(), o, 8 * 2 * (size_t)C1);
    }
  } catch (const DeviceError &) {
    StreamsPoisonAll();
    throw;
  }
}

}  // namespace rs

// Host orchestration of the batched transcribe pipeline on one MI355X (one process per GPU).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <condition_variable>
#include <atomic>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rhasspy_speech_hip.h"
#include "arena.h"
#include "call_plan.h"
#include "kernels.h"
#include "lattice.h"
#include "model.h"

namespace rs {

struct DeviceError : Error {
  explicit DeviceError(const std::string &m) : Error(m) {}
};
void HipCheck(hipError_t e, const char *what, const char *file, int line);
#define RS_HIP(x) ::rs::HipCheck((x), #x, __FILE__, __LINE__)

// The two arenas of a decode call (arena.h: blocks appended on demand, coalesced into one by the Reset that follows, so that a warm
// call allocates nothing; the first call of a further decode context of a model is told the rounds its siblings have completed --
// Model::round_mark_ -- and starts with that one block).  Device memory: every block zero-filled when it is allocated, and its last 1 MiB never handed out -- some
// kernels read a little past the end of their last buffer (the + 256 / + 8 / + 64 at the allocation sites), which has to stay in
// mapped memory.  Page-locked host staging: the small H2D / D2H transfers of a call are truly asynchronous from it and never wait on
// a pageable-memory bounce buffer.
struct DeviceBlocks {
  static constexpr size_t kAlign = 256, kTail = (size_t)1 << 20;
  using Stream = hipStream_t;
  void *Allocate(size_t bytes, hipStream_t s);      // filled before it returns: the block may be used on any stream
  void Free(void *p) { (void)hipFree(p); }
  void Synchronize(hipStream_t s);
};
struct PinnedBlocks {
  static constexpr size_t kAlign = 64, kTail = 0;
  using Stream = hipStream_t;
  void *Allocate(size_t bytes, hipStream_t s);
  void Free(void *p) { (void)hipHostFree(p); }
  void Synchronize(hipStream_t s);
};
using DeviceArena = Arena<DeviceBlocks>;
using HostArena = Arena<PinnedBlocks>;

struct Hypothesis {
  std::vector<int32_t> words;
  float graph_cost = 0, acoustic_cost = 0;
  // emit_alignment only: the transition-id of every decoder frame, and its phone segments (SplitAlignment)
  std::vector<int32_t> tids, phones, phone_start, phone_len;
  bool phones_ok = false;
};
struct UttResult {
  int status = RS_OK;
  std::string error;
  int num_frames = 0;
  std::vector<Hypothesis> hyps;
  int64_t counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<float> feats, ivector, loglikes;   // keep_intermediates only
  // keep_intermediates, batch calls: per convolution op, in op order, its output buffer's rows of the real frames (T x dim, the
  // fused stages applied; under --frame-subsampling-factor only the rows the op was evaluated on hold anything)
  std::vector<std::vector<float>> conv_out;
  std::vector<int> conv_dim;
  // ... per recurrent block of any kind, in op order, the rows the layers above read (LSTM: rp, or m without a projection; OPGRU and
  // PGRU: y, before any BatchNorm; fast-gru-layer: c: T x dim)
  std::vector<std::vector<float>> lstm_out;
  std::vector<int> lstm_dim;
  // the same per attention op: the RestrictedAttentionComponent's output rows (T x heads * (value-dim [+ context positions])), before
  // the ReLU / BatchNorm / Normalize nodes behind it
  std::vector<std::vector<float>> attention_out;
  std::vector<int> attention_dim;
  int feat_dim = 0, ivec_rows = 0, ivec_dim = 0, num_pdfs = 0;
  std::shared_ptr<CompactLat> clat;              // emit_lattice only
};
struct Result {
  enum { kNoAlignment = 0, kAlignment = 1, kPartialResult = 2 };
  int alignment = kNoAlignment;      // whether the hypotheses carry alignments; if not, why
  std::vector<UttResult> utts;
  float timings[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// Device-resident, immutable part of a model.
struct GemmPlan {        // one LayerOp of kind kGemm, uploaded
  const LayerOp *op = nullptr;
  float *d_W = nullptr, *d_bias = nullptr;
  void *d_W3 = nullptr;           // split-fp16 image of W for GemmKernelB3 (layers at least 192 columns wide)
  void *d_W3I = nullptr;          // the same for GemmKernelB3I (every source a frame buffer on a k-step boundary)
  float *d_w3_inv_scale = nullptr;   // inverse of the images' column scales (n3 floats)
  bool res_by_image = false;      // LayerOp::res_buf is read through its operand image (GemmDev::res_img) when the call runs on the image-fed kernels
  int k_pad = 0, n_pad = 0, n3 = 0;
  bool interleave = false;        // W3 k-steps alternate between the segments (see GemmKernelB3)
  std::vector<int> seg_k0;
  std::vector<std::pair<float *, float *>> d_stage;   // scale/offset vectors per stage
};

struct ConvOperands {     // one LayerOp of kind kConv (W in the kernel's order, the k -> LDS offset table) or kGather (part, column per output column)
  float *wt = nullptr;
  int *tab0 = nullptr, *tab1 = nullptr;
};

struct LstmOperands {     // one LayerOp of kind kLstm or kLstmp: LstmWeightImages' two matrices, the projection's bias, the nonlinearity's <Params>
  float *wr_t = nullptr, *wrp_t = nullptr, *b_rp = nullptr, *params = nullptr;
};
struct LstmbOperands {    // one LayerOp of kind kLstmb: LstmbWeightImages' two matrices, the scale / offset vectors, the nonlinearity's <Params>
  float *wam_t = nullptr, *wb_t = nullptr, *so_scale = nullptr, *so_offset = nullptr, *params = nullptr;
};
struct GruOperands {      // one LayerOp of kind kGru: GruWeightImages' two matrices, W_y's bias, the nonlinearity's <w_h>
  float *ws_t = nullptr, *wy_t = nullptr, *b_y = nullptr, *w_h = nullptr;
};
struct PgruOperands {     // one LayerOp of kind kPgru: PgruWeightImages' three matrices, W_y's bias (the last two null without a projection)
  float *wr_t = nullptr, *wzh_t = nullptr, *wy_t = nullptr, *b_y = nullptr;
};
// The utterances of the call a recurrent block is walked for (RunNnet): frames and first row of each, in the layout of kernels.h;
// for a stream advance also the frames each stream had before it and its slot, and the pool's parked state per kLstm op
struct LstmCall {
  int n_utts = 0;
  const int *num_frames = nullptr, *row_base = nullptr;
  const int *t0 = nullptr, *slot = nullptr;
  const std::vector<float *> *rings = nullptr;      // indexed like am_.nnet.ops (kLstm and kGru ops)
};

struct LatArcBuffer { void *d = nullptr; size_t cap = 0; };      // capacity in LatArc records

// HIP events around the stages of a call, on the stream the kernels are launched on
struct Timer {
  hipEvent_t ev[8];
  int n = 0;
  hipStream_t s;
  explicit Timer(hipStream_t st) : s(st) { for (auto &e : ev) (void)hipEventCreate(&e); }
  ~Timer() { for (auto &e : ev) (void)hipEventDestroy(e); }
  void Mark() { if (n < 8) (void)hipEventRecord(ev[n++], s); }
  void Reset() { n = 0; }
  float Ms(int a, int b) { float ms = 0; if (a < n && b < n) (void)hipEventElapsedTime(&ms, ev[a], ev[b]); return ms; }
};

struct StreamPool;                                                 // stream.cc
struct AdvanceSet;
struct BatchCall;                                                  // engine.cc
struct StagesBC;
void GemmRecordJoin(uint64_t gen);                               // engine.cc: the generation of recorded launches this thread enqueues for
uint64_t GemmRecordJoined();
void SampleGemmMode(bool exact, int *ovf_dev);                   // engine.cc: which layer GEMMs this thread's launches use, and whose range flag they raise
struct StreamPoolDeleter { void operator()(StreamPool *p) const; };

// Row lists of a batch for the layers that need fewer rows than the full halo: entry (lext, rext) lists, utterance after
// utterance, the physical rows of t in [-lext, T + rext) (kernels.h row layout).  (0, 0) = the real frames only.
struct RowMaps {
  // span128: the physical rows any 128 consecutive rows of the list reach over (GemmDev::row_map_span128), 0 = not known
  // stride: the list holds the rows t = 0 mod stride of [-lext, T + rext) (BufferInfo::stride)
  struct Entry { int lext, rext; const int *rows; int count; int span128 = 0; int stride = 1; int span160 = 0; };
  std::vector<Entry> maps;
  const Entry *Find(int lext, int rext, int stride = 1) const {
    for (auto &e : maps) if (e.lext == lext && e.rext == rext && e.stride == stride) return &e;
    return nullptr;
  }
};

// What a call's search runs (search_plan.h: PlanSearchCall) and its work buffers (engine.cc: PlanSearch / AllocSearch / LaunchSearch /
// CollectResults).
struct SearchPlan {
  SearchCall call{};
  bool unscale = false, want_lattice = false;      // (call.unscale, call.want_lattice)
  bool want_alignment = false;       // rs_decode_opts.emit_alignment, set by the calls whose results carry alignments (not the partials)
  int S = 0, tok_cap = 0, max_words = 1024, maxT = 0, n_utts = 0;
  DecodeOptsDev dopts{};
  DecodeWork w{};
  DenseWork dw{};
};

// Endpointing on the host (online2/online-endpoint.{h,cc}): the defaults, and EndpointDetected's five rules in float
void DefaultEndpointOpts(rs_endpoint_opts *o);
int EndpointRuleFired(const rs_endpoint_opts &o, int num_frames_decoded, int trailing_silence_frames, float frame_shift, float final_relative_cost);

class Model {
 public:
  Model(const std::string &final_mdl, const std::string &hclg, const std::string &online_conf, const rs_decode_opts &opts);
  ~Model();
  void ToDevice();
  // The online iVector estimator over K chunks of n streams / utterances in four launches (ivector_kernels.hip: IvecChainKernel);
  // d_fb / d_fe / d_or / d_ac: [K][n] frame ranges, iVector rows, "has new frames"; state rows slot[u] (null: u) of lin / quad / numf / x
  void IvecChunkChain(DeviceArena &arena, const BatchGeom &g, int n, int K, const float *stats_feats, int ld_l, const int *post_idx, const float *post_w,
                      const int *d_fb, const int *d_fe, const int *d_or, const int *d_ac, double *lin, double *quad, double *numf, double *x, const int *slot,
                      float *ivec_out, int ld_i, hipStream_t s) const;
  void ResolveDecoderOptions();      // opts_ := command line (rs_decode_opts) over online.conf over the reference's defaults
  std::string Describe() const;
  // streaming = true reproduces online2-cli-nnet3-decode-faster: 1024-sample ticks, one iVector per nnet chunk
  // estimated from the frames available at the tick the chunk is computed on (warm-started CG).
  std::unique_ptr<Result> DecodeBatchDevice(const int16_t *d_pcm, const int64_t *sample_offsets, int n_utts, int nbest,
                                            float lat_scale, hipStream_t stream, bool streaming = false);
  std::unique_ptr<Result> DecodeBatchHost(const int16_t *const *pcm, const int32_t *n_samples, int n_utts, int nbest,
                                          float lat_scale, bool streaming = false);
  const rs_decode_opts &opts() const { return opts_; }
  // rs_decode_opts.exact_token_order, RS_EXACT_ORDER overriding (read per call: tests compare the two searches on one model)
  bool ExactOrder() const { return ExactOrderAsked(ReadSearchSwitches(), opts_.exact_token_order); }
  const FeatureConfig &features() const { return fc_; }
  const AcousticModel &am() const { return am_; }
  const Hclg &hclg() const { return hclg_; }
  // Streams (stream.cc): a stream owns a slot and a row range of the model's pool from open to close; advance runs the
  // device work the accepted audio makes possible, batched over the given streams; final = end of input, results to res.
  void StreamOpen(rs_stream *st, const rs_adaptation *state = nullptr);      // state: checked by the caller (AdaptationMismatch)
  void StreamClose(rs_stream *st);
  // Speaker adaptation (stream.cc): a stream that ended through a finish / finalize keeps its slot and rows until it is freed (or the
  // pool needs them), so that StreamsAdaptation can take what OnlineIvectorFeature::GetAdaptationState / GetCmvnState return
  void StreamEnd(rs_stream *st, bool flushed);
  void StreamsAdaptation(rs_stream *const *streams, int n, rs_adaptation **out);      // out[i]: allocated by the caller
  void AdaptationFresh(rs_adaptation *a) const;                                        // what the reference constructs per speaker
  std::string AdaptationMismatch(const rs_adaptation &a) const;                         // "" = the state fits this model
  void StreamsAdvance(rs_stream *const *streams, int n, bool final, int nbest, float lat_scale, Result *res);
  void StreamsAdvanceLocked(rs_stream *const *streams, int n, bool final, int nbest, float lat_scale, Result *res,
                            bool every_tick = false, bool no_flush = false);      // pool_mu_ held; every_tick: no min_ticks coalescing; no_flush (with final): rs_streams_finalize
  // rs_streams_partial: the advance the accepted samples allow (every tick), then the best path over the frames searched so far
  // without final costs, one hypothesis per stream in `res`; the streams stay open
  void StreamsPartial(rs_stream *const *streams, int n, Result *res);
  // rs_streams_endpoint: the same catch-up, then per stream {trailing silence frames, rows read, flags, final relative cost} from the
  // frontier and the back pointers (decode_endpoint.hip); sil_phones: sorted, unique, not empty.  The streams stay open.
  void StreamsEndpoint(rs_stream *const *streams, int n, const std::vector<int32_t> &sil_phones, rs_endpoint_status *out, std::string *search_error);
  // rs_streams_finalize: the catch-up, then the end of a stream WITHOUT the flush of the feature tail (FinalizeDecoding without
  // InputFinished): results over the decoder frames searched
  void StreamsFinalize(rs_stream *const *streams, int n, int nbest, float lat_scale, Result *res);
  void EndpointOpts(rs_endpoint_opts *o) const;      // defaults <- online.conf's --endpoint.* lines; throws on a value that does not parse
  float EndpointFrameShift() const { return fc_.mfcc.opts.frame_shift_ms / 1000.0f * (float)opts_.frame_subsampling_factor; }      // online-nnet3-decoding.cc:90-92
  void StreamsPoisonAll(const std::string &why = std::string());          // pool_mu_ held

 private:
  struct DecodeContext;
  void DecodeGroup(DecodeContext &cx, int gi, const int16_t *d_pcm, const int64_t *sample_offsets, int n_utts, int nbest, float lat_scale,
                   hipStream_t s, bool streaming, UttResult *out_utts, float *timings);
  // DecodeGroup's stages (engine.cc)
  void BatchFrames(const int64_t *sample_offsets, BatchCall *b) const;
  void BatchSetupUpload(const int64_t *sample_offsets, BatchCall *b);
  void BatchFeatures(const int16_t *d_pcm, BatchCall *b);
  void BatchIvectors(BatchCall *b);
  void BatchDecoderRows(BatchCall *b, float **ll, int *ll_ld, BatchGeom *gdec);
  void BatchIntermediates(const BatchCall &b, const float *ll, int ll_ld, UttResult *out_utts) const;
  template <typename T> T *Upload(const std::vector<T> &v);
  void *UploadBytes(const void *p, size_t bytes);
  void BuildGemmPlan(const LayerOp &op, GemmPlan *plan);
  // imgs (may be null): operand images of the frame buffers (kernels.h: ActImage), indexed like src; out_buf = index of the
  // buffer `out` belongs to (-1: none of them)
  GemmDev MakeGemm(const GemmPlan &pl, const std::vector<float *> &src, const std::vector<int> &src_ld, float *ivec, int ivec_ld, float *out, int ldo,
                   int share, const std::vector<ActImage> *imgs = nullptr, int out_buf = -1) const;
  // operand images for the buffers the split-bf16 GEMM reads as images, from a call's arena
  std::vector<ActImage> AllocImages(DeviceArena &arena, int rows) const;
  std::vector<char> buf_image_, buf_f32_;      // per nnet buffer: has an operand image / is (also) read as plain floats
  // the request of a call with this model's options; PlanSearch: the choice for it (search_plan.h), failing where the plan refuses
  SearchRequest SearchRequestFor(int n_utts, int maxT, int nbest, float lat_scale) const;
  void PlanSearch(const SearchRequest &rq, SearchPlan *sp) const;
  void AllocSearch(SearchPlan *sp, DeviceArena &arena, hipStream_t s) const;
  void LaunchSearch(SearchPlan *sp, const BatchGeom &g, const float *ll, int ll_ld, hipStream_t s) const;
  void CollectResults(SearchPlan &sp, DecodeContext &cx, int gi, const BatchGeom &g, const int *T, const float *ll, int ll_ld, int nbest,
                      float lat_scale, hipStream_t s, UttResult *out_utts, float *timings);
  void RunNnet(const std::vector<float *> &bufp, const std::vector<int> &buf_ld, float *d_ivec, int ld_i, const int *d_row_ivec, int rows,
               const RowMaps &row_maps, int share, size_t op_begin, size_t op_end, hipStream_t s,
               const std::vector<ActImage> *imgs = nullptr, const LstmCall *lstm = nullptr) const;

  // keep_intermediates only: the layer GEMMs the most recent decode call or stream advance launched, one line per distinct launch
  // (Describe: "gemm_launch:").  A call opens a generation (GemmRecordBegin) and every thread that enqueues for it carries the
  // number (GemmRecordJoin, thread-local like the GEMM mode): what the pool's issuing thread still launches for an older advance
  // is dropped.  With the option at 0 LaunchGemmRecorded is LaunchGemm and the list stays empty.
  uint64_t GemmRecordBegin() const;
  void LaunchGemmRecorded(const std::string &name, const GemmDev &d, int rows, const int *row_ivec, hipStream_t s, const GemmSwitches *sw = nullptr) const;
  mutable std::mutex gemm_rec_mu_;
  mutable uint64_t gemm_rec_gen_ = 0;
  mutable std::vector<std::string> gemm_rec_;

  rs_decode_opts opts_;
  FeatureConfig fc_;
  AcousticModel am_;
  Hclg hclg_;
  std::vector<int32_t> arc_ilabel_;   // original transition-ids (device arcs carry pdf+1)

  bool on_device_ = false;
  std::mutex mu_;                      // ToDevice
  std::vector<void *> owned_;         // persistent device allocations
  int max_groups_ = 1;                 // RS_SUBBATCHES=2: two concurrent utterance groups inside one call
  // Everything one decode call needs for itself.  A model owns a few of them so that calls from different host threads can
  // be in flight together: the search of one batch is latency-bound and leaves the device to the next batch's GEMMs.
  struct DecodeContext {
    hipStream_t stream = nullptr, stream2 = nullptr;
    hipStream_t stream_dec = nullptr;      // the search of a time slab runs here while the next slab's output layer runs on `stream`
    hipEvent_t slab_ev[9] = {};
    hipEvent_t stage_ev[3] = {};           // end of this call's feature + iVector stage / of its acoustic-model stage / of its sample upload (StageChain)
    int *gemm_ovf = nullptr, *gemm_ovf_dev = nullptr;      // pinned + mapped word and the device's address of it (see exact_gemm_)
    hipEvent_t split_ev = nullptr;         // what `stream` held when a call split into two utterance groups (the second group's stream waits for it)
#ifndef RS_CONTEXT_SETS
#define RS_CONTEXT_SETS 4
#endif
    static constexpr int kSets = RS_CONTEXT_SETS;
    DeviceArena arena[kSets];              // one per concurrent utterance group (batch calls use two; stream advances rotate over all)
    HostArena host_arena[kSets];
    LatArcBuffer lat_arcs[kSets];          // lattice arc output of LatticeKernel, grow-only, one per utterance group
    int16_t *h_pcm_pinned = nullptr;       // pinned staging for host-buffer batches
    size_t h_pcm_cap = 0;
    int16_t *d_pcm = nullptr;
    int active_groups = 1;
    uint64_t gemm_rec_gen = 0;             // the call's generation of recorded layer GEMM launches (its group threads join it)
    bool force_exact = false;              // this call is the repetition of one that left the split-fp16 kernels' range
    bool busy = false;
  };
  std::vector<std::unique_ptr<DecodeContext>> ctx_;
  std::mutex ctx_mu_;
  // The largest round any context's arena of a set has completed, [0] device, [1] host.  The contexts of a model serve the same
  // traffic: a context publishes its rounds when its call ends (PublishRounds, before ReleaseContext -- not at its next Reset, which
  // in a burst of first calls comes after the siblings have started), and the Resets of a batch call pass the mark on, so that a
  // context's first call makes one allocation per arena instead of a spill and a coalescing call in the middle of the others' work.
  // (atomic: written and read by calls on different threads, like the counters Describe reads)
  RoundMark round_mark_[2][DecodeContext::kSets];
  void PublishRounds(const DecodeContext &cx);
  // Calls in flight on one model pass through the feature + iVector stage and through the acoustic-model stage ONE AFTER THE
  // OTHER (each stage's kernels fill the device; two calls in the same stage only slow each other down), so calls that arrive
  // at the same moment come out staggered -- the first after one call's latency, not all of them after four -- and the pipeline
  // of stages is full from the second call on.  Device-side only: the next call's stream waits for the event the previous
  // call recorded behind its stage; the host holds the stage's mutex just while it enqueues.  RS_STAGE_CHAIN=0 switches it off.
  std::mutex stage_mu_[3];
  hipEvent_t stage_tail_[3] = {nullptr, nullptr, nullptr};      // [2]: the copies of a call's samples to the device (DecodeBatchHost)
  std::condition_variable ctx_cv_;
  DecodeContext *AcquireContext();
  void ReleaseContext(DecodeContext *cx);
  bool OthersInFlight();
  std::unique_ptr<Result> DecodeInContext(DecodeContext &cx, const int16_t *d_pcm, const int64_t *sample_offsets, int n_utts, int nbest,
                                          float lat_scale, hipStream_t user_stream, bool streaming);
  friend struct StreamPool;
  std::unique_ptr<StreamPool, StreamPoolDeleter> pool_;
  std::unique_ptr<DecodeContext> stream_ctx_;
  mutable std::mutex pool_mu_;     // pool bookkeeping and advances of this model, one at a time
  StreamPool *Pool();
  void StreamsDrain(StreamPool *p, float *extra);
  void IssuerSync(StreamPool *p);     // everything handed to the pool's issuing thread has been queued; ITS failure poisons the open streams, then rethrows
  void StreamGrow(rs_stream *st, int need_frames);
  // One advance, stage by stage (stream.cc: StreamsAdvanceLocked is their outline)
  PlanConfig PlanCfg() const;         // the integers call_plan.h plans with
  int AdvanceTakeSet(StreamPool *p, bool final);
  void AdvancePlanStreams(StreamPool *p, rs_stream *const *streams, int n, bool flush, bool final, AdvancePlan *plan);
  void AdvanceUpload(StreamPool *p, rs_stream *const *streams, const AdvancePlan &plan, bool final, AdvanceSet *set);
  void AdvanceStageA(StreamPool *p, const AdvancePlan &plan, const AdvanceSet &set);
  void AdvanceIvectors(StreamPool *p, const AdvancePlan &plan, const AdvanceSet &set);
  void AdvanceStagesBC(StreamPool *p, const AdvancePlan &plan, const AdvanceSet &set, bool final, SearchPlan *sp);
  void IssueStagesBC(const StagesBC &j);      // on the caller's thread (a finishing call) or the pool's issuing thread
  void AdvanceBookkeeping(StreamPool *p, rs_stream *const *streams, const AdvancePlan &plan, int par, bool searched);
  void AdvanceFinish(StreamPool *p, rs_stream *const *streams, const AdvancePlan &plan, const AdvanceSet &set, SearchPlan &sp, bool flush, int nbest,
                     float lat_scale, std::chrono::steady_clock::time_point wall0, Result *res);
  void StreamsPartialLocked(rs_stream *const *streams, int n, Result *res);      // pool_mu_ held
  void StreamsEndpointLocked(rs_stream *const *streams, int n, const std::vector<int32_t> &sil_phones, rs_endpoint_status *out, std::string *search_error);      // pool_mu_ held
  // "the arc's transition-id belongs to a silence phone", one bit per HCLG arc, on the device; rebuilt when the phone list changes
  const unsigned *SilenceArcBitmap(const std::vector<int32_t> &sil_phones, hipStream_t s);      // pool_mu_ held
  std::vector<int32_t> sil_bitmap_phones_;
  unsigned *d_sil_bitmap_ = nullptr;
  std::vector<unsigned> h_sil_bitmap_;
  // The split-fp16 layer GEMMs carry activations below 65520 in magnitude (nnet_gemm_b3.hip).  A kernel that meets a larger
  // one sets the flag of the decode context it runs for (DecodeContext::gemm_ovf: host memory the device writes to); a batch
  // call that finds it set after its wait repeats itself on the exact-FP32 kernels (a model whose calls keep doing that changes
  // to them for good); a stream advance cannot be repeated: its call fails and the model changes kernels at once.
  std::atomic<bool> exact_gemm_{false};
  std::atomic<int> range_retries_{0};     // batch calls repeated so far; the third makes the change permanent
  std::atomic<int> precision_retries_{0}; // ... of them, those repeated because an operand row was too small for the split (GemmDev::ovf[1])
  struct RangeRetry {};             // thrown by a batch call that has to be repeated on the exact kernels
  void StreamsCheckRange();         // the same for stream advances (stream.cc)
  bool CheckGemmRange(DecodeContext &cx);      // after a wait: true if this call ran on the split-fp16 kernels and one of them overflowed
  // Guard rows of the frame buffers / operand images of a call: layers evaluated on all rows read up to their context beyond
  // the first and last row; what they compute from those rows is never used, but it passes through the range check above.
  void ZeroGuards(const std::vector<float *> &bufp, const std::vector<int> &buf_ld, int rows, const std::vector<ActImage> *imgs, hipStream_t s) const;
  std::vector<int> pdf_remap_;     // prune_output_pdfs: pdf id -> column of the pruned output layer (-1 = never read)
  int pruned_from_ = 0;            // number of pdfs before pruning (0 = not pruned)
  void PruneOutputLayer();

  MfccDev mfcc_dev_{};
  FbankDev fbank_dev_{};           // --feature-type=fbank (fc_.mfcc.fbank): what the filterbank kernel reads beside mfcc_dev_
  // the model's base-feature kernel (MFCC or log-mel filterbank) over the rows of g; arguments as LaunchMfcc's
  void LaunchBaseFeatures(int dither_frames, const BatchGeom &g, const int16_t *pcm, float *feats, int ld, hipStream_t s, bool exclusive,
                          const int *out_rows = nullptr);
  // Dither noise of frames [0, dither_frames_) on the device (nnet3_setup.h: the reference's draws for frame t are a constant of
  // the model).  Grows on demand by doubling; the table a growth step supersedes stays alive until the next step (launches in flight may still read it).
  MfccDev MfccWithDither(int frames);
  std::mutex dither_mu_;           // guards d_dither_ / dither_frames_ (read, publish)
  std::mutex dither_grow_mu_;      // one thread grows the table at a time
  const float *d_dither_ = nullptr;
  int dither_frames_ = 0;
  long dither_rand_calls_ = 0;
  std::vector<void *> dither_bufs_;
  CmvnDev cmvn_iv_dev_{}, cmvn_nnet_dev_{};
  IvecDev ivec_dev_{};
  LayerOp lda_op_;                    // splice + LDA of the iVector branch, as a segmented GEMM
  GemmPlan lda_plan_;
  // The same as ONE segment: with a row pitch equal to the feature dim, the spliced vector of frame t is the contiguous run of
  // floats from row t - left onwards (rows overlap), so the per-frame segments' padding to the k-tile (40 -> 64) disappears
  LayerOp lda_op1_;
  GemmPlan lda_plan1_;
  const GemmPlan &LdaPlan(int ld) const { return (lda_plan1_.op && ld == fc_.mfcc.nceps) ? lda_plan1_ : lda_plan_; }
  std::vector<GemmPlan> gemm_plans_;  // indexed like am_.nnet.ops (unused entries for eltwise ops)
  std::vector<ConvLaunchPlan> conv_plans_;   // indexed like am_.nnet.ops: what the planner chose at load for the convolutions
  std::vector<ConvOperands> conv_dev_;       // indexed like am_.nnet.ops: the convolutions' and gathers' device operands
  std::vector<LstmLaunchPlan> lstm_plans_;   // indexed like am_.nnet.ops: what the planner chose at load for the recurrent blocks
  std::vector<LstmOperands> lstm_dev_;       // indexed like am_.nnet.ops: their device operands
  std::vector<LstmbLaunchPlan> lstmb_plans_; // ... and for the blocks behind a bottleneck (lstmb-layer)
  std::vector<LstmbOperands> lstmb_dev_;
  std::vector<GruLaunchPlan> gru_plans_;     // the same for the GRU blocks
  std::vector<AttentionLaunchPlan> attention_plans_;   // the same for the attention ops
  std::vector<GruOperands> gru_dev_;
  std::vector<PgruLaunchPlan> pgru_plans_;   // ... and for the blocks around a GruNonlinearityComponent
  std::vector<PgruOperands> pgru_dev_;
  float *d_log_priors_ = nullptr;
  HclgDev hclg_dev_{};
  RevGraphDev rev_dev_{};
  RegGraphDev reg_dev_{};
  // search_plan.h: the graph's sizes, the switches as the constructor found them, what they allow on this graph
  SearchGraph search_graph_{};
  SearchSwitches search_sw_{};
  SearchLoad search_load_{};
  int L_ = 0, R_ = 0;
};

}  // namespace rs

struct rs_model { std::unique_ptr<rs::Model> m; };
struct rs_result { std::unique_ptr<rs::Result> r; };
struct rs_stream {
  rs_model *model = nullptr;
  bool finished = false, open = false;
  std::atomic<bool> failed{false}; // an rs_streams_advance over this stream threw: schedule and device rows disagree, only close is allowed
  std::string fail_why;            // ... and, when the failure surfaced in another call (an advance's deferred work), its message (written before `failed`)
  bool keep_pcm = false;           // RS_STREAM_BATCH=1: keep every sample and replay the stream as one batch at finish (cross-check path)
  std::vector<int16_t> pcm;        // samples from absolute index pcm_start on (the ones no complete frame has consumed yet)
  long pcm_start = 0, n_samples = 0;
  int slot = -1, row0 = 0, cap = 0;   // the stream's slot and frame-row range in the model's pool
  int frames_mfcc = 0;             // MFCC (and CMVN) frames produced
  rs::ChunkCursor sched;           // the chunk schedule so far: ticks seen, nnet chunks computed (call_plan.h)
  int stats_done = 0;              // frames accumulated into the iVector statistics
  int ll_done = 0;                 // frames with log-likelihoods in the pool
  int frames_decoded = 0;          // frames the incremental search has consumed
  bool dec_started = false;
  // speaker adaptation
  bool ended = false;              // finished / finalized, slot and rows still held for rs_streams_adaptation
  bool reclaimed = false;          // ... no longer: the pool needed them
  int adapt_frames = 0;            // raw MFCC frames the state's CMVN statistics cover
  std::vector<double> spk0;        // speaker CMVN statistics the stream was opened with: [2 x (C + 1) iVector branch | 2 x (C + 1) nnet input], empty: none
  bool spk_iv = false, spk_nn = false;      // ... with a count above zero: the CMVN of that branch reads them from the slot
};
// online2/online-ivector-feature.h: OnlineIvectorExtractorAdaptationState, plus the nnet-input OnlineCmvnState where the model has one
struct rs_adaptation {
  int feat_dim = 0, ivec_dim = 0;
  bool has_iv = false, has_nn = false;
  std::vector<double> lin, quad;   // the estimator's linear term, its quadratic term (packed lower triangle, row by row)
  double num_frames = 0.0;
  std::vector<double> cmvn_iv, cmvn_nn;      // speaker CMVN statistics, 2 x (feat_dim + 1): iVector branch (limited), nnet input (not limited)
};

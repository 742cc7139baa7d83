// Host-only planning of a decode call: which nnet chunk is computed on which 1024-sample tick, which iVector row every nnet row
// reads, the estimator's step tables, the row lists of a batch, and the index arrays of one stream advance.  Plain integer
// arithmetic on sample counts: nothing here includes a HIP header, launches or allocates on the device, so the arrays the kernels
// later use as row indices can be built and checked on a machine without a GPU (tests/host/call_plan_check.cc).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace rs {

// feature-window.cc:42-87 (snip_edges only): frames of `num_samples` samples
inline int FramesOf(long num_samples, int window, int shift) { return num_samples < window ? 0 : (int)(1 + (num_samples - window) / shift); }

constexpr long kTickSamples = 1024;      // what online2-cli-nnet3-decode-faster reads at a time

struct PlanConfig {
  int window = 400, shift = 160;     // MFCC window and shift in samples
  int chunk = 24;                    // frames per nnet chunk
  int L = 0, R = 0;                  // halo rows a segment carries on either side (the network's context, at least the splice's)
  int Rm = 0;                        // the network's own right context
  bool has_iv = false;
  int sl = 0, sr = 0;                // iVector splice (0 without an extractor)
  int fsf = 1;                       // --frame-subsampling-factor
  int Frames(long ns) const { return FramesOf(ns, window, shift); }
  int DecFrames(int t) const { return (t + fsf - 1) / fsf; }      // decoder frames of the first t feature frames (decodable-online-looped.cc:56-84)
};

// ---------------------------------------------------------------- the chunk schedule, resumable
// online2-cli-nnet3-decode-faster.cc:143-161, decodable-online-looped.cc:56-84,186-194: chunk k is computed on the first tick at
// which chunk (k + 1) + Rm frames exist, with an iVector that has seen the frames of that tick less the splice's right context;
// after the end of input the remaining chunks see everything.  A function of the sample count alone, so it does not matter how
// many ticks one call covers.
struct ChunkCursor {
  long ticks_done = 0;               // 1024-sample ticks the schedule has seen
  int chunks_sched = 0;              // nnet chunks scheduled
};
using ChunkList = std::vector<std::pair<int, int>>;      // (chunk index, last frame its iVector statistics have seen)
// Appends the chunks the first `ns` samples make computable beyond `cur` and advances it.  flush: end of input -- the partial last
// tick counts and the rest of the chunks get the last frame.
void ScheduleChunks(const PlanConfig &c, long ns, bool flush, ChunkCursor *cur, ChunkList *out);

// ---------------------------------------------------------------- which iVector row a nnet row reads
// Rows of the frames t_first, t_first + 1, ... (nr of them): the chunk whose iVector the row's Round(ivector, chunk) slot was supplied
// by (nnet-compile-looped.cc:164-231: chunk 0 supplies the slots of t in [-L, chunk + R), chunk k the new ones of
// [k chunk + R, (k + 1) chunk + R)) = the number of chunks j >= 1 with j chunk + Rm <= slot, at most kmax (the last scheduled one);
// out[r] = ivrow0 + that.  t / chunk is carried along instead of divided out per row (the division was 3.7 ms of a 24 ms step).
void FillIvecRows(const PlanConfig &c, int t_first, int nr, int kmax, int ivrow0, int *out);

// ---------------------------------------------------------------- the estimator's [step][unit] tables
struct StepTables {
  std::vector<int> fb, fe, orow, act;      // frame begin / end (relative to the unit's first statistics row), iVector row, "has new frames"
  void Reset(size_t steps, size_t units) { const size_t n = steps * units; fb.assign(n, 0); fe.assign(n, 0); orow.assign(n, -1); act.assign(n, 0); }
};
// Column `unit` of n_units: step k is the unit's k-th new chunk.  stats_done: the first statistics frame not yet accumulated (row 0
// of the unit's segment); ivrow0: the unit's first iVector row.
void FillStepTables(const ChunkList &chunks, int stats_done, int ivrow0, int unit, int n_units, StepTables *t);

// The streamed replay of a batch (DecodeGroup(streaming = true)): every utterance's whole schedule at once.
struct BatchSchedule {
  std::vector<int> ivrow_base;       // first iVector row of each utterance (n + 1)
  StepTables steps;                  // [max_chunks][n]
  int max_chunks = 1;
};
// row_ivec: row_base[n] entries, the iVector row of every nnet row (the caller's staging memory)
void PlanBatchSchedule(const PlanConfig &c, const long *n_samples, const int *T, const int *row_base, int n, int *row_ivec, BatchSchedule *out);

// ---------------------------------------------------------------- row lists of a batch
// The physical rows `window` consecutive entries of a stride-1 list reach over, exactly: the list is one run of consecutive rows per
// utterance with frames (t in [-lext, T + rext): T + lext + rext entries from row row_base + L - lext on); a window of 128 entries
// that holds the last entry of run a and the first of run b crosses every gap between them, and it can do so when the runs in
// between hold at most 126 entries.  An utterance without frames has no entries but still owns L + R rows (a too-short clip
// inside a batch), so the gap between two runs is not bounded by one halo: GemmKernelB3J's strip form trusts this number.
// runs: (first physical row, entries), ascending, no empty ones.
int SpanOfRuns(const std::vector<std::pair<int, int>> &runs, int window);

// Which row lists a batch needs: the real frames in slab-major order (slab k = frames [k * slab_len, (k + 1) * slab_len) of
// every utterance: layers nothing downstream reads with a time offset are evaluated on these rows only), and per hidden layer
// only as much halo as the layers after it reach (15 rows a side for the first, none for the last of the zamia-like net:
// 5 % fewer rows over the stack than evaluating the full halo everywhere).
struct RowList {
  int lext = 0, rext = 0, n_segs = 0, total = 0, L_eff = 0, slab_len = 0, span128 = 0;
  size_t seg_at = 0;                 // its n_segs + 1 segment offsets in RowListPlan::segs
  int stride = 1, first = 0, span160 = 0;
};
struct BufExtent { int lext, rext, stride; };      // of the buffer an op writes (BufferInfo)
struct RowListPlan {
  std::vector<RowList> lists;
  std::vector<int> segs;             // the lists' segment offsets, back to back
  std::vector<int> slab_off;         // n_slabs + 1: the frame list's first entry of every slab
};
enum class RowListStatus { kOk, kStridedInSlabs, kTooManyStrided };
// T / row_base: per utterance (row_base: n + 1); op_out: per op of the network, in order; max_lists: BatchSetup::kMaxLists;
// trim_halo: RS_TRIM_HALO.  A status other than kOk: the plan is not usable.
RowListStatus PlanRowLists(const int *T, const int *row_base, int n_utts, int maxT, int L, int R, const std::vector<BufExtent> &op_out, int n_slabs,
                           int slab_len, int max_lists, bool trim_halo, RowListPlan *out);

// ---------------------------------------------------------------- one stream advance
struct StreamView {                  // what the plan reads of a stream
  long n_samples = 0;
  ChunkCursor sched;
  int frames_mfcc = 0, stats_done = 0, ll_done = 0, frames_decoded = 0;
  bool dec_started = false;
  int row0 = 0, slot = 0;
  bool spk_iv = false, spk_nn = false;
};
struct StreamAdvance {
  int avail = 0;                     // frames computable from the samples accepted so far
  int mf0 = 0;                       // first new MFCC frame
  ChunkList chunks;                  // new nnet chunks
  int sa = 0, sb = 0;                // frames to splice / LDA / score for the iVector statistics: [sa, sb)
  int t0 = 0, t1 = 0;                // frames that get log-likelihoods in this advance: [t0, t1)
  ChunkCursor sched;                 // the stream's cursor after this advance
};
// Built in two steps, because a stream that outgrew its rows moves between them (StreamGrow: device work, changes row0):
//   PlanAdvanceSchedule  reads everything of the views but row0: `pl` (avail says how many rows each stream needs);
//   PlanAdvanceRows      with the final row0 of every view: the index arrays and the staging block.
// One object per arena set, reused: the vectors keep their capacity from advance to advance.
struct AdvancePlan {
  int n = 0;
  std::vector<StreamAdvance> pl;
  int max_new_chunks = 0;
  // stage 1, MFCC over the new frames (dense rows, no halo), rows -> pool; stage 2, CMVN resumed: the same streams
  int nM = 0, rowsM = 0;
  size_t pcm_total = 0;
  std::vector<int> m_T, m_rb, m_out, m_f0;
  std::vector<int64_t> m_so;
  std::vector<int> c_T, c_rb, c_tb, c_slot, c_spk_iv, c_spk_nn;
  bool any_spk_iv = false, any_spk_nn = false;      // a stream of the call carries speaker statistics: the CMVN kernel with that term
  // stage 3, iVector segments: the streams with new chunks
  int nI = 0, rowsI = 0;
  std::vector<int> I_idx, i_T, i_rb, i_src, i_slot;
  StepTables steps;
  // stage 4, nnet segments: the streams with new log-likelihood frames; per row the pool row it is gathered from (context rows
  // clamped to the stream's frames) and its iVector row; per output frame the pool row it goes to
  int nN = 0, rowsN = 0, framesN = 0, maxTn = 0;
  std::vector<int> N_idx, n_T, n_rb, n_fb, n_src, n_riv, n_lldst, n_llsrc;
  // stage 5, search windows (every stream of the call: a stream that ends without new rows still needs its traceback)
  int maxT = 0, max_feat_frames = 0;     // decoder frames / feature frames (the dither table is indexed by FEATURE frames)
  std::vector<int> d_T, d_rb, w_b, w_e, w_f, slots, row0s;
  std::vector<int> avails;               // decoder frames a final stage covers (host only)
  // the staging block: every array above, each padded to four ints, at these offsets
  std::vector<int> stage;
  struct Offsets {
    size_t mT, mrb, mout, mf0, mso, cT, crb, ctb, cslot, cspki, cspkn, iT, irb, isrc, islot, sfb, sfe, sor, sac, nT, nrb, nfb, nsrc, nriv, nll, nlls, dT, drb, wb,
        we, wf, slots, row0;
  } o{};
};
void PlanAdvanceSchedule(const PlanConfig &c, const StreamView *views, int n, bool flush, AdvancePlan *plan);
void PlanAdvanceRows(const PlanConfig &c, const StreamView *views, int n, bool flush, bool final, AdvancePlan *plan);

}  // namespace rs

// The walk every recurrent block kernel makes over the rows of a call (nnet_lstm.hip, nnet_lstmp.hip, nnet_lstmb.hip, nnet_gru.hip,
// nnet_pgru.hip, nnet_gruc.hip): which rows a chain visits, where a stream advance re-enters and which step's state row it parks.
// Host and device: nothing here includes a HIP header, the planners' host checks and tests/host/recurrent_walk_check.cc compile it
// with g++.
//
// Row t of a block needs row t - delay only, so the rows of an utterance fall into `delay` independent CHAINS, t = first, first +
// delay, ... (delay / stride of them where only every stride-th row is read, --frame-subsampling-factor), and the chains of
// different utterances never meet.  A workgroup of kRecWaves waves owns kRecChains chains for the whole launch (lstm_plan.h).
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define RS_HOST_DEVICE __host__ __device__
#else
#define RS_HOST_DEVICE
#endif

namespace rs {

constexpr int kRecChains = 16;                 // chains of a workgroup: the rows of one MFMA tile
constexpr int kRecWaves = 8;                   // waves of a workgroup
constexpr int kRecMaxLdsBytes = 144 * 1024;    // the LDS tiles of one workgroup (of the CU's 160 KiB)
constexpr int kLstmMaxDelay = 8;               // frames towards the past a block may reach

struct RecWalk {
  int delay, stride;
  // geometry: utterance u has frames [0, T_u) at rows row_base[u] + L + t; the walk covers t in [-lext, T_u + rext) (nothing where T_u = 0)
  int n_utts, L, lext, rext;
  const int *num_frames, *row_base;
  // streams: utterance u is the advance of a stream that has computed t0[u] frames before (t0 > 0: the walk re-enters at
  // -lext_cont, and a chain's first step reads the state row parked for it: ring row (t0 + t) mod delay of slot[u]); every chain parks
  // the state row the next advance re-enters behind, the t in [T_u - lext_cont - delay, T_u - lext_cont).  null: a batch call.
  const int *t0, *slot;
  int lext_cont;
  float *ring;           // [slot][delay][state_w]
  int state_w;           // floats of one parked row: the block's StateDim() (model.h)
};

// per chain of the workgroup
struct RecChain {
  int row0;        // physical row of the chain's first step; step n is row0 + n * delay
  int count;       // steps
  int ring_off;    // streams: offset of the chain's parked state row in RecWalk::ring
  int cont;        // its first step continues from the parked row (else from zeros)
  int save_step;   // the step whose state row is parked for the next advance, -1: none
};

// chains of a launch: per utterance with rows delay / stride (stride divides the delay wherever it is above 1: Nnet::SetSubsampling)
constexpr int RecChainsPerUtt(int delay, int stride) { return stride > 1 ? delay / stride : delay; }
constexpr int RecGridX(int n_utts, int delay, int stride) { return (n_utts * RecChainsPerUtt(delay, stride) + kRecChains - 1) / kRecChains; }

// chain `chain_index` of the launch (workgroup * kRecChains + its place in the workgroup): chain c of utterance u, the class t = c * step mod delay
RS_HOST_DEVICE inline RecChain RecChainSetUp(const RecWalk &w, int chain_index) {
  const int per_utt = RecChainsPerUtt(w.delay, w.stride), step = w.stride > 1 ? w.stride : 1;
  const int u = chain_index / per_utt, c = chain_index - u * per_utt;
  RecChain ch = {0, 0, 0, 0, -1};
  const int T = u < w.n_utts ? w.num_frames[u] : 0;
  if (T > 0) {
    const int t0 = w.t0 ? w.t0[u] : 0;
    ch.cont = w.slot != nullptr && t0 > 0;
    const int t_start = ch.cont ? -w.lext_cont : -w.lext, t_end = T + w.rext;
    int m = (c * step - t_start) % w.delay;      // the first t >= t_start of the chain's class
    if (m < 0) m += w.delay;
    const int t_first = t_start + m;
    if (t_first < t_end) ch.count = (t_end - 1 - t_first) / w.delay + 1;
    ch.row0 = w.row_base[u] + w.L + t_first;
    if (w.slot) {
      int rr = (t0 + t_first) % w.delay;
      if (rr < 0) rr += w.delay;
      ch.ring_off = (w.slot[u] * w.delay + rr) * w.state_w;
      const int re = T - w.lext_cont;            // where the next advance re-enters: it reads the rows [re - delay, re)
      if (re - 1 >= t_first) ch.save_step = (re - 1 - t_first) / w.delay;
    }
  }
  return ch;
}

}  // namespace rs

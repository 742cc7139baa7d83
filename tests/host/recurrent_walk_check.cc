// Host check of the walk the recurrent block kernels share (rhasspy_speech_amd/csrc/recurrent_walk.h): RecChainSetUp for every chain
// index of the grid, over every delay, stride, extent, length and stream position the kernels can meet, against an enumeration of
// the rows written here from the walk's definition alone.  Its own main; built with the address and undefined-behaviour sanitizers
// (tests/test_recurrent_walk_cpu.py), so an index past the two utterances' arrays is an error too.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/recurrent_walk.h"

namespace {

struct Case {
  int delay, stride, lext, rext, lext_cont;
  bool stream;
  int T[2], t0[2];
};

[[noreturn]] void Bad(const Case &k, int chain, const char *what) {
  std::printf("FAILED: %s (delay %d stride %d lext %d rext %d lext_cont %d %s T %d,%d t0 %d,%d chain %d)\n", what, k.delay, k.stride, k.lext, k.rext,
              k.lext_cont, k.stream ? "stream" : "batch", k.T[0], k.T[1], k.t0[0], k.t0[1], chain);
  std::exit(1);
}
#define REQUIRE(cond, what) do { if (!(cond)) Bad(k, chain, what); } while (0)

int Mod(int a, int m) { return ((a % m) + m) % m; }

constexpr int kL = 12, kStateW = 7, kRowBase[2] = {5, 70}, kSlot[2] = {3, 1}, kSlots = 4;

// heap arrays of exactly two entries: a read for an utterance beyond them is caught
struct Utts {
  std::vector<int> num_frames = std::vector<int>(2), row_base = std::vector<int>(kRowBase, kRowBase + 2), t0 = std::vector<int>(2),
                   slot = std::vector<int>(kSlot, kSlot + 2);
};

long Check(const Case &k, Utts *utts) {
  std::vector<int> &num_frames = utts->num_frames, &row_base = utts->row_base, &t0 = utts->t0, &slot = utts->slot;
  for (int u = 0; u < 2; u++) { num_frames[u] = k.T[u]; t0[u] = k.t0[u]; }
  rs::RecWalk w{};
  w.delay = k.delay; w.stride = k.stride;
  w.n_utts = 2; w.L = kL; w.lext = k.lext; w.rext = k.rext;
  w.num_frames = num_frames.data(); w.row_base = row_base.data();
  w.t0 = k.stream ? t0.data() : nullptr; w.slot = k.stream ? slot.data() : nullptr;
  w.lext_cont = k.lext_cont; w.ring = nullptr; w.state_w = kStateW;

  const int step = k.stride > 1 ? k.stride : 1, per_utt = k.delay / step;
  int chain = -1;
  REQUIRE(rs::RecChainsPerUtt(k.delay, k.stride) == per_utt, "chains per utterance");
  const int grid = rs::RecGridX(2, k.delay, k.stride);
  REQUIRE(grid * rs::kRecChains >= 2 * per_utt && (grid - 1) * rs::kRecChains < 2 * per_utt, "grid");

  // visits[u][t + span]: how often a chain's step lands on row t of utterance u
  const int span = k.delay + 2, width = span + 2 * k.delay + 3 + k.delay + 2;
  int visits[2][4 * rs::kLstmMaxDelay + 9] = {};
  bool ring_row_taken[kSlots * rs::kLstmMaxDelay] = {};
  long steps = 0;
  for (chain = 0; chain < grid * rs::kRecChains; chain++) {
    const rs::RecChain ch = rs::RecChainSetUp(w, chain);
    const int u = chain / per_utt, c = chain % per_utt;
    if (u >= 2 || k.T[u] == 0) {
      REQUIRE(ch.count == 0, "a chain without an utterance, or of an empty one, has steps");
      continue;
    }
    const int T = k.T[u];
    const bool cont = k.stream && k.t0[u] > 0;
    REQUIRE((ch.cont != 0) == cont, "cont");
    const int t_start = cont ? -k.lext_cont : -k.lext, t_end = T + k.rext;
    // the chain's class, by definition: every t with t = c * step (mod delay)
    int t_first = t_start;
    while (Mod(t_first - c * step, k.delay) != 0) t_first++;
    int n = 0;
    for (int t = t_start; t < t_end; t++) {
      if (Mod(t - c * step, k.delay) != 0) continue;
      REQUIRE(n < ch.count, "a row of the chain's class is not visited");
      REQUIRE(ch.row0 + n * k.delay == kRowBase[u] + kL + t, "a step's row");
      visits[u][t + span]++;
      n++;
    }
    REQUIRE(n == ch.count, "steps beyond the rows of the chain's class");
    steps += n;
    if (!k.stream) {
      REQUIRE(ch.save_step == -1 && ch.ring_off == 0, "a batch call parks nothing");
      continue;
    }
    // the row the next advance re-enters behind: the one member of the class in [T - lext_cont - delay, T - lext_cont)
    int t_save = T - k.lext_cont - k.delay, members = 0;
    for (int t = T - k.lext_cont - k.delay; t < T - k.lext_cont; t++)
      if (Mod(t - c * step, k.delay) == 0) { t_save = t; members++; }
    REQUIRE(members == 1, "the check's own window");
    if (t_save < t_first) {
      REQUIRE(ch.save_step == -1, "save_step where the parked row lies before the chain's first step");
    } else {
      REQUIRE(ch.save_step >= 0 && ch.save_step < ch.count, "save_step is not a step of the chain");
      REQUIRE(ch.row0 + ch.save_step * k.delay == kRowBase[u] + kL + t_save, "save_step's row");
    }
    REQUIRE(ch.ring_off >= 0, "a negative ring offset");
    REQUIRE(ch.ring_off == (kSlot[u] * k.delay + Mod(k.t0[u] + t_first, k.delay)) * kStateW, "ring_off");
    REQUIRE(ch.ring_off + kStateW <= kSlots * k.delay * kStateW, "a ring row beyond the slots");
    REQUIRE(!ring_row_taken[ch.ring_off / kStateW], "two chains share a ring row");
    ring_row_taken[ch.ring_off / kStateW] = true;
  }
  chain = -1;
  for (int u = 0; u < 2; u++) {
    const bool cont = k.stream && k.t0[u] > 0;
    const int t_start = cont ? -k.lext_cont : -k.lext, t_end = k.T[u] + k.rext;
    for (int t = -span; t < width - span; t++) {
      const bool in_walk = k.T[u] > 0 && t >= t_start && t < t_end && Mod(t, k.delay) % step == 0;
      REQUIRE(visits[u][t + span] == (in_walk ? 1 : 0), "a row is not visited exactly once");
    }
  }
  return steps;
}

}  // namespace

int main() {
  long cases = 0, steps = 0;
  Utts utts;
  for (int delay = 1; delay <= rs::kLstmMaxDelay; delay++)
    for (int stride = 1; stride <= delay; stride++) {
      if (delay % stride != 0) continue;      // (1, and every divisor of the delay above 1)
      for (int lext = 0; lext <= delay + 1; lext++)
        for (int rext = 0; rext <= delay + 1; rext++)
          for (int lext_cont = 0; lext_cont <= delay + 1; lext_cont++)
            for (int T = 0; T <= 2 * delay + 3; T++)
              for (int mode = 0; mode < 5; mode++) {      // batch, then a stream at t0 = 0, 1, delay, delay + 1
                const int t0s[4] = {0, 1, delay, delay + 1};
                Case k;
                k.delay = delay; k.stride = stride; k.lext = lext; k.rext = rext; k.lext_cont = lext_cont;
                k.stream = mode > 0;
                // (the second utterance: another length and another stream position, so the two differ in every case)
                k.T[0] = T; k.T[1] = (T + delay + 1) % (2 * delay + 4);
                k.t0[0] = t0s[mode > 0 ? mode - 1 : 0]; k.t0[1] = t0s[mode > 0 ? mode % 4 : 0];
                steps += Check(k, &utts);
                cases++;
              }
    }
  std::printf("recurrent walk: %ld cases, %ld steps, all as enumerated\n", cases, steps);
  return 0;
}

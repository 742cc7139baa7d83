// Stand-alone check of the hinted Reset of csrc/arena.h and of the shared high-water mark (tests/test_arena_hint_cpu.py builds it
// with the host compiler, once under the address and undefined-behaviour sanitizers and once under the thread sanitizer, and runs
// it as a child process).
//
// Without arguments: Arena over malloc / free backends that record their calls and poison what they free, one like the device's
// (256-byte alignment, the last 1 MiB of a block reserved), one like the host's (64 bytes, nothing reserved).  Commands on stdin,
// one per line; one line of output each.
//   new dev|host          destroys the arena (every block freed exactly once, or the program aborts) and makes a fresh one
//   round r1 r2 ...       Reset(s), then the requests in order
//   hint E r1 r2 ...      Reset(s, E), then the requests in order
//                         Every buffer is filled with its own byte when it is handed out, and all of them are read back once the
//                         last request is served.  Output of both:
//                           allocations frees synchronisations blocks bytes round | block:offset of every pointer
//                         (round: Arena::round() once the requests are served -- what a sibling would be given as its hint)
// The program asserts for itself: alignment, that every buffer lies inside one live block and ends before its reserved tail, that
// no two buffers of a round overlap (the read-back), and that the arena's counters are the backend's.
//
// `marks THREADS ROUNDS`: that many threads, released together, each run ROUNDS times "fresh arena, Reset with the shared mark, fixed
// requests, publish the round".  Asserted: the mark never decreases, it ends at the round's size, and every round that starts after
// some thread has published makes exactly one backend allocation (and no synchronisation).  Output: one line of counts.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/arena.h"

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "arena_hint_check: %s failed: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::abort(); } } while (0)

struct Log {
  std::vector<std::pair<char *, size_t>> live;
  size_t allocations = 0, frees = 0, syncs = 0;
};
static Log g_log;

template <size_t Align, size_t Tail>
struct Recording {
  static constexpr size_t kAlign = Align, kTail = Tail;
  using Stream = int;
  void *Allocate(size_t bytes, Stream s) {
    CHECK(s == 7, "a block allocated on stream %d, not the one of the last Reset", s);
    char *p = static_cast<char *>(std::aligned_alloc(Align, (bytes + Align - 1) / Align * Align));
    CHECK(p != nullptr, "out of memory (%zu bytes)", bytes);
    g_log.live.push_back({p, bytes});
    g_log.allocations++;
    return p;
  }
  void Free(void *p) {
    auto it = std::find_if(g_log.live.begin(), g_log.live.end(), [&](const std::pair<char *, size_t> &b) { return b.first == p; });
    CHECK(it != g_log.live.end(), "a block freed twice, or one the backend never allocated");
    std::memset(it->first, 0xDD, it->second);
    std::free(it->first);
    g_log.live.erase(it);
    g_log.frees++;
  }
  void Synchronize(Stream s) { CHECK(s == 7, "stream %d", s); g_log.syncs++; }
};

struct AnyArena {
  virtual ~AnyArena() {}
  virtual std::string Round(bool hinted, size_t expect, const std::vector<size_t> &req) = 0;
};

template <class Backend>
struct Checked : AnyArena {
  rs::Arena<Backend> arena;
  ~Checked() override {}
  std::string Round(bool hinted, size_t expect, const std::vector<size_t> &req) override {
    if (hinted) arena.Reset(7, expect);
    else arena.Reset(7);
    std::vector<char *> ptr;
    std::ostringstream where;
    for (size_t i = 0; i < req.size(); i++) {
      char *p = static_cast<char *>(arena.Alloc(req[i]));
      CHECK(reinterpret_cast<uintptr_t>(p) % Backend::kAlign == 0, "request %zu (%zu bytes) is not aligned", i, req[i]);
      size_t b = 0;
      while (b < g_log.live.size() && !(p >= g_log.live[b].first && p <= g_log.live[b].first + g_log.live[b].second)) b++;
      CHECK(b < g_log.live.size(), "request %zu lies in no live block", i);
      const size_t off = (size_t)(p - g_log.live[b].first);
      CHECK(off + req[i] <= g_log.live[b].second - Backend::kTail, "request %zu: [%zu, %zu) reaches into the tail of a block of %zu bytes", i, off, off + req[i],
            g_log.live[b].second);
      std::memset(p, (int)(i % 251) + 1, req[i]);
      ptr.push_back(p);
      where << " " << b << ":" << off;
    }
    for (size_t i = 0; i < req.size(); i++)      // (after a spill: the earlier buffers are still there, and nobody wrote over them)
      for (size_t k = 0; k < req[i]; k++) CHECK((unsigned char)ptr[i][k] == i % 251 + 1, "request %zu, byte %zu was overwritten", i, k);
    size_t bytes = 0;
    for (auto &b : g_log.live) bytes += b.second;
    CHECK(arena.blocks() == g_log.live.size() && arena.bytes() == bytes && arena.allocations() == g_log.allocations, "counters");
    std::ostringstream os;
    os << g_log.allocations << " " << g_log.frees << " " << g_log.syncs << " " << g_log.live.size() << " " << bytes << " " << arena.round() << " |" << where.str();
    return os.str();
  }
};

static int Commands() {
  std::unique_ptr<AnyArena> arena;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "new") {
      std::string kind;
      in >> kind;
      arena.reset();
      CHECK(g_log.live.empty() && g_log.frees == g_log.allocations, "%zu blocks outlive their arena", g_log.live.size());
      g_log = Log();
      if (kind == "dev") arena.reset(new Checked<Recording<256, (size_t)1 << 20>>());
      else arena.reset(new Checked<Recording<64, 0>>());
      std::cout << "new\n";
    } else if (cmd == "round" || cmd == "hint") {
      CHECK(arena != nullptr, "%s before new", cmd.c_str());
      size_t expect = 0;
      if (cmd == "hint") CHECK(static_cast<bool>(in >> expect), "hint without a size");
      std::vector<size_t> req;
      for (size_t r; in >> r;) req.push_back(r);
      std::cout << cmd << " " << arena->Round(cmd == "hint", expect, req) << "\n";
    } else {
      CHECK(false, "unknown command %s", cmd.c_str());
    }
  }
  arena.reset();
  CHECK(g_log.live.empty() && g_log.frees == g_log.allocations, "%zu blocks outlive their arena", g_log.live.size());
  return 0;
}

// ---- the shared mark: every thread counts its own backend calls
struct Counting {
  static constexpr size_t kAlign = 256, kTail = (size_t)1 << 20;
  using Stream = int;
  static thread_local size_t allocations, frees, syncs;
  void *Allocate(size_t bytes, Stream) {
    void *p = std::malloc(bytes);
    CHECK(p != nullptr, "out of memory (%zu bytes)", bytes);
    allocations++;
    return p;
  }
  void Free(void *p) { std::free(p); frees++; }
  void Synchronize(Stream) { syncs++; }
};
thread_local size_t Counting::allocations = 0;
thread_local size_t Counting::frees = 0;
thread_local size_t Counting::syncs = 0;

static int Marks(int n_threads, int n_rounds) {
  const std::vector<size_t> req = {0, 1, 255, 3 * ((size_t)1 << 20) + 17, 64, 2 * ((size_t)1 << 20) + 1, 12345, 7};
  size_t want = 0;
  for (size_t r : req) want = ((want + Counting::kAlign - 1) & ~(Counting::kAlign - 1)) + r;
  rs::RoundMark mark;
  std::atomic<int> ready{0}, published{0};
  std::atomic<size_t> hinted{0}, cold{0};
  auto body = [&] {
    ready.fetch_add(1);
    while (ready.load() < n_threads) std::this_thread::yield();
    size_t seen = 0;
    for (int k = 0; k < n_rounds; k++) {
      const bool after_publisher = published.load(std::memory_order_acquire) > 0;
      const size_t a0 = Counting::allocations, f0 = Counting::frees, s0 = Counting::syncs;
      {
        rs::Arena<Counting> arena;
        const size_t expect = mark.get();
        CHECK(expect >= seen, "the mark went from %zu back to %zu", seen, expect);
        CHECK(expect == 0 || expect == want, "a mark of %zu bytes: the round has %zu", expect, want);
        CHECK(!after_publisher || expect == want, "no mark after a thread has published");
        seen = expect;
        arena.Reset(7, expect);
        for (size_t i = 0; i < req.size(); i++) {
          char *p = static_cast<char *>(arena.Alloc(req[i]));
          if (req[i]) p[0] = p[req[i] - 1] = (char)i;
        }
        CHECK(arena.round() == want, "a round of %zu bytes, not %zu", arena.round(), want);
        const size_t made = Counting::allocations - a0;
        if (expect) CHECK(made == 1 && arena.blocks() == 1, "a hinted cold round made %zu allocations", made);
        else CHECK(made > 1, "an unhinted cold round of %zu bytes in one block", want);
        CHECK(Counting::syncs == s0 && Counting::frees == f0, "a cold round freed or waited");
        (expect ? hinted : cold).fetch_add(1);
        mark.Raise(arena.round());
        published.fetch_add(1, std::memory_order_release);
        const size_t now = mark.get();
        CHECK(now == want, "the mark is %zu after %zu was published", now, want);
        seen = now;
      }
      CHECK(Counting::frees - f0 == Counting::allocations - a0, "blocks outlive their arena");
    }
  };
  std::vector<std::thread> th;
  for (int t = 0; t < n_threads; t++) th.emplace_back(body);
  for (auto &t : th) t.join();
  CHECK(mark.get() == want, "the mark ends at %zu, the round has %zu", mark.get(), want);
  CHECK(hinted.load() + cold.load() == (size_t)n_threads * n_rounds && cold.load() >= 1 && cold.load() <= (size_t)n_threads, "%zu unhinted rounds", cold.load());
  std::cout << "marks threads=" << n_threads << " rounds=" << n_rounds << " unhinted=" << cold.load() << " hinted=" << hinted.load() << " mark=" << mark.get() << "\n";
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && std::string(argv[1]) == "marks") return Marks(std::atoi(argv[2]), std::atoi(argv[3]));
  CHECK(argc == 1, "usage: arena_hint_check [marks THREADS ROUNDS]");
  return Commands();
}

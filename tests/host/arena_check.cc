// Stand-alone check of csrc/arena.h (tests/test_arena_cpu.py builds it with the host compiler and the address and undefined-behaviour
// sanitizers, and runs it as a child process).  Arena is instantiated over malloc / free backends that record their calls and
// poison what they free: one like the device's (256-byte alignment, the last 1 MiB of a block reserved), one like the host's
// (64 bytes, nothing reserved).  Commands on stdin, one per line; one line of output each.
//   new dev|host          destroys the arena (every block freed exactly once, or the program aborts) and makes a fresh one
//   round r1 r2 ...       Reset, then the requests in order.  Every buffer is filled with its own byte when it is handed out, and all
//                         of them are read back once the last request is served.  Output:
//                           allocations frees synchronisations blocks bytes | block:offset of every pointer
// The program asserts for itself: alignment, that every buffer lies inside one live block and ends before its reserved tail, that
// no two buffers of a round overlap (the read-back), and that the arena's counters are the backend's.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../rhasspy_speech_amd/csrc/arena.h"

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "arena_check: %s failed: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::abort(); } } while (0)

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
  virtual std::string Round(const std::vector<size_t> &req) = 0;
};

template <class Backend>
struct Checked : AnyArena {
  rs::Arena<Backend> arena;
  ~Checked() override {}
  std::string Round(const std::vector<size_t> &req) override {
    arena.Reset(7);
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
    os << g_log.allocations << " " << g_log.frees << " " << g_log.syncs << " " << g_log.live.size() << " " << bytes << " |" << where.str();
    return os.str();
  }
};

int main() {
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
    } else if (cmd == "round") {
      CHECK(arena != nullptr, "round before new");
      std::vector<size_t> req;
      for (size_t r; in >> r;) req.push_back(r);
      std::cout << "round " << arena->Round(req) << "\n";
    } else {
      CHECK(false, "unknown command %s", cmd.c_str());
    }
  }
  arena.reset();
  CHECK(g_log.live.empty() && g_log.frees == g_log.allocations, "%zu blocks outlive their arena", g_log.live.size());
  return 0;
}

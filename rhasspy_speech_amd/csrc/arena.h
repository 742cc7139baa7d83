// The memory of one decode call: bump allocation out of blocks a backend supplies, everything handed back at once by Reset().
// Nothing here includes a HIP header, so the growth rules are checked on a machine without a GPU (tests/host/arena_check.cc,
// tests/host/arena_hint_check.cc).
//
// Nobody sizes an arena.  A request that does not fit the current block appends a block (pointers handed out earlier stay valid
// until the next Reset), and the Reset after such a round replaces the blocks by one that holds the whole round -- from then on
// the same sequence of requests lands at the same offsets of that block and the backend is not called again: a warm call makes no
// hipMalloc / hipFree (either one stalls every other call in flight on the device).
//
// An arena may be TOLD what to expect: Reset(s, expect) with the round() of an arena that has served the same kind of call (the
// decode contexts of one model: RoundMark).  An arena without a block then starts with the one block it would have ended up with
// -- one backend call instead of a dozen and a coalescing Reset that waits, frees and allocates while the siblings' calls run.  The
// hint is never needed to be right: a round that outgrows it spills and is coalesced like any other, and an arena that has its one
// block keeps it whatever it is told.
//
// Backend: kAlign (a power of two; Allocate returns memory aligned to it), kTail (bytes at the end of every block that are never
// handed out), Stream, Allocate(bytes, stream), Free(p), Synchronize(stream).
#pragma once
#include <atomic>
#include <cstddef>
#include <vector>

namespace rs {

template <class Backend>
class Arena {
 public:
  using Stream = typename Backend::Stream;
  Arena() = default;
  Arena(const Arena &) = delete;
  Arena &operator=(const Arena &) = delete;
  ~Arena() { Release(); }

  // Everything handed out so far is free again.  A round that fitted one block: no backend call.  A round that spilled: waits for
  // `s`, frees the blocks and allocates one for the whole round -- the caller knows that nothing else still uses the arena's memory.
  // Blocks appended during the round that follows are allocated on `s`.
  void Reset(Stream s) { Reset(s, 0); }
  // The same, expecting a round of `expect` bytes (a sibling's round(); 0: nothing known).  An arena without a block gets the block
  // for such a round now, a spilled one is coalesced into a block for the larger of its own round and `expect`; an arena with one
  // block is left alone (a warm context does not allocate again because a sibling once saw a larger call).
  void Reset(Stream s, size_t expect) {
    stream_ = s;
    const size_t round = round_;
    used_ = round_ = 0;
    if (blocks_.size() > 1) {
      backend_.Synchronize(s);
      Release();
      Append(round > expect ? round : expect);
    } else if (blocks_.empty() && expect > 0) {
      Append(expect);
    }
  }
  void *Alloc(size_t bytes) {
    size_t at = Up(used_);
    if (blocks_.empty() || at + bytes > blocks_.back().size - Backend::kTail) { Append(Up(round_) + bytes); at = 0; }
    used_ = at + bytes;
    round_ = Up(round_) + bytes;      // where the round would end in ONE block: what the next Reset asks for after a spill
    return blocks_.back().p + at;
  }
  template <typename T> T *AllocT(size_t n) { return static_cast<T *>(Alloc(n * sizeof(T))); }
  // The round so far in one-block terms: once its last request is served, what the next Reset asks for if the round spilled, and
  // what a sibling is given as `expect`.  For the thread that makes the requests (not atomic).
  size_t round() const { return round_; }

  // (atomic: Model::Describe reads them while calls run)
  size_t blocks() const { return n_blocks_.load(std::memory_order_relaxed); }
  size_t bytes() const { return bytes_.load(std::memory_order_relaxed); }
  size_t allocations() const { return allocations_.load(std::memory_order_relaxed); }      // backend allocations since construction

 private:
  struct Block { char *p; size_t size; };
  static size_t Up(size_t x) { return (x + Backend::kAlign - 1) & ~(Backend::kAlign - 1); }
  // A block for `need` bytes plus an eighth plus 1 MiB, and the tail behind that.  `need` is the whole round so far and a block is
  // left only when it is full, so the rounds' totals at which a cold round appends grow like 1 MiB times the Fibonacci numbers:
  // at most 2 + 1.44 (log2(N) - 20) backend calls for a round of N bytes.
  void Append(size_t need) {
    const size_t size = need + need / 8 + ((size_t)1 << 20) + Backend::kTail;
    blocks_.push_back({static_cast<char *>(backend_.Allocate(size, stream_)), size});
    n_blocks_++; bytes_ += size; allocations_++;
  }
  void Release() {
    for (Block &b : blocks_) backend_.Free(b.p);
    blocks_.clear();
    n_blocks_ = 0; bytes_ = 0;
  }

  Backend backend_;
  Stream stream_{};
  std::vector<Block> blocks_;      // requests come out of the last one
  size_t used_ = 0, round_ = 0;
  std::atomic<size_t> n_blocks_{0}, bytes_{0}, allocations_{0};
};

// The largest round any of several arenas has completed: written when a call ends, read by the Resets of calls on other threads.
class RoundMark {
 public:
  size_t get() const { return bytes_.load(std::memory_order_relaxed); }
  void Raise(size_t round) {      // never decreases
    size_t cur = bytes_.load(std::memory_order_relaxed);
    while (cur < round && !bytes_.compare_exchange_weak(cur, round, std::memory_order_relaxed)) {}
  }

 private:
  std::atomic<size_t> bytes_{0};
};

}  // namespace rs

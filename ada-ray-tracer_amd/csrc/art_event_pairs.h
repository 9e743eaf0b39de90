// art_event_pairs.h -- pools of timed HIP event pairs (host only).  begin() records a pair's first event, the Timer it fills records the
// second, fold() reads the elapsed time of the pairs that have completed.  A folded, cancelled or released pair waits on the free list for
// the next begin().  Only fold(wait = true) waits for the GPU.  The events belong to the device that was current when they were created.
// The includer provides the HIP event calls (<hip/hip_runtime.h>; tests/event_pairs_check.cpp: counting stubs).
#pragma once
#include <cstdint>
#include <vector>

namespace art {
class EventPairs {
 public:
  struct Pair { hipEvent_t e0 = nullptr, e1 = nullptr; uint8_t tag = 0; };
  // A pair that was begun.  end() -- at the latest the destructor, so on every way out -- records its second event on begin()'s stream;
  // cancel() instead takes a pair that has not ended out of the count.  After either, both do nothing.
  class Timer {
   public:
    Timer() = default;
    Timer(const Timer&) = delete; Timer& operator=(const Timer&) = delete;
    ~Timer() { (void)end(); }
    hipError_t end() { EventPairs* const p = pool_; pool_ = nullptr; return p ? hipEventRecord(e1_, stream_) : hipSuccess; }
    void cancel() {
      if (!pool_) return;
      std::vector<Pair>& live = pool_->live_;
      size_t i = live.size();
      while (i > 0 && live[i - 1].e1 != e1_) --i;                             // (from the newest)
      if (i > 0) { pool_->free_.push_back(live[i - 1]); live.erase(live.begin() + (i - 1)); }
      pool_ = nullptr;
    }
   private:
    friend class EventPairs;
    EventPairs* pool_ = nullptr; hipEvent_t e1_ = nullptr; hipStream_t stream_ = nullptr;
  };
  // A pair from the free list (or a new one), its first event recorded on `stream`: the pair is live and `t` ends it.  On an error the
  // pair is back on the free list and `t` stays idle: a pair whose first event was not recorded never reaches the live list.
  hipError_t begin(Timer& t, hipStream_t stream, uint8_t tag = 0) {
    Pair p; hipError_t e = hipSuccess;
    if (!free_.empty()) { p = free_.back(); free_.pop_back(); }
    else if ((e = hipEventCreate(&p.e0)) != hipSuccess) return e;
    else if ((e = hipEventCreate(&p.e1)) != hipSuccess) { (void)hipEventDestroy(p.e0); return e; }
    p.tag = tag;
    if ((e = hipEventRecord(p.e0, stream)) != hipSuccess) { free_.push_back(p); return e; }
    live_.push_back(p);
    t.pool_ = this; t.e1_ = p.e1; t.stream_ = stream;
    return hipSuccess;
  }
  // Completed pairs -> each(ms, tag), and on to the free list.  wait: every pair is waited for (a caller whose stream is idle takes all
  // of them); the first error is returned, and that pair and those after it stay live.  Else a pair still in flight (or in error) stays
  // live and hipSuccess is returned, so that a host which never synchronises keeps a list as long as its work in flight.
  template <typename Each>
  hipError_t fold(bool wait, Each each) {
    size_t kept = 0; hipError_t rc = hipSuccess;
    for (const Pair p : live_) {
      float ms = 0.0f;
      hipError_t e = rc != hipSuccess ? hipErrorNotReady : (wait ? hipEventSynchronize(p.e1) : hipEventQuery(p.e1));
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, p.e0, p.e1);
      if (e == hipSuccess) { each(ms, p.tag); free_.push_back(p); continue; }
      if (wait && rc == hipSuccess) rc = e;
      live_[kept++] = p;
    }
    live_.resize(kept);
    (void)hipGetLastError();                                                 // (hipErrorNotReady of a pair still in flight)
    return rc;
  }
  void release() { free_.insert(free_.end(), live_.begin(), live_.end()); live_.clear(); }      // what is live will not be counted
  void destroy() { release(); for (const Pair& p : free_) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); } free_.clear(); }      // shutdown
  size_t live() const { return live_.size(); }
  size_t idle() const { return free_.size(); }
 private:
  std::vector<Pair> live_, free_;      // begun and not yet folded | ready for reuse
};
}  // namespace art

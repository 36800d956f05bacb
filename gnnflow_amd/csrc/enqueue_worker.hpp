// The enqueue threads that issue every asynchronous launch chain, and the tickets the C ABI
// hands out for their jobs.  Private to csrc/; the workers themselves live in enqueue_worker.hip.
#pragma once

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <string>

#include "common.hpp"

namespace gf {

// Enqueue worker: issuing the ~25 launches of one step costs more host time (~3 us per
// launch) than the kernels take on the GPU at batch 600, so asynchronous submissions hand
// the work to this single thread (one issuer: no runtime-lock convoy between threads) and
// return; the caller overlaps its own host work (Python, building the next batch) and
// later waits for the *enqueue* to have happened (stream order covers the execution).
class EnqueueWorker {
 public:
  using Job = std::function<void()>;
  // lane 0: feature fetches, lane 1: sampling.  Two issuers by default: the sampling launches
  // (side stream) and the fetch launches (caller's stream) of a pipelined step go to different
  // HIP queues, and one thread issuing all 8 is the step's bottleneck whenever the host is
  // busy; GNNFLOW_ENQUEUE_LANES=1 puts both on one thread.
  static EnqueueWorker& get(int lane = 0);
  uint64_t submit(Job&& job) {
    bool wake;
    uint64_t ticket;
    {
      std::lock_guard<std::mutex> lk(mu_);
      q_.push_back(std::move(job));
      ticket = ++submitted_;
      wake = sleeping_;
    }
    pending_.fetch_add(1, std::memory_order_release);
    if (wake) cv_job_.notify_one();   // a futex wake costs microseconds: only when needed
    return ticket;
  }
  // status of the submission `ticket` — its own, not an earlier job's — once it has been
  // enqueued
  int wait(uint64_t ticket, std::string* err) {
    // the enqueue usually finishes within microseconds: poll before sleeping on the condvar
    for (int i = 0; i < 20000 && done_.load(std::memory_order_acquire) < ticket; ++i)
      __builtin_ia32_pause();
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return completed_ >= ticket; });
    auto it = failed_.find(ticket);
    if (it == failed_.end()) return GF_OK;
    const int rc = it->second.first;
    *err = std::move(it->second.second);
    failed_.erase(it);
    return rc;
  }

 private:
  EnqueueWorker();
  void run();
  std::mutex mu_;
  std::condition_variable cv_job_, cv_done_;
  std::deque<Job> q_;
  uint64_t submitted_ = 0, completed_ = 0;
  bool sleeping_ = false;                 // worker is (about to be) blocked on cv_job_
  std::atomic<uint64_t> pending_{0};      // jobs queued and not yet taken
  std::atomic<uint64_t> done_{0};         // == completed_, readable without the mutex
  std::map<uint64_t, std::pair<int, std::string>> failed_;   // ticket -> status of that job

 public:
  double busy_us_ = 0;   // time spent issuing work (diagnostics)
  void stats(double* busy_us, uint64_t* jobs) {
    std::unique_lock<std::mutex> lk(mu_);
    *busy_us = busy_us_;
    *jobs = completed_;
  }
};

// The enqueue thread that issues EVERYTHING with a collective in it — the partitioned sampler's
// chains and the pull rounds of sharded features: one thread, one order of collectives over all
// communicators, the same on every rank: the fetch lane's thread (two issuing threads slow each
// other down).
constexpr int kCollectiveLane = 0;

// A ticket names a job of one lane: the lane's own sequence number (EnqueueWorker::submit, from
// 1) with the lane marked in the two top bits — bit 63: lane 0 (fetches, collectives), bit 62:
// lane 2 (the second sampling issuer), neither: lane 1.  0 is no ticket.
inline uint64_t make_ticket(int lane, uint64_t seq) {
  return seq | (lane == 0 ? 1ull << 63 : lane == 2 ? 1ull << 62 : 0ull);
}
inline void split_ticket(uint64_t ticket, int* lane, uint64_t* seq) {
  *lane = (ticket >> 63) ? 0 : ((ticket >> 62) & 1) ? 2 : 1;
  *seq = ticket & ~(3ull << 62);
}
// waits until the ticket's lane has run the job; a failed job's message goes to gf_last_error()
int wait_ticket(uint64_t ticket);

}  // namespace gf

// The enqueue workers (one per lane per process, never destroyed) and gf_worker_stats.
#include "enqueue_worker.hpp"

#include <chrono>
#include <thread>

namespace gf {

EnqueueWorker& EnqueueWorker::get(int lane) {
  static const bool two = [] {
    const char* v = std::getenv("GNNFLOW_ENQUEUE_LANES");
    return !(v && std::atoi(v) == 1);
  }();
  static EnqueueWorker* w0 = new EnqueueWorker();   // intentionally leaked: no exit-order issues
  if (lane == 0 || !two) return *w0;
  static EnqueueWorker* w1 = new EnqueueWorker();
  if (lane != 2) return *w1;
  // lane 2: a second sampling issuer (gf_sampler_set_enqueue_lane) — a sample's four launches +
  // event cost 19 us of issuing time, which ONE thread serving both lanes of a sampling-only
  // loop spends per step: that loop runs at the issuer's pace, not at the GPU's
  static EnqueueWorker* w2 = new EnqueueWorker();
  return *w2;
}

EnqueueWorker::EnqueueWorker() { std::thread(&EnqueueWorker::run, this).detach(); }

void EnqueueWorker::run() {
  for (;;) {
    Job job;
    // In a running pipeline the next job arrives within tens of microseconds: poll for it
    // (bounded, ~100 us) before sleeping, so that the submitter does not pay a futex wake
    // and this thread does not pay the wake-up latency.
    // (GNNFLOW_ENQUEUE_SPIN_US=0 turns the polling off: one busy thread less per lane when
    // many ranks share few cores.)
    static const long spin_us = [] {
      const char* v = std::getenv("GNNFLOW_ENQUEUE_SPIN_US");
      return v ? std::atol(v) : 100L;
    }();
    if (spin_us > 0) {
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; pending_.load(std::memory_order_acquire) == 0; ++i) {
        __builtin_ia32_pause();
        if ((i & 255) == 255 &&
            std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) break;
      }
    }
    {
      std::unique_lock<std::mutex> lk(mu_);
      if (q_.empty()) {
        sleeping_ = true;
        cv_job_.wait(lk, [&] { return !q_.empty(); });
        sleeping_ = false;
      }
      job = std::move(q_.front());
      q_.pop_front();
    }
    pending_.fetch_sub(1, std::memory_order_relaxed);
    int rc = GF_OK;
    std::string msg;
    const auto t0 = std::chrono::steady_clock::now();
    try {
      job();
    } catch (const Error& e) {
      rc = e.code; msg = e.what();
    } catch (const std::exception& e) {
      rc = GF_ERR_INVALID_ARGUMENT; msg = e.what();
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(mu_);
    busy_us_ += std::chrono::duration<double, std::micro>(t1 - t0).count();
    ++completed_;
    done_.store(completed_, std::memory_order_release);
    if (rc != GF_OK) {
      failed_[completed_] = std::make_pair(rc, msg);   // jobs complete in ticket order
      while (failed_.size() > 64) failed_.erase(failed_.begin());   // never waited for
    }
    cv_done_.notify_all();
  }
}

int wait_ticket(uint64_t ticket) {
  int lane;
  uint64_t seq;
  split_ticket(ticket, &lane, &seq);
  std::string err;
  const int rc = EnqueueWorker::get(lane).wait(seq, &err);
  if (rc != GF_OK) set_last_error(err);
  return rc;
}

}  // namespace gf

extern "C" int gf_worker_stats(double* busy_us, uint64_t* jobs) {
  return gf::guarded([&] {
    GF_REQUIRE(busy_us && jobs, "gf_worker_stats: null output");
    gf::EnqueueWorker::get(0).stats(busy_us, jobs);
    double b1 = 0;
    uint64_t j1 = 0;
    if (&gf::EnqueueWorker::get(1) != &gf::EnqueueWorker::get(0)) {
      gf::EnqueueWorker::get(1).stats(&b1, &j1);
      double b2 = 0;
      uint64_t j2 = 0;
      gf::EnqueueWorker::get(2).stats(&b2, &j2);
      if (std::getenv("GNNFLOW_WORKER_STATS"))
        std::fprintf(stderr,
                     "[worker] lane0 %.0f us / %llu jobs, lane1 %.0f us / %llu jobs, lane2 %.0f us / %llu jobs\n",
                     *busy_us, (unsigned long long)*jobs, b1, (unsigned long long)j1, b2, (unsigned long long)j2);
      *busy_us += b1 + b2;
      *jobs += j1 + j2;
    }
  });
}

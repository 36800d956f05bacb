// Stand-alone check of gnnflow_amd/csrc/enqueue_worker.{hpp,hip} (tests/test_enqueue_worker.py
// builds it with ThreadSanitizer and runs it): no HIP call, no GPU.  Exits non-zero on the first
// failed check.
#include <cstdio>
#include <set>
#include <thread>
#include <vector>

#include "enqueue_worker.hpp"

namespace gf {
static std::string g_error;   // what the library keeps per thread (capi.hip)
void set_last_error(const std::string& msg) { g_error = msg; }
}  // namespace gf

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

using gf::EnqueueWorker;

static uint64_t g_submitted = 0;   // over all lanes, for gf_worker_stats

// 1 000 jobs of one thread run in ticket order, and wait(k) returns only after job k ran
static void test_order() {
  EnqueueWorker& w = EnqueueWorker::get(1);
  const int n = 1000;
  std::vector<int> order;            // written by the worker, read after the last wait
  std::atomic<int> ran{0};
  std::vector<uint64_t> tickets(n);
  for (int k = 0; k < n; ++k)
    tickets[k] = w.submit([&order, &ran, k] { order.push_back(k); ran.fetch_add(1); });
  g_submitted += n;
  std::string err;
  for (int k = 0; k < n; ++k) {
    CHECK(tickets[k] == tickets[0] + static_cast<uint64_t>(k));
    CHECK(w.wait(tickets[k], &err) == GF_OK);
    CHECK(ran.load() >= k + 1);
  }
  CHECK(static_cast<int>(order.size()) == n);
  for (int k = 0; k < n; ++k) CHECK(order[k] == k);
}

// a failing job hands its code and text to the wait of ITS ticket, not to its neighbours'
static void test_error_goes_to_its_ticket() {
  EnqueueWorker& w = EnqueueWorker::get(1);
  const uint64_t a = w.submit([] {});
  const uint64_t b = w.submit([] { throw gf::Error(GF_ERR_OUT_OF_MEMORY, "boom 7"); });
  const uint64_t c = w.submit([] {});
  const uint64_t d = w.submit([] { throw std::runtime_error("plain"); });
  g_submitted += 4;
  std::string err;
  CHECK(w.wait(c, &err) == GF_OK && err.empty());
  CHECK(w.wait(a, &err) == GF_OK && err.empty());
  CHECK(w.wait(b, &err) == GF_ERR_OUT_OF_MEMORY && err == "boom 7");
  CHECK(w.wait(d, &err) == GF_ERR_INVALID_ARGUMENT && err == "plain");
  err.clear();
  CHECK(w.wait(b, &err) == GF_OK && err.empty());   // a status is handed out once
}

// statuses nobody waits for: the newest 64 are kept, and a later job still gets its own
static void test_unwaited_failures_are_capped() {
  EnqueueWorker& w = EnqueueWorker::get(2);
  const int n = 100;
  std::vector<uint64_t> t(n);
  for (int i = 0; i < n; ++i)
    t[i] = w.submit([i] { throw gf::Error(GF_ERR_HIP, "f" + std::to_string(i)); });
  const uint64_t last = w.submit([] { throw gf::Error(GF_ERR_OUT_OF_MEMORY, "last"); });
  g_submitted += n + 1;
  std::string err;
  CHECK(w.wait(last, &err) == GF_ERR_OUT_OF_MEMORY && err == "last");
  // 101 failures, 64 kept: jobs 37..99 and `last`
  err.clear();
  CHECK(w.wait(t[0], &err) == GF_OK && err.empty());
  CHECK(w.wait(t[36], &err) == GF_OK && err.empty());
  CHECK(w.wait(t[37], &err) == GF_ERR_HIP && err == "f37");
  CHECK(w.wait(t[99], &err) == GF_ERR_HIP && err == "f99");
}

// two submitting threads: unique tickets, every job completes
static void test_two_submitters() {
  EnqueueWorker& w = EnqueueWorker::get(0);
  const int n = 500;
  std::atomic<int> ran{0};
  std::vector<uint64_t> tickets[2];
  auto submitter = [&](int who) {
    for (int k = 0; k < n; ++k) tickets[who].push_back(w.submit([&ran] { ran.fetch_add(1); }));
  };
  std::thread t0(submitter, 0), t1(submitter, 1);
  t0.join();
  t1.join();
  g_submitted += 2 * n;
  std::set<uint64_t> all(tickets[0].begin(), tickets[0].end());
  all.insert(tickets[1].begin(), tickets[1].end());
  CHECK(all.size() == static_cast<size_t>(2 * n));
  std::string err;
  for (uint64_t t : all) CHECK(w.wait(t, &err) == GF_OK);
  CHECK(ran.load() == 2 * n);
}

// (lane, sequence) -> ticket -> (lane, sequence), and wait_ticket finds the lane's worker
static void test_ticket_codec() {
  const uint64_t seqs[] = {1, 2, 12345, (1ull << 32) + 5, (1ull << 62) - 1};
  std::set<uint64_t> all;
  for (int lane = 0; lane < 3; ++lane)
    for (uint64_t seq : seqs) {
      const uint64_t t = gf::make_ticket(lane, seq);
      int l = -1;
      uint64_t s = 0;
      gf::split_ticket(t, &l, &s);
      CHECK(l == lane && s == seq && t != 0);
      all.insert(t);
    }
  CHECK(all.size() == 3 * sizeof(seqs) / sizeof(seqs[0]));
  for (int lane = 0; lane < 3; ++lane) {
    const std::string msg = "lane " + std::to_string(lane);
    const uint64_t ok = gf::make_ticket(lane, EnqueueWorker::get(lane).submit([] {}));
    const uint64_t bad = gf::make_ticket(
        lane, EnqueueWorker::get(lane).submit([msg] { throw gf::Error(GF_ERR_HIP, msg); }));
    g_submitted += 2;
    gf::g_error.clear();
    CHECK(gf::wait_ticket(ok) == GF_OK && gf::g_error.empty());
    CHECK(gf::wait_ticket(bad) == GF_ERR_HIP && gf::g_error == msg);
  }
}

int main() {
  test_order();
  test_error_goes_to_its_ticket();
  test_unwaited_failures_are_capped();
  test_two_submitters();
  test_ticket_codec();
  double busy_us = -1;
  uint64_t jobs = 0;
  CHECK(gf_worker_stats(&busy_us, &jobs) == GF_OK);
  CHECK(jobs == g_submitted && busy_us >= 0);
  std::printf("enqueue worker: %llu jobs, all checks passed\n", (unsigned long long)jobs);
  return 0;
}

// What edge_store.hip and edge_store_ingest.hip share and nobody else needs.
#pragma once

#include <algorithm>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

#include "edge_store.hpp"

namespace gf {

constexpr size_t kBlockSpace = 20;       // common.h:23-24 bytes per edge

// fn(begin, end) over [0, n) on up to 8 host threads; chunks of at least `grain` items, inline
// when one chunk covers everything.  Ingest is host-bound (gathers through a permutation), so
// the threads are what the 10^7-edge chunks of a graph build spend their time in.
template <typename F>
void parallel_for(size_t n, size_t grain, unsigned max_threads, F&& fn) {
  static const unsigned hw = std::max(1u, std::min(12u, std::thread::hardware_concurrency()));
  const size_t parts = std::min<size_t>(std::min(hw, std::max(1u, max_threads)),
                                        (n + grain - 1) / std::max<size_t>(grain, 1));
  if (parts <= 1) { fn(size_t(0), n); return; }
  std::vector<std::thread> th;
  std::exception_ptr err;
  std::mutex mu;
  const size_t step = (n + parts - 1) / parts;
  for (size_t p = 0; p < parts; ++p) {
    const size_t a = p * step, b = std::min(n, a + step);
    if (a >= b) break;
    th.emplace_back([&, a, b] {
      try { fn(a, b); } catch (...) { std::lock_guard<std::mutex> lk(mu); err = std::current_exception(); }
    });
  }
  for (auto& t : th) t.join();
  if (err) std::rethrow_exception(err);
}

template <typename F>
void parallel_for(size_t n, size_t grain, F&& fn) {
  parallel_for(n, grain, ~0u, std::forward<F>(fn));
}

inline uint64_t pow2_ceil(uint64_t n) {
  uint64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}
inline int log2_exact(uint64_t p) { return 63 - __builtin_clzll(p); }

// The device node-table entry of a vertex record (GraphView::table is an array of these).
inline NodeEntry node_entry(const NodeState& st) {
  NodeEntry e;
  e.start = st.seg_start + st.live_off;
  e.size = static_cast<uint32_t>(st.live_size);
  std::memcpy(&e.last_ts_bits, &st.last_ts, 4);
  return e;
}

}  // namespace gf

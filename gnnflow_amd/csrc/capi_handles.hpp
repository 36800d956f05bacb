// What the extern "C" units (capi*.hip) share: the structs behind the opaque handles of
// include/gnnflow_hip.h, the handle checks and two pointer conversions.  Private to csrc/.
#pragma once

#include <deque>
#include <memory>

#include <unistd.h>

#include "comm.hpp"
#include "common.hpp"
#include "edge_store.hpp"
#include "feature_cache.hpp"
#include "sampler.hpp"

struct gf_graph {
  gf::EdgeStore impl;
  template <typename... A> explicit gf_graph(A&&... a) : impl(std::forward<A>(a)...) {}
};
struct gf_sampler {
  gf::Sampler impl;
  std::deque<uint64_t> begin_tickets;   // 0 = begun synchronously
  int plain_lane = 1;   // enqueue thread of sample_begin_async (gf_sampler_set_enqueue_lane)
  template <typename... A> explicit gf_sampler(A&&... a) : impl(std::forward<A>(a)...) {}
};
struct gf_cache {
  gf::FeatureCache impl;
  template <typename... A> explicit gf_cache(A&&... a) : impl(std::forward<A>(a)...) {}
};
struct gf_comm {
  std::unique_ptr<gf::Exchange> owned;
  gf::Exchange& impl;
  gf::IpcExchange* ipc = nullptr;
  gf_comm(const uint8_t* id, int world, int rank, int device)
      : owned(new gf::RcclComm(id, world, rank, device)), impl(*owned) {}
  gf_comm(gf::IpcExchange* x) : owned(x), impl(*owned), ipc(x) {}
  gf_comm(gf::LoopbackExchange* x) : owned(x), impl(*owned), loopback(true) {}
  bool loopback = false;   // ranks are threads of this process: no shared enqueue thread
};
struct gf_pull_session {
  gf::PullSession impl;
  // over RCCL the round is issued by the enqueue thread that also issues the partitioned
  // sampler's chains: ONE global order of collectives over all communicators, on every rank
  bool ordered = false;
  gf_pull_session(gf::Exchange* ex, int device) : impl(ex, device) {}
};

namespace gf {
// A process forked from one that holds handles (multiprocessing's fork start method: a Manager
// server, a DataLoader worker) inherits the Python objects and may finalise them — its garbage
// collector runs their __del__.  The GPU state behind a handle belongs to the process that
// loaded the library: in any other process a destroy call is a no-op (the child's copy of the
// host memory goes with the process), it must never free the parent's device memory.
extern const pid_t g_load_pid;   // (capi.hip: set when the library is loaded, never later)
inline bool foreign_process() { return getpid() != g_load_pid; }
}  // namespace gf

using gf::guarded;

template <typename Handle> int destroy_handle(Handle* h) {   // every gf_*_destroy
  if (gf::foreign_process()) return GF_OK;
  return guarded([&] { delete h; });
}

#define GF_G(g) GF_REQUIRE((g) != nullptr, "null graph handle")
#define GF_S(s) GF_REQUIRE((s) != nullptr, "null sampler handle")
#define GF_C(c) GF_REQUIRE((c) != nullptr, "null cache handle")

inline hipStream_t as_stream(void* stream) { return static_cast<hipStream_t>(stream); }
// an optional cache handle (NULL: that kind of feature is not cached)
inline gf::FeatureCache* cache_or_null(gf_cache* c) { return c ? &c->impl : nullptr; }

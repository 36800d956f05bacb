// Event-based kernel time accounting: the state behind ProfileScope / profile_begin / profile_end
// (common.hpp) and the gf_profile_* entry points that read and reset it.
#include <atomic>
#include <mutex>

#include "common.hpp"

namespace gf {

namespace {
struct ProfileRecord { int slot; hipEvent_t start, stop; };
std::mutex g_prof_mu;
// read by the launching threads (caller + enqueue thread) without the mutex
std::atomic<unsigned> g_prof_mask{0};
std::atomic<unsigned> g_prof_stride{1};   // time every n-th interval of a slot
std::atomic<uint64_t> g_prof_seq[kProfSlots];
std::vector<hipEvent_t> g_prof_free;      // recycled events (creating one costs microseconds)
hipEvent_t take_event() {
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_free.empty()) { hipEvent_t e = g_prof_free.back(); g_prof_free.pop_back(); return e; }
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
std::vector<ProfileRecord> g_prof_pending;
double g_prof_ms[kProfSlots] = {0};
uint64_t g_prof_launches[kProfSlots] = {0};

void drain_profile_locked() {
  for (ProfileRecord& r : g_prof_pending) {
    float ms = 0;
    if (hipEventSynchronize(r.stop) == hipSuccess &&
        hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) {
      g_prof_ms[r.slot] += ms;
      g_prof_launches[r.slot]++;
    }
    g_prof_free.push_back(r.start);
    g_prof_free.push_back(r.stop);
  }
  g_prof_pending.clear();
}
}  // namespace

bool profile_enabled() { return g_prof_mask.load(std::memory_order_relaxed) != 0; }

ProfileScope::ProfileScope(int slot_, hipStream_t stream_) : slot(slot_), stream(stream_) {
  if (slot < 0) return;   // (the caller times the launch itself)
  if (!(g_prof_mask.load(std::memory_order_relaxed) & (1u << slot))) return;
  if (g_prof_seq[slot].fetch_add(1, std::memory_order_relaxed) %
          g_prof_stride.load(std::memory_order_relaxed) != 0) return;
  start = take_event();
  if (start) (void)hipEventRecord(start, stream);
}

ProfileScope::~ProfileScope() {
  if (!start) return;
  hipEvent_t stop = take_event();
  if (!stop) { (void)hipEventDestroy(start); return; }
  (void)hipEventRecord(stop, stream);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_pending.push_back({slot, start, stop});
}

bool profile_begin(int slot, hipEvent_t* start, hipEvent_t* stop) {
  if (!(g_prof_mask.load(std::memory_order_relaxed) & (1u << slot))) return false;
  if (g_prof_seq[slot].fetch_add(1, std::memory_order_relaxed) %
          g_prof_stride.load(std::memory_order_relaxed) != 0) return false;
  *start = take_event();
  *stop = take_event();
  if (*start && *stop) return true;
  if (*start) (void)hipEventDestroy(*start);
  if (*stop) (void)hipEventDestroy(*stop);
  return false;
}

void profile_end(int slot, hipEvent_t start, hipEvent_t stop) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_pending.push_back({slot, start, stop});
}

}  // namespace gf

extern "C" {

int gf_profile_enable(int mask) {
  std::lock_guard<std::mutex> lk(gf::g_prof_mu);
  gf::g_prof_mask = static_cast<unsigned>(mask);
  return GF_OK;
}
int gf_profile_reset(void) {
  std::lock_guard<std::mutex> lk(gf::g_prof_mu);
  gf::drain_profile_locked();
  for (int i = 0; i < gf::kProfSlots; ++i) {
    gf::g_prof_ms[i] = 0;
    gf::g_prof_launches[i] = 0;
    gf::g_prof_seq[i] = 0;
  }
  return GF_OK;
}
int gf_profile_launches(int which, uint64_t* launches) {
  return gf::guarded([&] {
    GF_REQUIRE(which >= 0 && which < gf::kProfSlots && launches, "gf_profile_launches: bad argument");
    std::lock_guard<std::mutex> lk(gf::g_prof_mu);
    *launches = gf::g_prof_seq[which];
  });
}
int gf_profile_set_stride(unsigned stride) {
  std::lock_guard<std::mutex> lk(gf::g_prof_mu);
  gf::g_prof_stride = stride ? stride : 1;
  return GF_OK;
}
int gf_profile_get(int which, double* total_ms, uint64_t* launches) {
  return gf::guarded([&] {
    GF_REQUIRE(which >= 0 && which < gf::kProfSlots, "gf_profile_get: bad slot");
    std::lock_guard<std::mutex> lk(gf::g_prof_mu);
    gf::drain_profile_locked();
    if (total_ms) *total_ms = gf::g_prof_ms[which];
    if (launches) *launches = gf::g_prof_launches[which];
  });
}

}  // extern "C"

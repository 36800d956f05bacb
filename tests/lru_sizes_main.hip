// Stand-alone check of the LRU buffer sizes in gnnflow_amd/csrc/feature_cache_ctx.hpp
// (tests/test_lru_sizes.py builds it for the host only and runs it): no HIP call, no GPU.
// lru_queue_cap(), lru_bit_tiles() and compact_layout() replaced expressions that used to be
// written out by hand in FeatureCache::init_queue, FeatureCache::resize,
// FeatureCache::compact_queue, FeatureCache::prepare and launch_lru_update; those expressions
// stand here literally as the expected values.  Exits non-zero on the first failed check.
#include <cstdio>

#include "feature_cache_ctx.hpp"

namespace gf {
void set_last_error(const std::string&) {}   // what the library keeps per thread (capi.hip)
}  // namespace gf

#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      std::fprintf(stderr, "%s:%d: capacity %zu: CHECK(%s) failed\n", __FILE__, __LINE__,    \
                   capacity, #cond);                                                         \
      std::exit(1);                                                                          \
    }                                                                                        \
  } while (0)

using namespace gf;

static void check_capacity(size_t capacity) {
  // the queue capacity rule, both forms (init_queue / resize)
  for (int form = 0; form < 2; ++form) {
    const bool queue_form_ = form != 0;
    const size_t capacity_ = capacity;
    const size_t queue_cap_ = queue_form_ ? capacity_ + capacity_ / 2 + 64 : capacity_;
    CHECK(lru_queue_cap(capacity, queue_form_) == queue_cap_);
  }
  const size_t queue_cap_ = capacity + capacity / 2 + 64;   // queue form from here on

  // the hit bitmap's tiles: the context fill's expression, then launch_lru_update's
  {
    const size_t bit_tiles = ((queue_cap_ + 64) / 32 + kBitTile - 1) / kBitTile + 1;
    CHECK(lru_bit_tiles(capacity) == bit_tiles);
  }
  {
    struct { uint32_t capacity; } c{static_cast<uint32_t>(capacity)};
    const size_t bit_tiles = ((size_t{c.capacity} * 3 / 2 + 128) / 32 + kBitTile - 1) / kBitTile + 1;
    CHECK(lru_bit_tiles(capacity) == bit_tiles);
  }
  // ... and they cover the bitmap words of every position below the largest tail
  CHECK(lru_bit_tiles(capacity) * kBitTile * 32 >= queue_cap_ + 64);
  CHECK(lru_bit_tiles(capacity) * kBitTile * sizeof(uint32_t) <= qbits_bytes(queue_cap_));

  const CompactLayout lay = compact_layout(queue_cap_);
  // the compaction scratch as compact_queue walked it
  {
    size_t p = 0;
    CHECK(lay.live_bits == p);
    p += align_up(((queue_cap_ + kRowTile - 1) / kRowTile + 1) * (kRowTile / 64) * 8, 256);
    CHECK(lay.tile_cnt == p);
    p += align_up(((queue_cap_ + kRowTile - 1) / kRowTile + 1) * 4, 256);
    CHECK(lay.group_sum == p);
    p += align_up((((queue_cap_ + kRowTile - 1) / kRowTile + 1 + kQGroup - 1) / kQGroup + 1) * 4, 256);
    CHECK(lay.state == p);
  }
  // ... and as init_queue / resize reserved it
  {
    const size_t tiles = (queue_cap_ + kRowTile - 1) / kRowTile + 1;
    const size_t groups = (tiles + kQGroup - 1) / kQGroup + 1;
    const size_t bytes = align_up(tiles * (kRowTile / 64) * 8, 256) + align_up(tiles * 4, 256) +
                         align_up(groups * 4, 256) + 256;
    CHECK(lay.bytes == bytes);
  }
  // the walk ends inside the reservation: the state block is its last 256 bytes, and the arrays
  // hold what a compaction of a full queue (tail = queue_cap) writes
  {
    const size_t tiles = (queue_cap_ + kRowTile - 1) / kRowTile;
    const size_t groups = (tiles + kQGroup - 1) / kQGroup;
    CHECK(lay.state + 256 == lay.bytes);
    CHECK(lay.tile_cnt - lay.live_bits >= tiles * (kRowTile / 64) * 8);
    CHECK(lay.group_sum - lay.tile_cnt >= tiles * 4);
    CHECK(lay.state - lay.group_sum >= groups * 4);
  }
}

int main() {
  const size_t group = size_t{kRowTile} * kQGroup;   // queue positions per group of list tiles
  const size_t capacities[] = {0,         1,     3,         4,       63,      64,      65,      199,
                               200,       340,   group - 1, group,   group + 1, 499999, 500000,
                               40000000};
  for (size_t capacity : capacities) check_capacity(capacity);
  // which form: from queue_min_capacity() slots on (0.5 M unless the environment says otherwise)
  if (!std::getenv("GNNFLOW_LRU_QUEUE_MIN_CAPACITY")) {
    const size_t capacity = size_t{1} << 19;
    CHECK(queue_min_capacity() == capacity);
  }
  std::printf("all checks passed\n");
  return 0;
}

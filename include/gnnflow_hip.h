/*
 * gnnflow_hip.h — C ABI of the MI355X-native GNNFlow hot path
 * (temporal edge store -> TemporalSampler.sample() -> feature gather / LRU cache).
 *
 * This is the drop-in boundary: every entry point below replaces one method of
 * the reference's pybind11 module `libgnnflow` (gnnflow/csrc/api.cc) or one step
 * of the Python feature cache (gnnflow/cache/cache.py, lru_cache.py).  Signatures
 * use only plain pointers and sizes — no torch / pybind / STL types — so the same
 * library binds from ctypes (gnnflow_amd/_capi.py), from pybind11
 * (gnnflow_amd/csrc/pybind_libgnnflow.cpp builds a module named `libgnnflow` with
 * the reference's class/method names) or from any other FFI.
 *
 * Conventions
 *   - every function returns GF_OK (0) or a GF_ERR_* code; gf_last_error() gives
 *     the message for the calling thread (the reference CHECK()/abort()s instead,
 *     gnnflow/csrc/logging.h:9-46 — an error code is strictly friendlier).
 *   - "host" pointers are ordinary CPU memory; "device" pointers are HBM
 *     addresses on the graph's device.  `stream` is a hipStream_t passed as
 *     void* (NULL = the null stream).
 *   - node / edge ids are int64, timestamps float32 (gnnflow/csrc/common.h:13-15).
 *   - not thread-safe per handle (one in-flight call per graph / sampler / cache,
 *     as in the reference: gnnflow/csrc/temporal_sampler.h:73-80); different
 *     handles may be used from different threads.  Calls do not hold the GIL.
 */
#ifndef GNNFLOW_HIP_H_
#define GNNFLOW_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_API __attribute__((visibility("default")))

/* ---- status ----------------------------------------------------------------- */
enum {
  GF_OK = 0,
  GF_ERR_INVALID_ARGUMENT = 1,
  GF_ERR_TIMESTAMP_ORDER = 2, /* add_edges: edges older than the node's newest edge
                                 (reference: CHECK_LE at gnnflow/csrc/utils.cu:42-43) */
  GF_ERR_OUT_OF_MEMORY = 3,   /* maximum_pool_size exceeded / hipMalloc failed */
  GF_ERR_HIP = 4,             /* a HIP runtime call failed */
  GF_ERR_IO = 5
};

/* gnnflow/csrc/api.cc:27-39 enum values, same order */
enum { GF_INSERTION_POLICY_INSERT = 0, GF_INSERTION_POLICY_REPLACE = 1 };
enum { GF_SAMPLING_POLICY_RECENT = 0, GF_SAMPLING_POLICY_UNIFORM = 1 };
enum { GF_MEM_CUDA = 0, GF_MEM_UNIFIED = 1, GF_MEM_PINNED = 2, GF_MEM_SHARED = 3 };

GF_API const char* gf_last_error(void);
GF_API const char* gf_version(void);

/* ---- DynamicGraph: gnnflow/csrc/api.cc:41-85, dynamic_graph.h:26-170 --------- */
typedef struct gf_graph gf_graph;

/* _DynamicGraph.__init__ (api.cc:42-47; `minium_block_size` spelling is the
 * reference's).  All four memory resource types place the edge store in HBM on
 * `device` (288 GB per MI355X makes the managed / pinned spill modes moot). */
GF_API int gf_graph_create(gf_graph** out, size_t initial_pool_size,
                           size_t maximum_pool_size, int mem_resource_type,
                           size_t minium_block_size, size_t blocks_to_preallocate,
                           int insertion_policy, int device, int adaptive_block_size);
GF_API int gf_graph_destroy(gf_graph* g);

/* _DynamicGraph.add_edges (api.cc:48-50 -> DynamicGraph::AddEdges,
 * dynamic_graph.cu:77-138).  Four host arrays of length n, any order inside the
 * batch; grouped by source and stable-sorted by timestamp on ingest. */
GF_API int gf_graph_add_edges(gf_graph* g, const int64_t* src, const int64_t* dst,
                              const float* ts, const int64_t* eids, size_t n);

/* _DynamicGraph.offload_old_blocks (api.cc:51-52 -> dynamic_graph.cu:382-411):
 * drops every whole logical block whose end timestamp < `timestamp`;
 * to_file != 0 also writes temporal_block_<node>-<k>.bin
 * (temporal_block_allocator.cu:182-221 format). */
GF_API int gf_graph_offload_old_blocks(gf_graph* g, float timestamp, int to_file,
                                       size_t* num_blocks);

/* api.cc:53-55,70-71 */
GF_API int gf_graph_num_vertices(const gf_graph* g, size_t* out);
GF_API int gf_graph_num_source_vertices(const gf_graph* g, size_t* out);
GF_API int gf_graph_num_edges(const gf_graph* g, size_t* out);
GF_API int gf_graph_max_vertex_id(const gf_graph* g, int64_t* out);
/* *out = 1 when every node id and every edge id inserted so far is in [0, 2^32 - 2]: the shared
 * chains of the partitioned sampler may then carry 12-byte reply slots (narrow_ids below).  No
 * reference counterpart. */
GF_API int gf_graph_ids_fit_u32(const gf_graph* g, int* out);
/* api.cc:56-59 out_degree(list) */
GF_API int gf_graph_out_degree(const gf_graph* g, const int64_t* nodes, size_t n,
                               size_t* out);
/* api.cc:60-69 nodes() / src_nodes() / edges(): pass out = NULL to query *count */
GF_API int gf_graph_nodes(const gf_graph* g, int64_t* out, size_t capacity, size_t* count);
GF_API int gf_graph_src_nodes(const gf_graph* g, int64_t* out, size_t capacity, size_t* count);
GF_API int gf_graph_edges(const gf_graph* g, int64_t* out, size_t capacity, size_t* count);
/* api.cc:72-78 get_temporal_neighbors(node) -> newest first; out arrays may be
 * NULL to query *count */
GF_API int gf_graph_get_temporal_neighbors(const gf_graph* g, int64_t node, int64_t* dst,
                                           float* ts, int64_t* eids, size_t capacity,
                                           size_t* count);
/* api.cc:79-85 */
GF_API int gf_graph_avg_linked_list_length(const gf_graph* g, float* out);
GF_API int gf_graph_memory_usage(const gf_graph* g, float* out);
GF_API int gf_graph_metadata_memory_usage(const gf_graph* g, float* out);
GF_API int gf_graph_device(const gf_graph* g, int* out);

/* ---- TemporalSampler: api.cc:111-120, temporal_sampler.h:19-38 -------------- */
typedef struct gf_sampler gf_sampler;

/* _TemporalSampler.__init__ (api.cc:112-116).  The sampler keeps a pointer to
 * the graph: destroy the sampler first (the reference holds `const DynamicGraph&`,
 * temporal_sampler.h:62). */
GF_API int gf_sampler_create(gf_sampler** out, gf_graph* g, const uint32_t* fanouts,
                             size_t num_layers, int sampling_policy,
                             uint32_t num_snapshots, float snapshot_time_window,
                             int prop_time, uint64_t seed);
GF_API int gf_sampler_destroy(gf_sampler* s);

/* One (layer, snapshot) SamplingResult (gnnflow/csrc/common.h:51-60).  Pointers
 * address the caller's output buffer; counts are valid after the call returns. */
typedef struct gf_block {
  int64_t* all_nodes;       /* [num_src_nodes] roots ++ sampled neighbours */
  float* all_timestamps;    /* [num_src_nodes] */
  float* delta_timestamps;  /* [num_edges] root ts - edge ts */
  int64_t* eids;            /* [num_edges] */
  int64_t* row;             /* [num_edges] root index of each edge (non-decreasing) */
  int64_t* col;             /* [num_edges] num_dst_nodes .. num_src_nodes-1 */
  uint64_t num_dst_nodes;   /* R */
  uint64_t num_src_nodes;   /* R + S */
  uint64_t num_edges;       /* S */
} gf_block;

/* Worst-case byte size of the output buffer of gf_sampler_sample for
 * `num_roots` roots (all layers x snapshots, every slot valid). */
GF_API int gf_sampler_output_bytes(const gf_sampler* s, size_t num_roots, size_t* bytes);

/* _TemporalSampler.sample (api.cc:117-118 -> TemporalSampler::Sample,
 * temporal_sampler.cu:279-305), device resident: roots / timestamps and the
 * output buffer are device pointers; all layers and snapshots are sampled without
 * leaving HBM (layer l+1 roots = layer l all_nodes / all_timestamps).
 * blocks: host array [num_layers * num_snapshots], index layer*num_snapshots+snap
 * (the reference's [layer][snapshot] order, before Python reverses the layers).
 * Synchronises `stream` once at the end to read the per-block sizes. */
GF_API int gf_sampler_sample(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                             size_t num_roots, void* d_out, size_t out_bytes,
                             gf_block* blocks, void* stream);

/* The same call split in two, for software pipelining (the reference overlaps the next
 * batch's sample() with training on a Python thread, scripts/offline_edge_prediction.py:
 * 343-346): begin enqueues everything on `stream` and returns without waiting; end waits
 * for that work and fills `blocks`.  One sample may be in flight per sampler. */
GF_API int gf_sampler_sample_begin(gf_sampler* s, const int64_t* d_roots,
                                   const float* d_root_ts, size_t num_roots, void* d_out,
                                   size_t out_bytes, void* stream);
GF_API int gf_sampler_sample_end(gf_sampler* s, gf_block* blocks);
/* Uniform sampling draws philox4x32-10(seed; slot, call) (include/gnnflow_rng.h), `call` = the
 * number of sample_layer invocations of the sampler so far — one per layer and snapshot of a
 * sample() (the reference draws from per-thread curand states, sampling_kernels.cu:109-273).
 * gf_sampler_call_counter reads it; gf_sampler_set_call_counter sets the number the NEXT begun
 * sample starts from (through_enqueue_thread != 0: ordered with gf_sampler_sample_begin_async).
 * Clones of one sampler over the same graph can then take turns — sampling lanes — and still
 * reproduce the one sampler's stream of draws: sample j starts at j x layers x snapshots. */
GF_API int gf_sampler_call_counter(const gf_sampler* s, uint64_t* out);
GF_API int gf_sampler_set_call_counter(gf_sampler* s, uint64_t value, int through_enqueue_thread);
/* As gf_sampler_sample_begin, but the launches are issued by the library's enqueue thread
 * (the one gf_cache_fetch_blocks_async uses, in submission order); gf_sampler_sample_end
 * waits for it.  The inputs must stay alive until gf_sampler_sample_end returns. */
GF_API int gf_sampler_sample_begin_async(gf_sampler* s, const int64_t* d_roots,
                                         const float* d_root_ts, size_t num_roots,
                                         void* d_out, size_t out_bytes, void* stream);
/* Which of the library's two sampling enqueue threads issues this sampler's
 * gf_sampler_sample_begin_async launches (1: the default, 2: the second one).  A sampling-only
 * pipeline whose lanes are a sampler and its clone puts the clone on 2: the four launches + event
 * of a sample cost ~19 us of issuing time, and one thread serving both lanes spends that per
 * sample — the loop then runs at the issuer's pace, not the GPU's.  No sample may be in flight.
 * (The reference samples on the caller's thread: gnnflow/temporal_sampler.py:149-165.) */
GF_API int gf_sampler_set_enqueue_lane(gf_sampler* s, int lane);

/* _TemporalSampler.sample_layer (api.cc:119-120 -> TemporalSampler::SampleLayer,
 * temporal_sampler.cu:97-277), device resident; *bytes variant sizes the buffer. */
GF_API int gf_sampler_layer_output_bytes(const gf_sampler* s, size_t num_roots,
                                         uint32_t layer, size_t* bytes);
GF_API int gf_sampler_sample_layer(gf_sampler* s, const int64_t* d_roots,
                                   const float* d_root_ts, size_t num_roots,
                                   uint32_t layer, uint32_t snapshot, void* d_out,
                                   size_t out_bytes, gf_block* block, void* stream);

/* Host-vector forms with the reference's exact calling convention (host arrays
 * in, freshly allocated host arrays out; api.cc:17-24 copies into numpy the same
 * way).  Results are released with gf_host_blocks_free. */
GF_API int gf_sampler_sample_host(gf_sampler* s, const int64_t* nodes, const float* ts,
                                  size_t num_roots, gf_block* blocks);
GF_API int gf_sampler_sample_layer_host(gf_sampler* s, const int64_t* nodes,
                                        const float* ts, size_t num_roots, uint32_t layer,
                                        uint32_t snapshot, gf_block* block);
GF_API void gf_host_blocks_free(gf_block* blocks, size_t n);

/* ---- feature gather + LRU cache: gnnflow/cache/cache.py, lru_cache.py -------- */
typedef struct gf_cache gf_cache;
typedef struct gf_comm gf_comm;   /* RCCL communicator of the partitioned path, below */

/* One cache "kind" (node or edge) of Cache.__init__ (cache.py:82-134) +
 * LRUCache.__init__ (lru_cache.py:56-61): `capacity` rows of `dim` float32 in
 * HBM, id -> slot map over `num_ids`, slot -> id table, LRU stamps.
 * d_feats: the full feature table [num_ids, dim] float32 — a device pointer, or
 * device-accessible pinned host memory (misses are then read over PCIe). */
GF_API int gf_cache_create(gf_cache** out, size_t num_ids, size_t capacity, size_t dim,
                           const float* d_feats, int device);
GF_API int gf_cache_destroy(gf_cache* c);
/* Replacement policy: LRU (lru_cache.py, the default), LFU (lfu_cache.py:
 * a hit adds 1 to the slot's use count, the k smallest counts are evicted, a new entry
 * starts at 1) or FIFO (fifo_cache.py: slots are refilled in rotation, hits change nothing).
 * Set before the first fetch. */
enum { GF_CACHE_LRU = 0, GF_CACHE_LFU = 1, GF_CACHE_FIFO = 2 };
GF_API int gf_cache_set_policy(gf_cache* c, int policy);
/* FIFOCache.reset (fifo_cache.py:70-75): forget the replacement order (next refill starts
 * at slot 0 again) but keep the cached rows. */
GF_API int gf_cache_reset_order(gf_cache* c, void* stream);
/* GNNLabStaticCache.init_cache (gnnlab_static_cache.py:87-168): slot i caches d_ids[i]
 * (n <= capacity, device array); used with update = 0 fetches. */
GF_API int gf_cache_init_ids(gf_cache* c, const int64_t* d_ids, size_t n, void* stream);
/* Cache.init_cache / LRUCache.reset (cache.py:157-195, lru_cache.py:74-105):
 * slots 0..capacity-1 hold ids 0..capacity-1, LRU state zeroed. */
GF_API int gf_cache_init(gf_cache* c, void* stream);
/* Cache.resize (cache.py:197-221) */
GF_API int gf_cache_resize(gf_cache* c, size_t new_num_ids, size_t new_capacity,
                           const float* d_feats, void* stream);

/* One block of Cache.fetch_feature (cache.py:255-400): out[i,:] = feats[ids[i],:]
 * served from the cache on a hit and from d_feats on a miss, then (update != 0
 * and at least one miss) the LRU replacement of lru_cache.py:121-201.
 * d_ids [n] int64 device, d_out [n, dim] float32 device.  d_stats (device,
 * 16 x uint32, zeroed by the caller, may be NULL) accumulates the block's hit count in
 * the even words (8 shards; hits = sum of d_stats[0,2,..,14]) and n in d_stats[1]; no
 * host synchronisation. */
GF_API int gf_cache_fetch(gf_cache* c, const int64_t* d_ids, size_t n, float* d_out,
                          int update, uint32_t* d_stats, void* stream);

/* Sharded feature tables (Cache(distributed=True): cache.py:293-312,351-388 pull the missed
 * rows from the owning machine's KVStore, gnnflow/distributed/kvstore.py:70-126; here the
 * owners are the GPUs of the node and the pull is the caller's all-to-all-v):
 *   gf_cache_probe        d_slot[i] = slot of d_ids[i] (>= 0), -1 not cached, -2 out of range
 *   gf_cache_fetch_pulled as gf_cache_fetch, but the row of a missed id i is
 *                         d_miss_rows[d_miss_index[i]] (the pulled rows), not d_feats[id]
 *   gf_cache_init_rows    slot i caches d_ids[i] with row d_rows[i] (init_cache when the first
 *                         `capacity` rows live on other GPUs, cache.py:175-195) */
GF_API int gf_cache_probe(gf_cache* c, const int64_t* d_ids, size_t n, int32_t* d_slot,
                          void* stream);
GF_API int gf_cache_fetch_pulled(gf_cache* c, const int64_t* d_ids, size_t n, float* d_out,
                                 int update, uint32_t* d_stats, const float* d_miss_rows,
                                 const uint32_t* d_miss_index, void* stream);
GF_API int gf_cache_init_rows(gf_cache* c, const int64_t* d_ids, size_t n, const float* d_rows,
                              void* stream);

/* The same pull planned natively, for all contexts of a fetch round at once (a node block, an
 * edge block, cache-free target rows — up to 4), without torch ops and with ONE host
 * synchronisation per round (reference: cache.py:288-313,351-388 probe / unique / pull;
 * kvstore.py:285-339).  owner(key) = splitmix64(key) mod world_size; the key of row i is
 * d_key_base[d_key_index[i]] (edge rows: the edge's source node = the block's root of that
 * edge), d_key_base[i], or the id itself when d_key_base is NULL.
 *   gf_pull_count    settles the claims of the missed ids (lowest row wins, the claim the
 *                    fetch's own gather makes) and counts the rows that travel — the winners,
 *                    and every row of a cache-free context — per owner:
 *                    d_counts[ctx * world_size + owner] (uint32, zeroed by the call);
 *   — the caller exchanges the counts and reads own and received counts back: the round's one
 *     host synchronisation (they are the split sizes of the two exchanges below) —
 *   gf_pull_scatter  writes the travelling ids compact and owner-major (offsets = the exclusive
 *                    prefix of gf_pull_count's d_counts) into d_send_ids and d_req_pos[row] =
 *                    the position of the row's id = the index of its row among the pulled rows,
 *                    which arrive in the same order (d_cursor: [n * world_size] scratch);
 *   — ids out (all-to-all-v), gf_gather_rows_indexed on the owner, rows back —
 *   gf_cache_fetch_blocks_pulled   the fetch round with the pulled rows standing in for the
 *                    local table; a missed row finds its row through the settled claim. */
typedef struct gf_pull_desc {
  gf_cache* cache;             /* NULL: cache-free rows (every row travels) */
  const int64_t* d_ids;
  size_t n;
  const int64_t* d_key_base;   /* NULL: the id is the key */
  const int64_t* d_key_index;  /* NULL: key = d_key_base[i] */
  size_t num_ids;              /* id space of a cache-free context (a cache knows its own) */
  int64_t* d_send_ids;         /* [n] gf_pull_scatter */
  uint32_t* d_req_pos;         /* [n] gf_pull_scatter */
} gf_pull_desc;
GF_API int gf_pull_count(const gf_pull_desc* descs, size_t n, int world_size, uint32_t* d_counts,
                         int device, void* stream);
GF_API int gf_pull_scatter(const gf_pull_desc* descs, size_t n, int world_size,
                           uint32_t* d_counts, uint32_t* d_cursor, int device, void* stream);
/* the owner's side of a pull: d_out[i,:] = d_rows[d_index[d_ids[i]],:] (d_index: global id ->
 * local row of this shard, int32, -1 = not owned: *d_flag is set to 1 and row 0 is served) */
GF_API int gf_gather_rows_indexed(const float* d_rows, size_t num_local_rows, size_t dim,
                                  const int32_t* d_index, size_t num_ids, const int64_t* d_ids,
                                  size_t n, float* d_out, uint32_t* d_flag, int device,
                                  void* stream);
typedef struct gf_fetch_pulled_desc {
  int kind;                    /* 0: node block, 1: edge block (executed in array order) */
  int update;
  const int64_t* d_ids;
  size_t n;
  float* d_out;
  uint32_t* d_stats;
  const float* d_pulled_rows;  /* the rows that came back for this context */
  const uint32_t* d_req_pos;   /* gf_pull_scatter's */
} gf_fetch_pulled_desc;
GF_API int gf_cache_fetch_blocks_pulled(gf_cache* node_cache, gf_cache* edge_cache,
                                        const gf_fetch_pulled_desc* descs, size_t n,
                                        void* stream);

/* The whole round in ONE call (the stages above + the exchanges through `comm`, which may be
 * NULL with one rank): per context the pull description, this rank's shard of the context's
 * table (rows + global id -> local row index) and where the fetched rows go.  kind 2 = cache-free
 * (target edge features): d_out[i,:] = the pulled row of d_ids[i].  `flag` travels to every rank
 * in the count exchange and *any_flag = OR over all ranks (Cache uses it to agree on the prefix
 * alias).  rows_pulled / bytes_sent [n]: per context, rows fetched from OTHER ranks and bytes
 * this rank put on the wire (ids out + rows served).  One host synchronisation. */
typedef struct gf_pull_ctx {
  gf_pull_desc pull;           /* cache, d_send_ids, d_req_pos are ignored (the session's own) */
  const float* d_shard_rows;   /* [shard_rows, dim] */
  size_t shard_rows;
  const int32_t* d_shard_index;/* [pull.num_ids] */
  size_t dim;
  int kind;                    /* 0 node block, 1 edge block, 2 cache-free rows */
  int update;
  float* d_out;                /* [pull.n, dim] */
  uint32_t* d_stats;
} gf_pull_ctx;
typedef struct gf_pull_session gf_pull_session;
GF_API int gf_pull_session_create(gf_pull_session** out, gf_comm* comm, int device);
GF_API int gf_pull_session_destroy(gf_pull_session* s);
GF_API int gf_pull_round(gf_pull_session* s, gf_cache* node_cache, gf_cache* edge_cache,
                         const gf_pull_ctx* ctxs, size_t n, int flag, int* any_flag,
                         uint64_t* rows_pulled, uint64_t* bytes_sent, uint32_t* d_error_flag,
                         void* stream);

/* All fetches of one Cache.fetch_feature() call (cache.py:255-413) in one call.
 * kind 0: block of node ids through node_cache (srcdata['h'], cache.py:269-323);
 * kind 1: block of edge ids through edge_cache (edata['f'], cache.py:326-400), executed
 *         in array order; kind 2: cache-free gather from the edge feature table
 *         (target_edge_features, cache.py:411).
 * The i-th node block and the i-th edge block share one round of launches (the kernels
 * take several contexts and blockIdx.y selects one), so the two caches advance together
 * on `stream`; no host synchronisation. */
typedef struct gf_fetch_desc {
  int kind;
  int update;
  const int64_t* d_ids;
  size_t n;
  float* d_out;
  uint32_t* d_stats;
} gf_fetch_desc;
GF_API int gf_cache_fetch_blocks(gf_cache* node_cache, gf_cache* edge_cache,
                                 const gf_fetch_desc* descs, size_t n, void* stream);

/* Asynchronous submission of the same work: the descriptors are copied and handed to an
 * enqueue thread inside the library, the call returns at once with a ticket, and
 * gf_cache_fetch_wait(ticket) blocks until that submission has been ENQUEUED on `stream`
 * (and returns its status); ordering of the results is then the stream's.  Submissions
 * are enqueued in ticket order.  The caller keeps ids / outputs alive until the wait. */
GF_API int gf_cache_fetch_blocks_async(gf_cache* node_cache, gf_cache* edge_cache,
                                       const gf_fetch_desc* descs, size_t n, void* stream,
                                       uint64_t* ticket);
GF_API int gf_cache_fetch_wait(uint64_t ticket);

/* ---- host-resident feature tables: the staging ring ---------------------------------------
 * Reference: the tables live in host memory and every miss is host -> pinned -> device inside
 * fetch_feature (gnnflow/cache/cache.py:288-313,381-388, gnnflow/utils.py:284-297).  With
 * gf_cache_set_staging(generations, rows) a cache over a HOST table (pinned, device-mapped) owns
 * a ring of `generations` x `rows` table rows in HBM; gf_cache_prefetch_blocks(descs) — same
 * descriptors as the coming gf_cache_fetch_blocks, d_out / d_stats / update ignored — pulls, on
 * `stream` (a side stream), the rows of the ids that are neither cached nor already in the ring,
 * one generation per call; the next gf_cache_fetch_blocks makes its stream wait for the pulls
 * issued so far and reads a missed row from the ring when it is there, from the host table
 * otherwise.  A hint: cache state, hit counts and the fetched rows never depend on it.
 * *issued = 0 when the call issued nothing (no ring, or the generation was dropped because
 * fetches that may still read the region it would overwrite had not finished).
 * generations: a power of two in 8..64, or 0 = ring off; the ring's index takes 16 bytes per
 * table row (where an id was staged last and the time before).  gf_cache_invalidate_staging: the
 * table's contents changed.  gf_cache_staging_state out[9]: generations, rows per generation,
 * generations issued, generations dropped, rows pulled over the host link (synchronises), bytes
 * of HBM the ring and its index take, rows the gathers still read from the host table,
 * microseconds the issuing thread waited for fetches to leave a region before reusing it,
 * fetches (of the process) whose stream had to wait for a pull's event (it had not landed). */
/* The cached rows' copy in HBM.  on (default): slot s holds a copy of its id's row, a hit reads
 * it (the reference's cache buffer, gnnflow/cache/cache.py:84-99).  off — only for a feature
 * table that is itself in device memory: the slots hold ids only, every row is read from the
 * table (a hit and a miss are the same bytes at the same distance there), an install moves
 * nothing; hit ratios and the set of cached ids — the state the reference's protocol lets a
 * caller observe — are unchanged.  gnnflow_amd.cache.Cache turns it off for
 * feature_placement="device"; pinned / sharded tables keep it. */
GF_API int gf_cache_set_row_mirror(gf_cache* c, int on);
/* Diagnostics of the one-launch LRU list update (lru_list_fused_kernel): with tracing on, every
 * workgroup of an update stamps the 100 MHz wall clock at its role's stages; gf_debug_lru_trace
 * copies the last update's stamps out — words [0..3] = count / row / write workgroups and the
 * launch tag, then 8 words per workgroup (0: entry; count role 1: inputs in, 2: published; row
 * role 1: ranked + published, 2: look-back complete, 3: installed, 4: rows copied; write role 1:
 * granules in, 2: list written).  scripts/lru_hop_trace.py prints the account. */
GF_API int gf_debug_lru_trace_enable(gf_cache* c, int on);
GF_API int gf_debug_lru_trace(gf_cache* c, uint64_t* out, size_t capacity_words, size_t* words);
GF_API int gf_cache_set_staging(gf_cache* c, size_t generations, size_t rows_per_generation);
GF_API int gf_cache_invalidate_staging(gf_cache* c);
GF_API int gf_cache_staging_state(gf_cache* c, uint64_t* out);
GF_API int gf_cache_prefetch_blocks(gf_cache* node_cache, gf_cache* edge_cache,
                                    const gf_fetch_desc* descs, size_t n, void* stream,
                                    int* issued);
/* ... through the enqueue thread that issues the asynchronous fetches (same order of issue);
 * the ticket is waited for with gf_cache_fetch_wait. */
GF_API int gf_cache_prefetch_blocks_async(gf_cache* node_cache, gf_cache* edge_cache,
                                          const gf_fetch_desc* descs, size_t n, void* stream,
                                          uint64_t* ticket);
/* One submission for a pipelined step: gf_cache_fetch_blocks_async(descs) of batch i followed by
 * the prefetch of a later batch (one hand-over to the enqueue thread, one ticket).  The later
 * batch is given by descriptors (next_descs) and / or by the block array a sample() of it filled
 * (next_blocks: [next_layers x next_snapshots] as gf_sampler_sample_end wrote it, copied before
 * the call returns): the node ids of the last layer's blocks and the edge ids of every block are
 * announced — the ring's index drops the ids that blocks share. */
GF_API int gf_cache_fetch_announce_async(gf_cache* node_cache, gf_cache* edge_cache,
                                         const gf_fetch_desc* descs, size_t n, void* stream,
                                         const gf_fetch_desc* next_descs, size_t next_n,
                                         const gf_block* next_blocks, size_t next_layers,
                                         size_t next_snapshots, void* prefetch_stream,
                                         uint64_t* ticket);
/* A pipelined loop announces batches `lag` + 1 steps before it fetches them, so that a pull has
 * landed when its fetch is issued: a fetch then depends on — waits for, and reads rows of — the
 * generations up to the newest one but `lag` (default 0: every generation issued so far). */
GF_API int gf_cache_set_staging_lag(gf_cache* c, size_t lag);
/* Diagnostics: cumulative time the enqueue thread spent issuing work, and jobs done. */
GF_API int gf_worker_stats(double* busy_us, uint64_t* jobs);

/* Cache-free gather, gnnflow/utils.py:465-474 prepare_input and
 * cache.py:411 `edge_feats[eid]`: out[i,:] = feats[ids[i],:]. */
GF_API int gf_gather_rows(const float* d_feats, size_t num_rows, size_t dim,
                          const int64_t* d_ids, size_t n, float* d_out, int device,
                          void* stream);

/* ---- TGN memory / mailbox: gnnflow/models/modules/memory.py -------- */
/* Memory.prepare_input (memory.py:156-190): mem = node_memory[ids], mem_ts =
 * node_memory_ts[ids], mail_ts = mailbox_ts[ids], mem_input = mailbox[ids] — the reference's
 * CPU unique + inverse scatter is only an optimisation of exactly that.  One launch.
 * dim_mail = 2 * dim_memory + dim_edge.  An id outside [0, num_nodes) is no error: its four
 * output rows are all zero.  The call trusts its shapes (tables of num_nodes rows, d_ids and the
 * outputs of n rows); gnnflow_amd.memory.Memory checks them before it calls. */
GF_API int gf_memory_prepare_input(const float* d_node_memory, const float* d_node_memory_ts,
                                   const float* d_mailbox, const float* d_mailbox_ts,
                                   size_t num_nodes, size_t dim_memory, size_t dim_mail,
                                   const int64_t* d_ids, size_t n, float* d_mem, float* d_mem_ts,
                                   float* d_mail_ts, float* d_mem_input, int device,
                                   void* stream);
/* Memory.update_mem_mail (memory.py:192-269): d_nid / d_memory / d_ts are the
 * last_updated_{nid,memory,ts} of the n = (2 + neg_sample_ratio) * B roots; d_edge_feats
 * [B, dim_edge] or NULL (zeros).  Per distinct node the LAST occurrence wins (mailbox: in the
 * interleaved src0,dst0,src1,... order; memory: in src.. ++ dst.. order).  d_win_mail /
 * d_win_mem: caller-owned uint64[num_nodes] scratch, zero-initialised once; epoch: strictly
 * increasing, starting at 1 and below 2^31 (a caller that gets there zeroes both scratch tables
 * and starts again at 1).  A position whose id is outside [0, num_nodes) is skipped, in the
 * table whose order meets it; the batch's other positions are written as usual.  The call
 * trusts its shapes (d_nid and d_ts of n, d_memory of n rows, d_edge_feats of
 * n / (2 + neg_sample_ratio) rows) and reads past a shorter buffer;
 * gnnflow_amd.memory.Memory checks them before it calls. */
GF_API int gf_memory_update(float* d_node_memory, float* d_node_memory_ts, float* d_mailbox,
                            float* d_mailbox_ts, size_t num_nodes, size_t dim_memory,
                            size_t dim_edge, const int64_t* d_nid, const float* d_memory,
                            const float* d_ts, const float* d_edge_feats, size_t n,
                            int neg_sample_ratio, uint64_t* d_win_mail, uint64_t* d_win_mem,
                            uint64_t epoch, int device, void* stream);

/* Introspection for tests / get_mem_size (cache.py:136-155): copies the slot ->
 * id table (int64[capacity], -1 = empty) to a host array. */
GF_API int gf_cache_slot_ids(const gf_cache* c, int64_t* out, size_t capacity);
GF_API int gf_cache_mem_bytes(const gf_cache* c, size_t* out);
/* LRU bookkeeping state (no reference counterpart; diagnostics and tests).  out[0] = 1 if the
 * replacement order is kept as a queue with dead entries (caches of >= 0.5 M slots),
 * 0 if as a list; out[1] = entries allocated per queue buffer; out[2] = head, out[3] = tail of
 * the queue; out[4] = compactions so far; out[5] = updates of a queue-form cache that went
 * through the list form (block > capacity / 4 rows); out[6] = updates whose victim search had
 * to walk past the chunks behind the head.  Synchronises the device. */
GF_API int gf_cache_lru_state(const gf_cache* c, uint64_t out[7]);

/* ---- hash-partitioned sampling across the GPUs of a node ---------- */
/* The reference buckets a layer's roots by partition on the host and samples remote ones over
 * RPC (gnnflow/distributed/dist_sampler.py:159-314).  Here each rank runs, per layer:
 *   gf_partition_plan            bucket the roots by owner(v) = splitmix64(v) mod world_size
 *   (all-to-all-v of the request prefix — the caller's torch.distributed / RCCL call)
 *   gf_sampler_sample_layer_padded   on its own share (overlapping the exchange) and on the
 *                                    requests it received: fixed `fanout` slots per root
 *   (all-to-all-v of the replies)
 *   gf_sampler_merge_padded      replies -> the layer's block in the original root order,
 *                                bit-identical to single-GPU sampling (most-recent policy).
 * d_requests [n][2] int64 = (root id, root-ts bits in the low word), ordered
 * [other owners ascending | this rank]; d_pos[i] = row of root i; d_counts[world_size] device
 * words.  Replies [n][fanout][3] int64 = (dst, eid, ts | dt << 32), unused slots -1. */
GF_API int gf_partition_scratch_bytes(size_t num_roots, int world_size, size_t* out);
GF_API int gf_partition_plan(const int64_t* d_nodes, const float* d_ts, size_t num_roots,
                             int world_size, int rank, int64_t* d_requests, uint32_t* d_pos,
                             uint64_t* d_counts, void* d_scratch, size_t scratch_bytes,
                             int device, void* stream);
GF_API int gf_sampler_sample_layer_padded(gf_sampler* s, const int64_t* d_requests, size_t n,
                                          uint32_t layer, uint32_t snapshot, int64_t* d_out,
                                          void* stream);
/* d_out / out_bytes / block as gf_sampler_sample_layer (gf_sampler_layer_output_bytes);
 * synchronises `stream` once to read the edge count. */
GF_API int gf_sampler_merge_padded(gf_sampler* s, const int64_t* d_roots, const float* d_ts,
                                   size_t n, uint32_t layer, const int64_t* d_replies,
                                   const uint32_t* d_pos, void* d_out, size_t out_bytes,
                                   gf_block* block, void* stream);

/* Chained form of the same exchange — no read-back between the layers (reference loop:
 * gnnflow/distributed/dist_sampler.py:129-157 sample(), one RPC round per layer):
 *   gf_sampler_part_begin
 *   for every (layer, snapshot):
 *     gf_sampler_part_plan_own    bucket the layer's roots (their count is device resident:
 *                                 the previous layer's R + S) and sample this rank's own share
 *     — the caller exchanges: counts, request rows [0, R - counts[rank]) of the workspace out,
 *       gf_sampler_sample_layer_padded on what it received, reply rows back into the workspace —
 *     gf_sampler_part_merge       replies -> the layer's block, sizes stay on the device
 *   gf_sampler_part_commit        publishes the sizes; gf_sampler_sample_end returns the blocks
 * A rank with no roots (R = 0) still takes part in every step.  With one rank
 * gf_sampler_sample_partitioned issues the whole chain (`d_ws`: the layouts' totals, layer
 * after layer, snapshot after snapshot).  Offsets of one (layer, snapshot) workspace: */
typedef struct gf_part_layout {
  size_t root_bound;     /* worst-case roots of the layer when sample() starts from R0 roots */
  size_t requests;       /* [root_bound][2] int64, ordered [other owners ascending | own] */
  size_t replies;        /* [root_bound][fanout][3] int64, same row order */
  size_t counts;         /* [world_size] uint64: roots per owner */
  size_t pos;            /* [root_bound] uint32: row of root i */
  size_t scratch;
  size_t scratch_bytes;
  size_t total;          /* bytes of this workspace */
  /* slotted form only (0 otherwise): */
  size_t slot_stride;    /* request / reply rows per peer slot = 1 header row + capacity */
  size_t inbox;          /* [world_size][slot_stride][2] int64: the requests this rank received */
  size_t served;         /* [world_size][slot_stride][fanout][3] int64: its replies to them */
} gf_part_layout;
GF_API int gf_sampler_part_layout(const gf_sampler* s, size_t num_roots, uint32_t layer,
                                  int world_size, gf_part_layout* out);
GF_API int gf_sampler_part_begin(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                                 size_t num_roots, void* d_out, size_t out_bytes,
                                 int world_size, int rank, void* stream);
/* phases: 1 = bucket the roots, 2 = sample this rank's own share (call it right after starting
 * the request all-to-all-v: the two overlap), 3 = both */
GF_API int gf_sampler_part_plan_own(gf_sampler* s, uint32_t layer, uint32_t snapshot, void* d_ws,
                                    size_t ws_bytes, int phases);
GF_API int gf_sampler_part_merge(gf_sampler* s, uint32_t layer, uint32_t snapshot, void* d_ws,
                                 size_t ws_bytes);
GF_API int gf_sampler_part_commit(gf_sampler* s);
GF_API int gf_sampler_part_abort(gf_sampler* s);

/* Slotted form of the chained exchange: NO host synchronisation inside a sample.  The
 * variable-size exchange above needs each layer's per-owner counts on the host (they are the
 * split sizes of the all-to-all-v).  Here every peer has a slot of FIXED capacity — slack x
 * the even share of the layer's worst-case root count for a batch of `slot_roots` roots, a
 * number all ranks agree on once (their own batches may be smaller or larger: a larger one
 * merely overflows sooner) — in the request and reply buffers:
 *   requests  [world_size slots][slot_stride rows][2] int64, row 0 of a slot = its header
 *             {rows that follow, bit 0: a slot of the sender overflowed}, then this rank's own
 *             share from row world_size * slot_stride on; replies: the same rows x fanout x 3
 * so the exchanges are equal-split all-to-alls whose sizes the host knows in advance:
 *   gf_sampler_part_begin_slotted
 *   per (layer, snapshot):
 *     gf_sampler_part_plan_own(phase 1)   bucket into the slots, write the headers
 *     — all-to-all, equal split: request rows [0, world_size * slot_stride) -> `inbox` —
 *     gf_sampler_part_plan_own(phase 2)   own share, overlapping the exchange
 *     gf_sampler_part_serve               inbox -> `served` (reply row = request row)
 *     — all-to-all, equal split: `served` -> reply rows [0, world_size * slot_stride) —
 *     gf_sampler_part_merge
 *   gf_sampler_part_commit; gf_sampler_sample_end; gf_sampler_part_overflowed
 * A slot that would overflow drops the excess roots and raises a flag that travels in the
 * headers, so EVERY rank sees it in the same exchange; gf_sampler_part_overflowed reports it
 * for the sample gf_sampler_sample_end returned last, and all ranks then sample that batch
 * again through the variable-size exchange (no reference counterpart: the reference's RPC
 * futures are variable-size by construction, gnnflow/distributed/dist_sampler.py:188-242). */
GF_API int gf_sampler_part_layout_slotted(const gf_sampler* s, size_t num_roots, uint32_t layer,
                                          int world_size, double slack, size_t slot_roots,
                                          gf_part_layout* out);
/* What one slot of a shared chain's exchanges takes on the wire for `layer` (the layout the
 * native chains use, sampler_group.hip group_layout): out[0] = rows per request slot (16 B each, header
 * row included), out[1] = bytes of one reply slot (compact: offsets + packed edges; edge_fill 0:
 * the fixed records), out[2] = edges a compact reply slot holds at most, out[3] = bytes of its
 * offsets (2 / 4).  narrow: bit 0 = 12-byte reply records, bit 1 = layer l + 1 does not request
 * layer l's roots again (its slots are sized for the roots that are new in it).
 * gnnflow_amd.dist.DevicePartitionedSampler.wire_bytes_per_sample reports from this, so the
 * figures in bench.py's line are the native layout's, not a restatement. */
GF_API int gf_sampler_part_group_slot(const gf_sampler* s, size_t num_roots, uint32_t layer,
                                      int world_size, double slack, size_t slot_roots, int narrow,
                                      double edge_fill, uint64_t* out);
GF_API int gf_sampler_part_begin_slotted(gf_sampler* s, const int64_t* d_roots,
                                         const float* d_root_ts, size_t num_roots, void* d_out,
                                         size_t out_bytes, int world_size, int rank, double slack,
                                         size_t slot_roots, void* stream);
GF_API int gf_sampler_part_serve(gf_sampler* s, uint32_t layer, uint32_t snapshot, void* d_ws,
                                 size_t ws_bytes);
GF_API int gf_sampler_part_overflowed(const gf_sampler* s, int* out);
GF_API int gf_sampler_sample_partitioned(gf_sampler* s, const int64_t* d_roots,
                                         const float* d_root_ts, size_t num_roots, void* d_out,
                                         size_t out_bytes, void* d_ws, size_t ws_bytes,
                                         void* stream);
/* ... the same, issued by the library's enqueue thread (see gf_sampler_sample_begin_async) */
GF_API int gf_sampler_sample_partitioned_async(gf_sampler* s, const int64_t* d_roots,
                                               const float* d_root_ts, size_t num_roots,
                                               void* d_out, size_t out_bytes, void* d_ws,
                                               size_t ws_bytes, void* stream);

/* ---- RCCL communicator of the partitioned path ------------------------------------------- */
/* The exchanges above issued by the library itself over RCCL / xGMI (the reference's transport
 * is torch RPC between machines, gnnflow/distributed/dist_sampler.py:188-242).  RCCL is resolved
 * at run time (the librccl.so.1 already in the process, else ROCm's), so a single-GPU user never
 * loads it.  Bootstrap: rank 0 calls gf_comm_unique_id and hands the 128 bytes to every rank by
 * whatever channel it has (torch.distributed broadcast, a file, MPI); then EVERY rank calls
 * gf_comm_create (collective).  gf_comm_all_to_all: bytes_per_peer bytes to / from every rank
 * (equal split, this rank included), ordered on `stream`; gf_comm_all_to_all_v: host arrays of
 * world_size byte counts / byte offsets. */
GF_API int gf_comm_unique_id(uint8_t out[128]);
GF_API int gf_comm_create(gf_comm** out, const uint8_t id[128], int world_size, int rank,
                          int device);
GF_API int gf_comm_destroy(gf_comm* c);
GF_API int gf_comm_all_to_all(gf_comm* c, const void* d_send, void* d_recv, size_t bytes_per_peer,
                              void* stream);
GF_API int gf_comm_all_to_all_v(gf_comm* c, const void* d_send, const size_t* send_bytes,
                                const size_t* send_offsets, void* d_recv, const size_t* recv_bytes,
                                const size_t* recv_offsets, void* stream);
/* What the transport itself reports: out = {ranks, this rank, device, kind (0 RCCL, 1 hipIpc, 2
 * loopback)}; for RCCL these are ncclCommCount / ncclCommUserRank / ncclCommCuDevice — bench.py
 * puts them into the N > 1 line ("did RCCL see N ranks on N devices?").  The reference all-gathers
 * its per-rank sampling timers the same way (gnnflow/distributed/dist_sampler.py:108-127). */
GF_API int gf_comm_info(gf_comm* c, int32_t out[4]);
/* Gives the communicator up without waiting for its peers (ncclCommAbort): for a rank whose
 * collective never completes.  Only gf_comm_destroy may follow. */
GF_API int gf_comm_abort(gf_comm* c);
/* `iters` back-to-back equal-split all-to-alls of `bytes_per_peer` on scratch buffers: device time
 * (events around the batch) and the issuing thread's host time, per exchange, in microseconds —
 * the x and c of DESIGN 6.2's projection.  Collective. */
GF_API int gf_comm_time_all_to_all(gf_comm* c, size_t bytes_per_peer, int iters, void* stream,
                                   double* device_us, double* host_us);
/* PCI bus id of a HIP device ("0000:c1:00.0"), len >= 16. */
GF_API int gf_device_pci_bus_id(int device, char* out, size_t len);
/* Do two streams of `device` run on the same hardware queue?  HIP spreads its streams over four
 * hardware queues and kernels of streams that share one run one after the other: a side stream
 * meant to work BESIDE another (a sampling lane, the staging ring's pull stream) must not share
 * its queue.  The probe holds stream `a` with a kernel that spins for `spin_us` microseconds of
 * wall clock and looks whether a one-thread kernel on stream `b` finishes meanwhile.
 * *shared = 1: it did not (same queue, or the device would not run the two side by side).
 * Synchronises both streams.  gnnflow_amd.pipeline.side_stream picks its streams with it. */
GF_API int gf_streams_share_queue(int device, void* a, void* b, unsigned spin_us, int* shared);
/* The same exchanges between processes that map each other's device memory (hipIpc*) — the ranks
 * of one node, several ranks SHARING one GPU included (where RCCL refuses to run): a
 * host-synchronising test / single-box transport (copy-out, process barrier over POSIX shared
 * memory, copy-in from the peers' mailboxes, barrier).  Every rank: gf_ipc_comm_create (same
 * `shm_name`, "/..."; `mailbox_bytes` = its largest message), gf_ipc_comm_handle -> 64 bytes to
 * publish to all ranks, gf_ipc_comm_open(all handles, rank-major).  The handle then works with
 * every gf_comm_* / *_comm entry point. */
GF_API int gf_ipc_comm_create(gf_comm** out, int world_size, int rank, int device,
                              size_t mailbox_bytes, const char* shm_name);
GF_API int gf_ipc_comm_handle(gf_comm* c, uint8_t out[64]);
GF_API int gf_ipc_comm_open(gf_comm* c, const uint8_t* handles);

/* The same exchanges between "ranks" that live in ONE process (world_size handles, rank r =
 * out[r], all on `device`): each rank is driven by its own host thread, an exchange is a thread
 * barrier + device copies straight out of the peers' send buffers.  Host-synchronising test
 * transport: it runs the native multi-rank chains at world sizes a one-GPU box cannot give as
 * processes (8 ranks).  Works with every gf_comm_* / *_comm entry point except the *_async
 * ones (one enqueue thread cannot serve ranks that wait for each other).  No reference
 * counterpart (the reference has no distributed test). */
GF_API int gf_loopback_comm_create(gf_comm** out, int world_size, int device);

/* The slotted chain of one sample() over `c` in ONE call (and through the enqueue thread):
 * gf_sampler_part_begin_slotted, then per (layer, snapshot) plan -> request slots out -> own
 * share + serve -> reply slots back -> merge, then commit; nothing is read back.
 * d_ws: the slotted layouts' totals, layer after layer, snapshot after snapshot.
 * overlap != 0: the exchanges run on the communicator's own stream, the request exchange while
 * this rank's own share is sampled on `stream`.  gf_sampler_sample_end + gf_sampler_part_overflowed
 * complete it. */
GF_API int gf_sampler_sample_partitioned_comm(gf_sampler* s, gf_comm* c, const int64_t* d_roots,
                                              const float* d_root_ts, size_t num_roots,
                                              void* d_out, size_t out_bytes, void* d_ws,
                                              size_t ws_bytes, double slack, size_t slot_roots,
                                              int overlap, void* stream);
GF_API int gf_sampler_sample_partitioned_comm_async(gf_sampler* s, gf_comm* c,
                                                    const int64_t* d_roots, const float* d_root_ts,
                                                    size_t num_roots, void* d_out, size_t out_bytes,
                                                    void* d_ws, size_t ws_bytes, double slack,
                                                    size_t slot_roots, int overlap, void* stream);

/* Up to GF_PART_GROUP_MAX samples in ONE chain: at batch 600 the chain's throughput is bound by
 * the host thread that issues its ~11 stream operations, so m consecutive batches share their
 * launches and their exchanges — sample j through its own sampler `samples[j].sampler` (m
 * samplers over the same graph with the same arguments: each keeps its own output, block
 * counters and publish record; gf_sampler_sample_end / gf_sampler_part_overflowed per sampler as
 * usual).  Owner q's requests of sample j travel in slot m q + j of ONE buffer, so one
 * equal-split all-to-all moves every sample's slots; 11 operations per m samples.
 * gf_sampler_part_group_ws_bytes: size of the shared exchange workspace for samples of
 * roots[0..m) roots, 0 if they cannot share a chain (several snapshots, a layer beyond 32 768
 * roots, fanout > 256): the caller then issues single chains.  force_overflow (bit j: sample
 * j): flag that sample as overflowed whatever its slots hold — for a batch that is too large for
 * this chain although the batch size the ranks agreed on is not, the caller submits an EMPTY
 * stand-in with this bit set, every rank sees the flag in the same exchange and the real batch
 * is sampled in the redo.  c == NULL: ONE rank with nothing to exchange (world size 1, every root
 * its own) — the same chain without the two all-to-alls.  narrow_ids != 0: reply slots of 12
 * bytes {destination, edge id, edge time} instead of 24 — half the bytes of the reply exchange;
 * the SAME value on every rank (it is part of the wire format), and only while every rank's
 * shard satisfies gf_graph_ids_fit_u32 (a rank whose shard stops fitting sets every bit of
 * force_overflow: all ranks then redo those samples through the wide variable-size form).
 * No reference counterpart (its RPC
 * futures are per partition and per call, gnnflow/distributed/dist_sampler.py:188-220). */
#define GF_PART_GROUP_MAX 4
typedef struct gf_group_sample {
  gf_sampler* sampler;
  const int64_t* d_roots;
  const float* d_root_ts;
  size_t num_roots;
  void* d_out;          /* gf_sampler_output_bytes(num_roots) bytes, as for gf_sampler_sample */
  size_t out_bytes;
} gf_group_sample;
/* `narrow_ids` of the three entry points below is a flags word: bit 0 = 12-byte reply records;
 * bit 1 = a layer does not request the previous layer's roots again (its first roots ARE those,
 * with the same timestamps: with most-recent sampling and equal fanouts the merge takes their
 * edges from the previous layer's block; the reference requests every root of every layer,
 * gnnflow/distributed/dist_sampler.py:174-186);
 * bits 8..23 = COMPACT replies, the edge fill in 1/1000: a reply slot that travels back then holds,
 * per request row, the offset of its edges and, packed behind the offsets, the edges themselves —
 * at most fill x (slot rows x fanout) of them — instead of `fanout` fixed records per row, most of
 * which are empty (the reference ships back exactly a partition's sampled edges,
 * gnnflow/distributed/common.py:4-19, dist_sampler.py:244-314).  A slot with more edges flags the
 * sample as overflowed on every rank (it is redone through the variable-size exchange).  Part of
 * the wire format: the same on every rank; 0 = the fixed records travel. */
GF_API int gf_sampler_part_group_ws_bytes(const gf_sampler* s, const size_t* roots, int m,
                                          int world_size, double slack, size_t slot_roots,
                                          int narrow_ids, size_t* bytes);
GF_API int gf_sampler_sample_partitioned_comm_group(gf_comm* c, const gf_group_sample* samples,
                                                    int m, void* d_ws, size_t ws_bytes,
                                                    double slack, size_t slot_roots,
                                                    int force_overflow, int narrow_ids,
                                                    void* stream);
/* ... issued by the library's enqueue thread (like gf_sampler_sample_partitioned_comm_async) */
GF_API int gf_sampler_sample_partitioned_comm_group_async(gf_comm* c,
                                                          const gf_group_sample* samples, int m,
                                                          void* d_ws, size_t ws_bytes,
                                                          double slack, size_t slot_roots,
                                                          int force_overflow, int narrow_ids,
                                                          void* stream);

/* ---- message passing on a sampled block ---------------------- */
/* The DGL calls of the reference's layers on an MFG (gnnflow/models/modules/layers.py:153-159,
 * models/graphsage.py:27-31, models/gat.py:28-46), as segment operations: a block's edges are
 * grouped by destination (`row` non-decreasing, as the sampler emits them).  fp32, device
 * pointers, ordered on `stream`.
 * offsets[d] = first edge with row >= d, d = 0..num_dst (so offsets[num_dst] = num_edges). */
GF_API int gf_block_segment_offsets(const int64_t* d_row, size_t num_edges, size_t num_dst,
                                    int64_t* d_offsets, int device, void* stream);
/* dgl.ops.edge_softmax(block, logits[num_edges, heads]): softmax over each destination's edges */
GF_API int gf_block_edge_softmax(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                 size_t heads, const float* d_logits, float* d_out, int device,
                                 void* stream);
GF_API int gf_block_edge_softmax_backward(const int64_t* d_offsets, size_t num_dst,
                                          size_t num_edges, size_t heads, const float* d_out,
                                          const float* d_grad_out, float* d_grad_logits,
                                          int device, void* stream);
/* update_all(copy_src | u_mul_e, sum | mean): out[d, :] = reduce over edges k of d of
 * edge_weight[k, head] * src[col[k], :]  (d_edge_weight NULL: copy_src; else [num_edges, heads]
 * with dim % heads == 0, each weight covering dim / heads consecutive columns).
 * d_col NULL = the sampler's own layout col[k] = num_dst + k (then num_src must be
 * num_dst + num_edges): contiguous reads, and a backward pass without atomics. */
GF_API int gf_block_reduce(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                           const float* d_src, size_t dim, const float* d_edge_weight,
                           size_t heads, int mean, float* d_out, int device, void* stream);
/* d_grad_src [num_src, dim] is zeroed then accumulated (NULL: skipped); d_grad_edge_weight
 * [num_edges, heads] or NULL. */
GF_API int gf_block_reduce_backward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                                    const float* d_src, size_t dim, const float* d_edge_weight,
                                    size_t heads, int mean, const float* d_grad_out,
                                    float* d_grad_src, size_t num_src,
                                    float* d_grad_edge_weight, int device, void* stream);

/* update_all(copy_src, max) — dgl.nn.SAGEConv's 'pool' aggregator: out[d, c] = max over the
 * in-edges of src[col[k], c] (0 without in-edges); d_arg [num_dst, dim] receives the winning
 * edge per element (-1: none), which the backward pass routes the gradient through. */
GF_API int gf_block_reduce_max(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                               const float* d_src, size_t dim, float* d_out, int64_t* d_arg,
                               int device, void* stream);
GF_API int gf_block_reduce_max_backward(size_t num_dst, const int64_t* d_col, size_t dim,
                                        const float* d_grad_out, const int64_t* d_arg,
                                        float* d_grad_src, size_t num_src, int device,
                                        void* stream);

/* Fused attention of the reference's TransfomerAttentionLayer (layers.py:144-159), whose keys
 * and values are PER EDGE: q [num_dst, heads, head_dim], k / v [num_edges, heads, head_dim],
 *   z[e,h] = sum_c q[d,h,c] k[e,h,c]   (d = destination of e, from d_offsets)
 *   att    = edge softmax of leaky_relu(z, negative_slope)          -> d_att [num_edges, heads]
 *   out[d,h,:] = sum over the edges e of d of att[e,h] v[e,h,:]     -> d_out [num_dst, heads, head_dim]
 * (a destination without in-edges: 0).  k and v are read once, no atomics; d_att is what the
 * backward pass needs besides the inputs.  heads, head_dim >= 1 with
 * heads * head_dim <= GF_BLOCK_ATTENTION_MAX_WIDTH, else GF_ERR_INVALID_ARGUMENT. */
#define GF_BLOCK_ATTENTION_MAX_WIDTH 1024
GF_API int gf_block_attention(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                              size_t heads, size_t head_dim, const float* d_q, const float* d_k,
                              const float* d_v, float negative_slope, float* d_out, float* d_att,
                              int device, void* stream);
/* Each of d_grad_q [num_dst, ...], d_grad_k, d_grad_v [num_edges, ...] may be NULL (not needed:
 * its work is skipped); every element of the others is written exactly once, rows of
 * destinations without in-edges included. */
GF_API int gf_block_attention_backward(const int64_t* d_offsets, size_t num_dst,
                                       size_t num_edges, size_t heads, size_t head_dim,
                                       const float* d_q, const float* d_k, const float* d_v,
                                       const float* d_att, float negative_slope,
                                       const float* d_grad_out, float* d_grad_q,
                                       float* d_grad_k, float* d_grad_v, int device,
                                       void* stream);
/* gf_block_attention with dropout on the attention weights (after the softmax, as the reference's
 * att_dropout, layers.py:153-155), from a stateless mask: with i the position of an edge in the
 * grouped order of d_offsets and p an fp32 value in [0, 1),
 *   T         = (uint32_t)((double)p * 4294967296.0)
 *   keep[i,h] = gf_philox4x32_10_first(seed, i * heads + h, 0) >= T        (gnnflow_rng.h)
 *   w[i,h]    = keep ? 1.0f / (1.0f - p) : 0
 *   out[d,h,:] = sum over the edges i of d of (att[i,h] * w[i,h]) * v[i,h,:]
 * d_att receives the PRE-dropout softmax (what the backward needs); d_att_dropped, unless NULL,
 * receives att * w [num_edges, heads].  A dropped edge contributes exactly 0 and its v row is not
 * read, so a non-finite v there does not propagate.  p outside [0, 1) or NaN:
 * GF_ERR_INVALID_ARGUMENT; p == 0 gives the bits of gf_block_attention.  The backward draws the
 * mask again from (p, seed): nothing else is stored.  gv rows of dropped edges are exact zeros;
 * otherwise as gf_block_attention_backward. */
GF_API int gf_block_attention_dropout(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                      size_t heads, size_t head_dim, const float* d_q,
                                      const float* d_k, const float* d_v, float negative_slope,
                                      float p, uint64_t seed, float* d_out, float* d_att,
                                      float* d_att_dropped, int device, void* stream);
GF_API int gf_block_attention_dropout_backward(const int64_t* d_offsets, size_t num_dst,
                                               size_t num_edges, size_t heads, size_t head_dim,
                                               const float* d_q, const float* d_k,
                                               const float* d_v, const float* d_att,
                                               float negative_slope, float p, uint64_t seed,
                                               const float* d_grad_out, float* d_grad_q,
                                               float* d_grad_k, float* d_grad_v, int device,
                                               void* stream);

/* The four entry points above for bfloat16 q, k, v, out and gradients, carried as uint16_t (the
 * upper half of a float32); d_att and d_att_dropped stay float32.  Every element is widened to
 * float32 when it is loaded (exact), the arithmetic is that of the float32 entry points in the
 * same order, and each result is rounded once, to nearest even, when it is stored (NaN -> 0x7FC0,
 * overflow -> infinity).  So d_out, d_grad_q, d_grad_k and d_grad_v hold, bit for bit, the
 * float32 entry point's results on the widened inputs, rounded to bfloat16; d_att and
 * d_att_dropped are equal to its outputs.  Arguments, order, checks and limits are the float32
 * siblings'. */
GF_API int gf_block_attention_bf16(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                   size_t heads, size_t head_dim, const uint16_t* d_q,
                                   const uint16_t* d_k, const uint16_t* d_v, float negative_slope,
                                   uint16_t* d_out, float* d_att, int device, void* stream);
GF_API int gf_block_attention_bf16_backward(const int64_t* d_offsets, size_t num_dst,
                                            size_t num_edges, size_t heads, size_t head_dim,
                                            const uint16_t* d_q, const uint16_t* d_k,
                                            const uint16_t* d_v, const float* d_att,
                                            float negative_slope, const uint16_t* d_grad_out,
                                            uint16_t* d_grad_q, uint16_t* d_grad_k,
                                            uint16_t* d_grad_v, int device, void* stream);
GF_API int gf_block_attention_dropout_bf16(const int64_t* d_offsets, size_t num_dst,
                                           size_t num_edges, size_t heads, size_t head_dim,
                                           const uint16_t* d_q, const uint16_t* d_k,
                                           const uint16_t* d_v, float negative_slope, float p,
                                           uint64_t seed, uint16_t* d_out, float* d_att,
                                           float* d_att_dropped, int device, void* stream);
GF_API int gf_block_attention_dropout_bf16_backward(const int64_t* d_offsets, size_t num_dst,
                                                    size_t num_edges, size_t heads,
                                                    size_t head_dim, const uint16_t* d_q,
                                                    const uint16_t* d_k, const uint16_t* d_v,
                                                    const float* d_att, float negative_slope,
                                                    float p, uint64_t seed,
                                                    const uint16_t* d_grad_out,
                                                    uint16_t* d_grad_q, uint16_t* d_grad_k,
                                                    uint16_t* d_grad_v, int device,
                                                    void* stream);

/* Fused GAT attention (dgl.nn.GATConv's message passing) over a block: feat [num_src, heads,
 * head_dim], el [num_src, heads], er [num_dst, heads]; src(e) = d_col[e], or num_dst + e when
 * d_col is NULL (the sampler's layout; num_src must then be num_dst + num_edges),
 *   z[e,h] = el[src(e),h] + er[d,h]   (d = destination of e, from d_offsets)
 *   att    = edge softmax of leaky_relu(z, negative_slope)            -> d_att [num_edges, heads]
 *   out[d,h,:] = sum over the edges e of d of (att[e,h] * w[e,h]) * feat[src(e),h,:]
 * (a destination without in-edges: 0).  w is the dropout mask of gf_block_attention_dropout,
 * unchanged: p an fp32 value in [0, 1) (else GF_ERR_INVALID_ARGUMENT), i the position of an edge
 * in the grouped order of d_offsets, keep[i,h] = gf_philox4x32_10_first(seed, i * heads + h, 0)
 * >= (uint32_t)((double)p * 4294967296.0), w = keep ? 1.0f / (1.0f - p) : 0; p == 0 is the call
 * without dropout (w = 1, seed unused).  d_att receives the PRE-dropout softmax; d_att_dropped,
 * unless NULL, receives att * w.  Each feat row is read at most once and a dropped edge's row not
 * at all.  heads * head_dim <= GF_BLOCK_ATTENTION_MAX_WIDTH, else GF_ERR_INVALID_ARGUMENT. */
GF_API int gf_block_gat(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                        const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                        const float* d_feat, const float* d_el, const float* d_er,
                        float negative_slope, float p, uint64_t seed, float* d_out, float* d_att,
                        float* d_att_dropped, int device, void* stream);
/* d_att and d_out as the forward wrote them, (p, seed) as the forward got them: the mask is drawn
 * again.  Each of d_grad_feat [num_src, heads, head_dim], d_grad_el [num_src, heads] and
 * d_grad_er [num_dst, heads] may be NULL (skipped); every element of the others is written.
 * d_col NULL: no atomics, each element written exactly once (the rows [0, num_dst) no edge reads
 * are zeros), bit-identical from run to run.  Otherwise d_grad_feat and d_grad_el are zeroed and
 * accumulated with atomic adds (a source may feed several edges): rows no edge reads are exact
 * zeros, the rest may differ in the last bits from run to run. */
GF_API int gf_block_gat_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                 const int64_t* d_col, size_t num_src, size_t heads,
                                 size_t head_dim, const float* d_feat, const float* d_el,
                                 const float* d_er, const float* d_att, const float* d_out,
                                 float negative_slope, float p, uint64_t seed,
                                 const float* d_grad_out, float* d_grad_feat, float* d_grad_el,
                                 float* d_grad_er, int device, void* stream);

/* gf_block_reduce, gf_block_reduce_max, gf_block_gat and their backward passes for bfloat16
 * source rows (d_src, d_feat), outputs (d_out) and their gradients (d_grad_out, d_grad_src,
 * d_grad_feat), carried as uint16_t.  What autocast leaves float32 stays float32: the edge
 * weights and their gradient, d_arg, d_el, d_er, d_att, d_att_dropped, d_grad_el, d_grad_er.
 * Every bfloat16 element is widened where it is loaded (exact), the arithmetic is that of the
 * float32 entry point in the same order, and each bfloat16 result is rounded once, to nearest
 * even, where it is stored: the bfloat16 results hold, bit for bit, the float32 entry point's
 * results on the widened inputs rounded to bfloat16, and the float32 results are equal to its.
 * Arguments, order, checks and limits are the float32 siblings'; what a bfloat16 entry point
 * needs besides comes LAST, after `stream`:
 *   d_scratch   float32 [num_src, dim] (gf_block_gat_backward_bf16: [num_src, heads, head_dim]),
 *               caller-owned, contents irrelevant.  With d_col the gradient of the source rows is
 *               accumulated there with float32 atomic adds -- a bfloat16 add would round once per
 *               edge -- and rounded into d_grad_src / d_grad_feat by one more launch.  May be
 *               NULL when d_col is NULL (each element is then stored once, directly in bfloat16,
 *               without atomics) or when that gradient is not asked for.
 *   d_out_f32   float32 [num_dst, heads, head_dim]: gf_block_gat_bf16 writes the sums there
 *               before it rounds them into d_out, and gf_block_gat_backward_bf16 takes it where
 *               gf_block_gat_backward takes d_out (the rounded d_out would give another
 *               gout . out than the float32 op's).  NULL in the forward: not written. */
GF_API int gf_block_reduce_bf16(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                                const uint16_t* d_src, size_t dim, const float* d_edge_weight,
                                size_t heads, int mean, uint16_t* d_out, int device,
                                void* stream);
GF_API int gf_block_reduce_backward_bf16(const int64_t* d_offsets, size_t num_dst,
                                         const int64_t* d_col, const uint16_t* d_src, size_t dim,
                                         const float* d_edge_weight, size_t heads, int mean,
                                         const uint16_t* d_grad_out, uint16_t* d_grad_src,
                                         size_t num_src, float* d_grad_edge_weight, int device,
                                         void* stream, float* d_scratch);
GF_API int gf_block_reduce_max_bf16(const int64_t* d_offsets, size_t num_dst,
                                    const int64_t* d_col, const uint16_t* d_src, size_t dim,
                                    uint16_t* d_out, int64_t* d_arg, int device, void* stream);
GF_API int gf_block_reduce_max_backward_bf16(size_t num_dst, const int64_t* d_col, size_t dim,
                                             const uint16_t* d_grad_out, const int64_t* d_arg,
                                             uint16_t* d_grad_src, size_t num_src, int device,
                                             void* stream, float* d_scratch);
GF_API int gf_block_gat_bf16(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                             const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                             const uint16_t* d_feat, const float* d_el, const float* d_er,
                             float negative_slope, float p, uint64_t seed, uint16_t* d_out,
                             float* d_att, float* d_att_dropped, int device, void* stream,
                             float* d_out_f32);
GF_API int gf_block_gat_backward_bf16(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                      const int64_t* d_col, size_t num_src, size_t heads,
                                      size_t head_dim, const uint16_t* d_feat, const float* d_el,
                                      const float* d_er, const float* d_att,
                                      const float* d_out_f32, float negative_slope, float p,
                                      uint64_t seed, const uint16_t* d_grad_out,
                                      uint16_t* d_grad_feat, float* d_grad_el, float* d_grad_er,
                                      int device, void* stream, float* d_scratch);

/* Fused time encoding (the reference's TimeEncode, layers.py:16-42, and the torch.cat around
 * it): d_out [n, width_a + width_b + dim_time], row-major and contiguous,
 *   out[i, 0:width_a]                = a[i, :]      (width_a may be 0, d_a NULL)
 *   out[i, width_a:width_a+width_b]  = b[i, :]      (width_b may be 0, d_b NULL)
 *   out[i, width_a+width_b+j]        = cosf(w[j] * t[i] + bias[j]),  j < dim_time
 * in one launch, every element written exactly once; d_a / d_b are contiguous [n, width].
 * dim_time >= 1 and fewer than 2^32 output elements, else GF_ERR_INVALID_ARGUMENT; n == 0
 * launches nothing. */
GF_API int gf_time_encode_cat(const float* d_a, size_t width_a, const float* d_b, size_t width_b,
                              const float* d_t, const float* d_w, const float* d_bias, size_t n,
                              size_t dim_time, float* d_out, int device, void* stream);
/* Rows of the caller-owned partials buffer gf_time_encode_backward needs for n input rows
 * (at most 1024 whatever n is): the buffer holds rows * 2 * dim_time floats. */
GF_API int gf_time_encode_backward_partial_rows(size_t n, size_t* rows);
/* Gradients of w and bias from the time columns g[i, j] = d_grad_out[i * grad_pitch + grad_col + j]
 * (read in place; grad_col + dim_time <= grad_pitch):
 *   grad_w[j]    = - sum_i g[i,j] * sinf(w[j] * t[i] + bias[j]) * t[i]
 *   grad_bias[j] = - sum_i g[i,j] * sinf(w[j] * t[i] + bias[j])
 * summed in a fixed order without atomics (bit-identical from run to run).  d_grad_w or
 * d_grad_bias may be NULL (skipped).  There is no gradient for t.  The gradients of a and b
 * are the column slices of grad_out and need no call. */
GF_API int gf_time_encode_backward(const float* d_t, const float* d_w, const float* d_bias,
                                   size_t n, size_t dim_time, const float* d_grad_out,
                                   size_t grad_pitch, size_t grad_col, float* d_partials,
                                   size_t partial_rows, float* d_grad_w, float* d_grad_bias,
                                   int device, void* stream);

/* gf_time_encode_cat with a bfloat16 d_out (uint16_t as above; parts, t, w and bias float32):
 * every column is the float32 entry point's value rounded once to nearest even, so a copied
 * column is a plain float32 -> bfloat16 conversion.  gf_time_encode_backward_bf16 reads a
 * bfloat16 d_grad_out (grad_pitch and grad_col in elements), widened on load; the partials
 * (gf_time_encode_backward_partial_rows as before), grad_w and grad_bias stay float32 and are the
 * float32 entry point's on the widened gradient, bit for bit.  The same checks. */
GF_API int gf_time_encode_cat_bf16(const float* d_a, size_t width_a, const float* d_b,
                                   size_t width_b, const float* d_t, const float* d_w,
                                   const float* d_bias, size_t n, size_t dim_time,
                                   uint16_t* d_out, int device, void* stream);
GF_API int gf_time_encode_backward_bf16(const float* d_t, const float* d_w, const float* d_bias,
                                        size_t n, size_t dim_time, const uint16_t* d_grad_out,
                                        size_t grad_pitch, size_t grad_col, float* d_partials,
                                        size_t partial_rows, float* d_grad_w, float* d_grad_bias,
                                        int device, void* stream);

/* Fused edge score (the tail of the reference's EdgePredictor, layers.py:186-197, after src_fc
 * and dst_fc): d_src [num_src, dim], d_dst [num_dst, dim], d_w [dim], d_bias [1], d_out
 * [num_dst], all fp32, row-major and contiguous; num_dst = r * num_src, row j of dst pairs with
 * row j mod num_src of src,
 *   out[j] = bias + sum_d w[d] * max(src[j mod num_src, d] + dst[j, d], 0)
 * in one launch.  The order of summation depends on dim alone.  dim >= 1, num_dst a multiple of
 * num_src >= 1 and fewer than 2^31 dst rows, else GF_ERR_INVALID_ARGUMENT; num_dst == 0
 * launches nothing. */
GF_API int gf_edge_score(const float* d_src, const float* d_dst, const float* d_w,
                         const float* d_bias, size_t num_src, size_t num_dst, size_t dim,
                         float* d_out, int device, void* stream);
/* Rows of the caller-owned partials buffer gf_edge_score_backward needs for num_src src rows
 * (at most 1024 whatever num_src is): the buffer holds rows * (dim + 1) floats. */
GF_API int gf_edge_score_backward_partial_rows(size_t num_src, size_t* rows);
/* Gradients of the edge score from g = d_grad_out [num_dst], with x[j,d] = src[j mod num_src, d]
 * + dst[j, d]:
 *   grad_dst[j,d] = x[j,d] > 0 ? g[j] * w[d] : 0
 *   grad_src[i,d] = grad_dst[i,d] + grad_dst[i + num_src,d] + ...      (ascending)
 *   grad_w[d]     = sum_j g[j] * max(x[j,d], 0)          grad_bias = sum_j g[j]
 * in at most two launches, summed in a fixed order without atomics (bit-identical from run to
 * run).  Any of d_grad_src, d_grad_dst, d_grad_w, d_grad_bias may be NULL (skipped); d_partials
 * is needed only when d_grad_w or d_grad_bias is not NULL. */
GF_API int gf_edge_score_backward(const float* d_src, const float* d_dst, const float* d_w,
                                  size_t num_src, size_t num_dst, size_t dim,
                                  const float* d_grad_out, float* d_partials, size_t partial_rows,
                                  float* d_grad_src, float* d_grad_dst, float* d_grad_w,
                                  float* d_grad_bias, int device, void* stream);

/* gf_edge_score and gf_edge_score_backward for bfloat16 d_src and d_dst rows (uint16_t as above)
 * and bfloat16 d_grad_src / d_grad_dst; d_w, d_bias, d_out, d_grad_out, the partials
 * (gf_edge_score_backward_partial_rows as before), d_grad_w and d_grad_bias stay float32.  Rows
 * are widened on load, the arithmetic and its order are the float32 entry points', and grad_src
 * and grad_dst are rounded once on store: every output equals the float32 entry point's on the
 * widened rows (grad_src, grad_dst: rounded to bfloat16), bit for bit.  The same checks. */
GF_API int gf_edge_score_bf16(const uint16_t* d_src, const uint16_t* d_dst, const float* d_w,
                              const float* d_bias, size_t num_src, size_t num_dst, size_t dim,
                              float* d_out, int device, void* stream);
GF_API int gf_edge_score_backward_bf16(const uint16_t* d_src, const uint16_t* d_dst,
                                       const float* d_w, size_t num_src, size_t num_dst,
                                       size_t dim, const float* d_grad_out, float* d_partials,
                                       size_t partial_rows, uint16_t* d_grad_src,
                                       uint16_t* d_grad_dst, float* d_grad_w, float* d_grad_bias,
                                       int device, void* stream);

/* Fused epilogue of the reference's TemporalAttentionLayer (layers.py: layer_norm(relu(dropout(
 * w_out(rst)))), after the GEMM): d_x [num_rows, dim], d_gamma and d_beta [dim], d_out
 * [num_rows, dim], d_mean and d_rstd [num_rows], all fp32, row-major and contiguous.  With p an
 * fp32 value in [0, 1), T = (uint32_t)((double)p * 4294967296.0) and sc = 1.0f / (1.0f - p):
 *   keep[r,d] = gf_philox4x32_10_first(seed, r * dim + d, 0) >= T        (gnnflow_rng.h)
 *   y[r,d]    = max(keep ? x[r,d] * sc : 0, 0)            p == 0: y = max(x, 0), seed unused
 *   mean[r]   = sum_d y / dim      var[r] = sum_d (y - mean)^2 / dim
 *   rstd[r]   = 1 / sqrtf(var + eps)
 *   out[r,d]  = (y - mean) * rstd * gamma[d] + beta[d]
 * in one launch: one wave per row, the row read once, the variance taken from the deviations.  No
 * mask is written; d_mean and d_rstd are what the backward needs besides x.  The bits depend on
 * dim alone, not on num_rows, the grid or the alignment of the pointers.  dim == 0, dim >
 * GF_LAYER_EPILOGUE_MAX_WIDTH, p outside [0, 1) or NaN, eps not > 0, 2^31 rows or more, or a NULL
 * pointer when num_rows > 0: GF_ERR_INVALID_ARGUMENT; num_rows == 0 launches nothing. */
#define GF_LAYER_EPILOGUE_MAX_WIDTH 1024
GF_API int gf_layer_epilogue(const float* d_x, const float* d_gamma, const float* d_beta,
                             size_t num_rows, size_t dim, float eps, float p, uint64_t seed,
                             float* d_out, float* d_mean, float* d_rstd, int device,
                             void* stream);
/* Rows of the caller-owned partials buffer gf_layer_epilogue_backward needs for num_rows rows (at
 * most 1024 whatever num_rows is): the buffer holds rows * 2 * dim floats. */
GF_API int gf_layer_epilogue_backward_partial_rows(size_t num_rows, size_t* rows);
/* Gradients of gf_layer_epilogue from d_grad_out [num_rows, dim], with y and keep recomputed from
 * x, p and seed, and d_mean / d_rstd as the forward wrote them:
 *   xhat = (y - mean) * rstd          g = grad_out * gamma
 *   dy   = rstd * (g - sum_d(g) / dim - xhat * (sum_d(g * xhat) / dim))
 *   grad_x[r,d]   = (keep && x[r,d] * sc > 0) ? dy * sc : 0
 *   grad_gamma[d] = sum_r grad_out * xhat          grad_beta[d] = sum_r grad_out
 * in at most two launches, summed in a fixed order without atomics (bit-identical from run to
 * run).  Any of d_grad_x, d_grad_gamma, d_grad_beta may be NULL (skipped); d_partials is needed,
 * with at least the rows gf_layer_epilogue_backward_partial_rows gives, only when d_grad_gamma or
 * d_grad_beta is not NULL, and without them there is one launch.  num_rows == 0 zeroes the
 * parameter gradients given and launches nothing.  The checks of gf_layer_epilogue otherwise. */
GF_API int gf_layer_epilogue_backward(const float* d_x, const float* d_gamma,
                                      const float* d_mean, const float* d_rstd, size_t num_rows,
                                      size_t dim, float p, uint64_t seed,
                                      const float* d_grad_out, float* d_partials,
                                      size_t partial_rows, float* d_grad_x, float* d_grad_gamma,
                                      float* d_grad_beta, int device, void* stream);
/* gf_layer_epilogue and gf_layer_epilogue_backward for a bfloat16 d_x (uint16_t as above) and a
 * bfloat16 d_grad_x; d_gamma, d_beta, d_out, d_mean, d_rstd, d_grad_out, the partials, d_grad_gamma
 * and d_grad_beta stay float32.  Rows are widened on load, the arithmetic and its order are the
 * float32 entry points', and grad_x is rounded once to nearest even on store: every output equals
 * the float32 entry point's on the widened rows (grad_x: rounded to bfloat16), bit for bit.  The
 * same checks. */
GF_API int gf_layer_epilogue_bf16(const uint16_t* d_x, const float* d_gamma, const float* d_beta,
                                  size_t num_rows, size_t dim, float eps, float p, uint64_t seed,
                                  float* d_out, float* d_mean, float* d_rstd, int device,
                                  void* stream);
GF_API int gf_layer_epilogue_backward_bf16(const uint16_t* d_x, const float* d_gamma,
                                           const float* d_mean, const float* d_rstd,
                                           size_t num_rows, size_t dim, float p, uint64_t seed,
                                           const float* d_grad_out, float* d_partials,
                                           size_t partial_rows, uint16_t* d_grad_x,
                                           float* d_grad_gamma, float* d_grad_beta, int device,
                                           void* stream);

/* Fused gates of a GRU cell (torch.nn.GRUCell; the reference's TGN memory updater,
 * modules/memory_updater.py:62-85) behind its two GEMMs: d_gi = x W_ih^T + b_ih and d_gh = h W_hh^T
 * + b_hh [n, 3 * hidden], gate chunks in the order r, z, n, d_hx [n, hidden], row-major and
 * contiguous, fp32:
 *   r = 1 / (1 + expf(-(gi_r + gh_r)))      z = 1 / (1 + expf(-(gi_z + gh_z)))
 *   n = tanhf(gi_n + r * gh_n)              u = (1 - z) * n + z * hx
 *   out[i]  = u[i] (+ residual[i])          i < n
 *   last[i] = u[i]                          i < num_last       (never the residual)
 * in one launch that writes d_out [n, hidden] and d_last [num_last, hidden] (fp32) and nothing
 * else.  d_residual [n, hidden] may be NULL (none); it is fp32 when residual_bf16 == 0 and
 * bfloat16 (uint16_t as above, widened on load) when it is 1.  16-byte accesses when hidden % 4
 * == 0 and every pointer is 16-byte aligned, element by element otherwise; the bits do not depend
 * on which.  No pre-activation gives a NaN or an infinity.  hidden == 0, num_last > n,
 * residual_bf16 other than 0 or 1, 2^31 rows or 2^38 elements or more, or, with n > 0, a NULL
 * d_gi, d_gh, d_hx or d_out or a NULL d_last with num_last > 0: GF_ERR_INVALID_ARGUMENT; n == 0
 * launches nothing. */
GF_API int gf_gru_cell(const float* d_gi, const float* d_gh, const float* d_hx,
                       const void* d_residual, int residual_bf16, size_t n, size_t hidden,
                       size_t num_last, float* d_out, float* d_last, int device, void* stream);
/* Gradients of gf_gru_cell from g = d_grad_out [n, hidden] (fp32), with r, z, n recomputed from
 * d_gi, d_gh and d_hx by the forward's expressions:
 *   a_n = g * (1 - z) * (1 - n * n)      a_z = g * (hx - n) * z * (1 - z)
 *   a_r = a_n * gh_n * r * (1 - r)
 *   grad_gi = [a_r, a_z, a_n]      grad_gh = [a_r, a_z, a_n * r]      grad_hx = g * z
 * in one launch, without a reduction (bit-identical from run to run).  Any of d_grad_gi,
 * d_grad_gh [n, 3 * hidden] and d_grad_hx [n, hidden] may be NULL (skipped; all three: no
 * launch).  The gradient of the residual is d_grad_out itself.  The checks of gf_gru_cell. */
GF_API int gf_gru_cell_backward(const float* d_gi, const float* d_gh, const float* d_hx, size_t n,
                                size_t hidden, const float* d_grad_out, float* d_grad_gi,
                                float* d_grad_gh, float* d_grad_hx, int device, void* stream);
/* gf_gru_cell and gf_gru_cell_backward for bfloat16 d_gi and d_gh (uint16_t as above) and
 * bfloat16 d_grad_gi / d_grad_gh; d_hx, d_out, d_last, d_grad_out and d_grad_hx stay fp32.  Gates
 * are widened on load, the arithmetic and its order are the fp32 entry points', and grad_gi and
 * grad_gh are rounded once to nearest even on store: every output equals the fp32 entry point's
 * on the widened gates (grad_gi, grad_gh: rounded to bfloat16), bit for bit.  16-byte accesses
 * when hidden % 8 == 0, 8-byte gate accesses when hidden % 4 == 0, and the pointers are aligned
 * for them.  The same checks. */
GF_API int gf_gru_cell_bf16(const uint16_t* d_gi, const uint16_t* d_gh, const float* d_hx,
                            const void* d_residual, int residual_bf16, size_t n, size_t hidden,
                            size_t num_last, float* d_out, float* d_last, int device,
                            void* stream);
GF_API int gf_gru_cell_backward_bf16(const uint16_t* d_gi, const uint16_t* d_gh,
                                     const float* d_hx, size_t n, size_t hidden,
                                     const float* d_grad_out, uint16_t* d_grad_gi,
                                     uint16_t* d_grad_gh, float* d_grad_hx, int device,
                                     void* stream);

/* Link-prediction metrics of one validation batch from the scores d_pos [num_pos] of its true
 * edges and d_neg [num_neg] of its negative ones (float32, compared as IEEE compares them, so
 * -0 == +0): d_out[3] = {AP, AUC, MRR} as float64, what scikit-learn's average_precision_score
 * and roc_auc_score give for the concatenated scores with labels 1 / 0.  Nothing is sorted; with
 *   pge_i = #{j : pos[j] >= pos[i]}   nge_i = #{k : neg[k] >= pos[i]}
 *   nlt_i = #{k : neg[k] <  pos[i]}   neq_i = #{k : neg[k] == pos[i]}
 *   AP  = (1 / num_pos) sum_i pge_i / (pge_i + nge_i)
 *   AUC = (sum_i (2 nlt_i + neq_i)) / (2 num_pos num_neg)
 *   MRR = (1 / num_pos) sum_i 1 / (1 + gt_i + eq_i / 2)
 * where gt_i / eq_i count positive i's OWN negatives d_neg[k * num_pos + i], k < num_neg /
 * num_pos (the block layout of gf_edge_score), that are > / == d_pos[i]: the mean of the
 * optimistic and the pessimistic rank.  MRR is NaN when num_neg is not a multiple of num_pos.
 * Two launches on `stream`, no atomics, sums in a fixed order: the same inputs give the same
 * bits, and the host never waits.
 * d_acc (may be NULL) is a caller-owned running sum of 8 doubles: {sum_ap, sum_auc, sum_mrr,
 * batches, mrr_batches, nonfinite, reserved, reserved}.  A call adds its AP and AUC and 1 to
 * batches, and, when it has an MRR, the MRR and 1 to mrr_batches.  If any score is NaN or
 * infinite the three outputs are NaN, nonfinite grows by 1 and no other field changes.
 * d_partials: caller-owned scratch of rows * GF_LINK_METRICS_PARTIAL_WORDS 8-byte words, 8-byte
 * aligned, rows from gf_link_metrics_partial_rows(num_pos) (at most 256).  The scores pass
 * through LDS in tiles of GF_LINK_METRICS_TILE.  NULL d_pos, d_neg, d_partials or d_out,
 * num_pos == 0, num_neg == 0 or num_pos + num_neg > GF_LINK_METRICS_MAX_SCORES:
 * GF_ERR_INVALID_ARGUMENT. */
#define GF_LINK_METRICS_MAX_SCORES 65536
#define GF_LINK_METRICS_TILE 2048
#define GF_LINK_METRICS_PARTIAL_WORDS 4
GF_API int gf_link_metrics_partial_rows(size_t num_pos, size_t* rows);
GF_API int gf_link_metrics(const float* d_pos, const float* d_neg, size_t num_pos,
                           size_t num_neg, void* d_partials, size_t partial_rows, double* d_out,
                           double* d_acc, int device, void* stream);

/* Ranking with the edge score: d_src [num_src, dim] against ONE candidate set d_cand [num_cand,
 * dim] (both fp32, row-major, contiguous), d_w [dim], d_bias [1],
 *   score(i, c) = bias + sum_d w[d] * max(src[i, d] + cand[c, d], 0)
 * which is what gf_edge_score returns for that pair of rows, bit for bit (the same adds in the
 * same order), except that a NaN in src[i, d] + cand[c, d] stays a NaN.  Neither the pairs
 * [num_src * num_cand, dim] nor the scores [num_src, num_cand] are stored.  Per source i:
 *   d_values, d_indices [num_src, k]   the k best candidates, score descending, then candidate
 *       index ascending among equal scores; a NaN score sorts below -inf (by ascending index among
 *       NaNs) and is returned as NaN; a row with fewer than k candidates left ends in (-inf, -1).
 *   d_greater, d_equal [num_src]       the number of candidates with score > / == d_ref_score[i]
 *       (a NaN on either side: neither).  The rank of the reference is 1 + greater + equal / 2,
 *       the convention of gf_link_metrics.
 * Candidate d_skip[i] is left out of row i's counts and list; a value outside [0, num_cand)
 * excludes nothing.  d_ref_score NULL: no counts, d_greater and d_equal are not touched; k == 0:
 * no list; d_skip NULL: nothing skipped.  num_src == 0, or k == 0 without d_ref_score, launches
 * nothing.  Two launches on `stream`, no atomics, selection under a total order: the same inputs
 * give the same bits, and the host never waits.  16-byte loads when dim % 4 == 0 and d_src,
 * d_cand and d_w are 16-byte aligned, element loads otherwise, the same result either way.
 * d_scratch: caller-owned, 8-byte aligned, the bytes gf_edge_rank_scratch(num_src, num_cand, k)
 * gives.  A workgroup pass covers GF_EDGE_RANK_CHUNK candidates.  dim == 0, num_cand == 0 or
 * >= 2^31, k > min(num_cand, GF_EDGE_RANK_MAX_K): GF_ERR_INVALID_ARGUMENT. */
#define GF_EDGE_RANK_MAX_K 64
#define GF_EDGE_RANK_CHUNK 256
GF_API int gf_edge_rank_scratch(size_t num_src, size_t num_cand, size_t k, size_t* bytes);
GF_API int gf_edge_rank(const float* d_src, const float* d_cand, const float* d_w,
                        const float* d_bias, size_t num_src, size_t num_cand, size_t dim, size_t k,
                        const float* d_ref_score, const int64_t* d_skip, void* d_scratch,
                        size_t scratch_bytes, float* d_values, int64_t* d_indices,
                        int64_t* d_greater, int64_t* d_equal, int device, void* stream);
/* gf_edge_rank with a per-source set of candidates to leave out.  d_exclude: uint64
 * [num_src, W], W = ceil(num_cand / 64), row-major, contiguous; candidate c is left out of row
 * i's counts and list, exactly as d_skip[i] is, when bit c % 64 of word [i, c / 64] is set.
 * Bits at positions >= num_cand are ignored.  d_skip and d_exclude may both be given.  A row
 * with every candidate excluded gets a list of (-inf, -1) and zero counts.  d_exclude NULL is
 * gf_edge_rank, which forwards here with NULL; the scratch is gf_edge_rank_scratch's.  What
 * gf_graph_seen_mask writes is a d_exclude. */
GF_API int gf_edge_rank_masked(const float* d_src, const float* d_cand, const float* d_w,
                               const float* d_bias, size_t num_src, size_t num_cand, size_t dim,
                               size_t k, const float* d_ref_score, const int64_t* d_skip,
                               const uint64_t* d_exclude, void* d_scratch, size_t scratch_bytes,
                               float* d_values, int64_t* d_indices, int64_t* d_greater,
                               int64_t* d_equal, int device, void* stream);

/* The loss of a link-prediction step from the logits d_pos [num_pos] of its true edges and
 * d_neg [num_neg] of its negative ones: BCE-with-logits of d_pos against 1 plus that of d_neg
 * against 0, each a mean, as one float32 d_out[1].  With t(x) = log1p(exp(-|x|)):
 *   l_pos(x) = max(-x, 0) + t(x)        l_neg(y) = max(y, 0) + t(y)
 *   loss     = (1 / num_pos) sum_i l_pos(pos[i]) + (1 / num_neg) sum_j l_neg(neg[j])
 * Every term is float32 arithmetic; the two sums are float64, in an order that depends on
 * num_pos and num_neg alone; the loss is rounded to float32 once.  No atomics: the same inputs
 * give the same bits.  One launch on `stream` while ceil(num_pos / GF_LINK_LOSS_TILE) +
 * ceil(num_neg / GF_LINK_LOSS_TILE) <= GF_LINK_LOSS_SINGLE_TILES, two beyond; the host never
 * waits.
 * d_acc (may be NULL) is a caller-owned running sum of GF_LINK_LOSS_ACC_FIELDS doubles:
 * {sum_loss, sum_loss_times_num_pos, batches, nonfinite, sum_num_pos}.  A call adds its float32
 * loss, the loss times num_pos, 1, and num_pos.  A NaN logit gives a NaN loss; infinities follow
 * the formulas.  When the loss is not finite, nonfinite grows by 1 and no other field changes.
 * d_partials: caller-owned scratch of gf_link_loss_partial_rows(num_pos, num_neg) doubles (at
 * most GF_LINK_LOSS_MAX_PARTIAL_ROWS; 0 for the one-launch sizes, where it may be NULL).
 * gf_link_loss_backward writes d_grad_pos[i] = -s(-pos[i]) * d_grad_out[0] / num_pos and
 * d_grad_neg[j] = s(neg[j]) * d_grad_out[0] / num_neg, s the logistic function, in one launch;
 * d_grad_out is one float32 in device memory; a NULL d_grad_pos or d_grad_neg is not computed
 * (both NULL: nothing is launched).
 * The _bf16 forms take bfloat16 logits (widened on load, exact) and store bfloat16 gradients
 * (the float32 value rounded once, to nearest even); the loss is float32 and equals the float32
 * form's on the widened logits bit for bit.
 * NULL d_pos, d_neg, d_out or d_grad_out, num_pos == 0, num_neg == 0, a side of 2^31 logits or
 * more, or a d_partials that is missing or too small: GF_ERR_INVALID_ARGUMENT, nothing launched. */
#define GF_LINK_LOSS_TILE 1024
#define GF_LINK_LOSS_SINGLE_TILES 8
#define GF_LINK_LOSS_MAX_PARTIAL_ROWS 256
#define GF_LINK_LOSS_ACC_FIELDS 5
GF_API int gf_link_loss_partial_rows(size_t num_pos, size_t num_neg, size_t* rows);
GF_API int gf_link_loss(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                        double* d_partials, size_t partial_rows, float* d_out, double* d_acc,
                        int device, void* stream);
GF_API int gf_link_loss_backward(const float* d_pos, const float* d_neg, size_t num_pos,
                                 size_t num_neg, const float* d_grad_out, float* d_grad_pos,
                                 float* d_grad_neg, int device, void* stream);
GF_API int gf_link_loss_bf16(const uint16_t* d_pos, const uint16_t* d_neg, size_t num_pos,
                             size_t num_neg, double* d_partials, size_t partial_rows,
                             float* d_out, double* d_acc, int device, void* stream);
GF_API int gf_link_loss_backward_bf16(const uint16_t* d_pos, const uint16_t* d_neg,
                                      size_t num_pos, size_t num_neg, const float* d_grad_out,
                                      uint16_t* d_grad_pos, uint16_t* d_grad_neg, int device,
                                      void* stream);

/* One batch of an edge stream that lives in device memory, as the reference's utils.get_batch
 * lays it out, its negative destinations drawn on the device.  d_src, d_dst (int64) and d_time
 * (float32) are the num_rows rows of the stream, [lo, hi) the batch, B = hi - lo, K = neg_ratio,
 * d_dl the ascending list of distinct destinations and M = d_dl_count[0] its length, READ FROM
 * DEVICE MEMORY when the kernel runs (the set may have grown since without the host knowing):
 *   d_roots[0:B]          = d_src[lo:hi]
 *   d_roots[B:2B]         = d_dst[lo:hi]
 *   d_roots[2B + k*B + i] = d_dl[((uint64_t)u * M) >> 32]       k < K, i < B
 *   d_ts[j*B + i]         = d_time[lo + i]                      j < 2 + K
 *   u   = gf_philox4x32_10_first(seed, tid, epoch)              (gnnflow_rng.h)
 *   tid = (first_row + lo + i) * K + k                          (uint64, wrapping)
 * k-major: positive i's negatives are at stride B, the layout gf_link_metrics takes.  The key of
 * a draw is the GLOBAL row first_row + lo + i of the edge, so an edge gets the same negatives
 * whatever the batch borders are and whichever rank (each with the first_row of its slice)
 * assembles it.  The range reduction is one 32 x 32 -> 64 multiply, no modulo; as in the
 * reference a negative may equal the true destination.  M <= 0 or M >= 2^32: every negative is
 * -1.  The edge ids of the batch are d_eid[lo:hi] as they stand and need no kernel.
 * d_roots and d_ts hold (2 + K) * B elements.  One launch on `stream`, no atomics, every output
 * written once; 16-byte loads and stores where lo, B and the pointers allow, scalar otherwise.
 * lo == hi: nothing is launched.
 * d_src == NULL asks for the negatives alone (then d_dst, d_time and d_ts must be NULL too and
 * num_rows only bounds hi): d_roots[k*B + i], K * B elements, same tid.
 * gf_batch_assemble_many assembles num_batches consecutive batches in one launch: batch b is
 * [d_borders[b], d_borders[b + 1]) with the num_batches + 1 int64 borders in device memory, and
 * its slices of d_roots / d_ts start at element (2 + K) * (d_borders[b] - d_borders[0]), laid out
 * as above with its own B.  capacity: elements d_roots and d_ts each hold.  max_batch_rows sizes
 * the grid (a longer batch is still written in full).  A batch whose borders are not ascending,
 * negative, past num_rows, or whose slices would pass capacity writes nothing.
 * lo > hi, hi > num_rows, a NULL buffer that is needed, K > 0 with a NULL d_dl or d_dl_count,
 * K >= 65536, num_rows >= 2^44, num_batches >= 2^31: GF_ERR_INVALID_ARGUMENT, nothing launched. */
GF_API int gf_batch_assemble(const int64_t* d_src, const int64_t* d_dst, const float* d_time,
                             size_t num_rows, size_t lo, size_t hi, size_t neg_ratio,
                             const int64_t* d_dl, const int64_t* d_dl_count, uint64_t seed,
                             uint64_t epoch, uint64_t first_row, int64_t* d_roots, float* d_ts,
                             int device, void* stream);
GF_API int gf_batch_assemble_many(const int64_t* d_src, const int64_t* d_dst,
                                  const float* d_time, size_t num_rows, const int64_t* d_borders,
                                  size_t num_batches, size_t max_batch_rows, size_t neg_ratio,
                                  const int64_t* d_dl, const int64_t* d_dl_count, uint64_t seed,
                                  uint64_t epoch, uint64_t first_row, int64_t* d_roots,
                                  float* d_ts, size_t capacity, int device, void* stream);

/* The set of distinct destinations behind d_dl: a bitmap of num_nodes bits in
 * ceil(num_nodes / 64) 64-bit words (bit id % 64 of word id / 64), zeroed by the caller.
 * gf_dst_set_mark sets the bit of each of the n ids (atomic OR); an id outside [0, num_nodes)
 * sets nothing and adds 1 to d_out_of_range[0].  One launch; n == 0: none.
 * gf_dst_set_compact writes the set's ids in ascending order to d_ids and their number to
 * d_count[0] (what numpy.unique gives for everything marked so far): a popcount per tile of
 * GF_DST_SET_TILE_WORDS words, an exclusive scan of the tile counts by one workgroup, an emit
 * per tile; three launches on `stream`, no atomics, no kernel waits on another workgroup.  Ids
 * past ids_capacity are not written and d_count[0] is then ids_capacity.  d_scratch:
 * gf_dst_set_scratch_bytes(num_nodes) bytes, 8-byte aligned, caller-owned.
 * num_nodes >= 2^40, a NULL buffer that is needed, or a d_scratch that is too small or
 * misaligned: GF_ERR_INVALID_ARGUMENT, nothing launched. */
#define GF_DST_SET_TILE_WORDS 1024
GF_API int gf_dst_set_mark(const int64_t* d_ids, size_t n, uint64_t* d_bitmap, size_t num_nodes,
                           uint64_t* d_out_of_range, int device, void* stream);
GF_API int gf_dst_set_scratch_bytes(size_t num_nodes, size_t* bytes);
GF_API int gf_dst_set_compact(const uint64_t* d_bitmap, size_t num_nodes, int64_t* d_ids,
                              size_t ids_capacity, int64_t* d_count, void* d_scratch,
                              size_t scratch_bytes, int device, void* stream);

/* Historical negatives: one launch overwrites the first Kh = hist_ratio negative planes of
 * batches that gf_batch_assemble[_many] has already written.  A slot is overwritten only where
 * a historical negative exists.  A slot without one keeps the random draw it already holds, so
 * the fall-back costs nothing and no slot is left undefined.  Every other element stays
 * bit-identical: the src and dst planes, the negative planes k >= Kh, and all of ts.
 *
 * Inputs per slot.  The slot belongs to batch-local row i with global row
 * g = first_row + lo + i.  It has source s, true destination d, time t, and index
 * k < Kh <= K.
 *
 * History size c.
 * - Let e = table[s].
 * - c is the number of elements x in ts_pool[e.start .. e.start + e.size) with x < t.
 * - The comparison is strict and uses the float < operator, so a NaN t gives c = 0.
 * - c counts only the live range, that is, what offload_old_blocks has left.
 * - If s < 0, s >= table_len or c == 0, the slot is kept.
 *
 * Draw.  For attempts a = 0 .. GF_HIST_NEG_ATTEMPTS - 1 (4 attempts):
 * - u = gf_philox4x32_10_first(seed ^ (GF_HIST_NEG_SEED_TAG + a), tid, epoch).
 * - tid = g * K + k, wrapping, as in gf_batch_assemble.
 * - j = (uint64(u) * c) >> 32.
 * - cand = nbr_pool[e.start + j].dst.
 * - Index j counts from the node's oldest live edge in the store's order.  That order is the
 *   reverse of what get_temporal_neighbors returns.
 * - The first attempt with cand != d is written to roots[2B + k*B + i].  If all four attempts
 *   fail, the slot is kept.
 *
 * Documented consequences.
 * - Draws are with replacement.
 * - A historical negative may be a destination of another edge of s at time t.
 * - On a graph built with reverse edges the history includes nodes that pointed at s.
 *
 * table, ts_pool and nbr_pool are the node table and the two pools of the graph's temporal edge
 * store (one contiguous, chronologically sorted segment per node).  GF_HIST_NEG_SEED_TAG keeps
 * the historical draws independent of the random ones of the same tid; hist_ratio == 0 draws
 * nothing, so what gf_batch_assemble wrote stands.
 *
 * d_src, d_dst, d_time, num_rows, d_borders, num_batches, max_batch_rows, neg_ratio, seed,
 * epoch, first_row, d_roots and capacity are those of the gf_batch_assemble_many call that wrote
 * the batches (a single batch: num_batches = 1 and d_borders advanced to its two borders; a
 * batch written by gf_batch_assemble: the same with capacity = (2 + K) * B).  A batch with bad
 * borders, or one whose slices would pass capacity, writes nothing, as there.  d_filled: NULL,
 * or a device uint64 to which the number of slots overwritten is ADDED (one atomic add per
 * workgroup; zero it yourself).  One launch on `stream`, which must be the stream of the
 * assemble call or ordered behind it.
 * Ordering against ingest: the call takes the graph's device view (table and pool addresses,
 * table length) when it is made, as gf_sampler_sample does.  gf_graph_add_edges and
 * gf_graph_offload_old_blocks run on the graph's own stream and return with the device state
 * complete, so a call made after they return sees their edges without further ordering.  They
 * move segments that fill, reuse freed ones and may reallocate the table and the pools: every
 * earlier launch of this call must have COMPLETED (stream synchronised, or an event waited for
 * on the host) before either of them is called, and the graph must outlive the launch.
 * A NULL graph, a NULL buffer that is needed, hist_ratio > neg_ratio, neg_ratio >= 65536,
 * num_rows >= 2^44, num_batches >= 2^31: GF_ERR_INVALID_ARGUMENT, nothing launched.
 * hist_ratio == 0 or num_batches == 0: GF_OK, nothing launched. */
#define GF_HIST_NEG_ATTEMPTS 4
#define GF_HIST_NEG_SEED_TAG 0x484953544E454730ULL /* "HISTNEG0" */
GF_API int gf_batch_hist_negatives(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                                   const float* d_time, size_t num_rows,
                                   const int64_t* d_borders, size_t num_batches,
                                   size_t max_batch_rows, size_t neg_ratio, size_t hist_ratio,
                                   uint64_t seed, uint64_t epoch, uint64_t first_row,
                                   int64_t* d_roots, size_t capacity, uint64_t* d_filled,
                                   int device, void* stream);

/* Which of num_cand candidate nodes has each of num_rows sources already met.  Row i has source
 * s = d_src[i] and time t = d_ts[i].  Its considered edges:
 * - e = table[s]; c = the number of x in ts_pool[e.start .. e.start + e.size) with x < t, strict
 *   and with the float < operator (a NaN t gives c = 0), over the live range only, as in
 *   gf_batch_hist_negatives;
 * - n = c, or min(c, max_history) when max_history > 0: the NEWEST n of those c edges,
 *   nbr_pool[e.start + c - n .. e.start + c).
 * The candidates are given sorted: d_sorted_ids [num_cand] ascending (duplicates allowed, ids
 * unknown to the graph allowed) and d_perm [num_cand], the position of each in the caller's own
 * order (what a sort returns as its permutation; an entry outside [0, num_cand) sets nothing).
 * For every considered edge and every j with d_sorted_ids[j] == its dst, bit d_perm[j] % 64 of
 * word d_mask[i * W + d_perm[j] / 64] is set, W = ceil(num_cand / 64).  d_mask is uint64
 * [num_rows, W] and must be ZEROED by the caller: bits are ORed in (atomic OR on the words, the
 * only atomic; the same inputs give the same bits) and bits at positions >= num_cand are never
 * set.  s < 0, s >= table_len or c == 0: the row is not touched.  On a graph built with reverse
 * edges the history includes nodes that pointed at s.  The layout is gf_edge_rank_masked's
 * d_exclude.
 * One launch on `stream`, plain loads, a wave per row; the cost is proportional to the edges
 * considered (a hub's whole history when max_history == 0).  Ordering against
 * gf_graph_add_edges / gf_graph_offload_old_blocks: as gf_batch_hist_negatives.
 * A NULL graph, a NULL buffer with num_rows > 0, num_cand == 0 or >= 2^31, num_rows >= 2^31:
 * GF_ERR_INVALID_ARGUMENT, nothing launched.  num_rows == 0: GF_OK, nothing launched. */
GF_API int gf_graph_seen_mask(const gf_graph* g, const int64_t* d_src, const float* d_ts,
                              size_t num_rows, const int64_t* d_sorted_ids, const int64_t* d_perm,
                              size_t num_cand, size_t max_history, uint64_t* d_mask, int device,
                              void* stream);

/* Has each of num_rows (source, destination) pairs interacted before the row's time, how often,
 * and when last.  Row i has source s = d_src[i], destination d = d_dst[i], time t = d_ts[i] and,
 * when d_since is not NULL, lower end lo = d_since[i].  Its considered edges:
 * - e = table[s]; c = the number of x in ts_pool[e.start .. e.start + e.size) with x < t, strict
 *   and with the float < operator (a NaN t gives c = 0), over the live range only, as in
 *   gf_batch_hist_negatives;
 * - c0 = 0, or with d_since min(c, the number of x with x < lo), the same operator: a NaN lo
 *   gives c0 = 0, no lower end, and the lower end is inclusive (lo equal to an edge's time keeps
 *   that edge);
 * - n = c - c0, or min(c - c0, max_history) when max_history > 0: the NEWEST n edges of the
 *   window, nbr_pool[e.start + c - n .. e.start + c), that is lo <= ts < t.
 * Then
 *   d_count[i]    = the number of considered edges whose dst == d              int64
 *   p             = the largest pool position among them
 *   d_last_ts[i]  = nbr_pool[p].ts,  -infinity when d_count[i] == 0            float32
 *   d_last_eid[i] = nbr_pool[p].eid, -1 when d_count[i] == 0                   int64
 * Among matching edges with the same timestamp the last is the latest in the store's order, the
 * first match in gf_graph_get_temporal_neighbors' newest-first list.  Any d is legal (negative,
 * unknown to the graph): it matches nothing.  s < 0, s >= table_len, no live edge, c == 0 or a
 * store without a node: 0, -infinity, -1.  Every element of the three outputs ([num_rows] each)
 * is written: they need no initialisation.  On a graph built with reverse edges the history
 * includes edges that pointed at s, so without max_history the answer is symmetric in (s, d).
 * One launch on `stream`, plain loads and stores, a wave per row, integer cross-lane reductions,
 * no atomics: the same inputs give the same bits.  The cost is proportional to the edges
 * considered (a hub's whole history when max_history == 0 and d_since == NULL); max_history
 * > 2^32 - 1 is no bound.  Ordering against gf_graph_add_edges / gf_graph_offload_old_blocks: as
 * gf_batch_hist_negatives.
 * A NULL graph, a NULL buffer other than d_since with num_rows > 0, num_rows >= 2^31:
 * GF_ERR_INVALID_ARGUMENT, nothing launched.  num_rows == 0: GF_OK, nothing launched. */
GF_API int gf_graph_pair_history(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                                 const float* d_ts, const float* d_since /* NULL: no lower end */,
                                 size_t num_rows, size_t max_history,
                                 int64_t* d_count, float* d_last_ts, int64_t* d_last_eid,
                                 int device, void* stream);

/* Which nodes have BOTH ends of each of num_rows pairs met before the row's time.  Row i has
 * source s = d_src[i], destination d = d_dst[i], time t = d_ts[i] and, when d_since is not NULL,
 * lower end lo = d_since[i].  The window of a node v is gf_graph_pair_history's:
 * - e = table[v]; c = the number of x in ts_pool[e.start .. e.start + e.size) with x < t, strict
 *   and with the float < operator (a NaN t gives c = 0), over the live range only;
 * - c0 = 0, or with d_since min(c, the number of x with x < lo), the same operator: a NaN lo
 *   gives c0 = 0, and the lower end is inclusive;
 * - n = min(c - c0, H), H = max_history, which is REQUIRED here, 1 <= H <= GF_CN_MAX_HISTORY: it
 *   bounds the table a row is intersected in;
 * - the window's records are nbr_pool[e.start + c - n .. e.start + c), at positions 0 .. n - 1,
 *   oldest first;
 * - v < 0, v >= table_len, no live edge or a store without a node: the window is empty.
 * A is the window of s, B the window of d, both at the same t and lo.  A record whose dst is
 * negative counts as an edge but is nobody's neighbour.  For z >= 0, a(z) and b(z) are the
 * numbers of records of A and of B with dst == z, and pa(z) is the largest position in A that
 * holds z.  With K = max_common, 0 <= K <= GF_CN_MAX_HISTORY:
 *   d_n_src[i], d_n_dst[i] = |A|, |B|: edges, multi-edges counted               int32 [num_rows]
 *   d_u_src[i], d_u_dst[i] = #{z : a(z) > 0}, #{z : b(z) > 0}                   int32 [num_rows]
 *   d_common[i]            = #{z : a(z) > 0 and b(z) > 0}, not capped by K      int32 [num_rows]
 *   d_nodes[i, :]          = those z by DESCENDING pa(z) -- the one the source met most recently
 *                            first --, the first min(d_common[i], K), then -1   int64 [num_rows, K]
 *   d_cnt_src[i, k], d_cnt_dst[i, k] = a(z), b(z) of z = d_nodes[i, k]; 0 in the padding
 *                                                                               int32 [num_rows, K]
 * Every element of the eight outputs, row-major and contiguous, is written: they need no
 * initialisation.  s == d is legal: every neighbour is then common.  The endpoints themselves are
 * not removed from the sets: on a graph built with reverse edges a pair that has interacted has
 * d among the neighbours of s.
 * One launch on `stream`: a row's two windows are inserted into an open-addressing table in LDS
 * (at most 2H keys in >= 4H slots; a probe that finds no place after as many trips as there are
 * slots drops its record, which cannot happen at that load) with LDS atomics on integers, counted
 * with integer cross-lane sums, and the common nodes are placed by their rank among A's
 * positions, one writer per element, no atomics on global memory: the same inputs give the same
 * bits.  The cost is the 2H records read per row.  Ordering against gf_graph_add_edges /
 * gf_graph_offload_old_blocks: as gf_batch_hist_negatives.
 * A NULL graph, a NULL buffer other than d_since with num_rows > 0 (d_nodes, d_cnt_src and
 * d_cnt_dst may be NULL when K == 0), max_history outside [1, GF_CN_MAX_HISTORY], max_common >
 * GF_CN_MAX_HISTORY, num_rows >= 2^31: GF_ERR_INVALID_ARGUMENT, nothing launched.
 * num_rows == 0: GF_OK, nothing launched. */
#define GF_CN_MAX_HISTORY 512
GF_API int gf_graph_common_neighbors(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                                     const float* d_ts,
                                     const float* d_since /* NULL: no lower end */,
                                     size_t num_rows, size_t max_history, size_t max_common,
                                     int32_t* d_n_src, int32_t* d_n_dst, int32_t* d_u_src,
                                     int32_t* d_u_dst, int32_t* d_common, int64_t* d_nodes,
                                     int32_t* d_cnt_src, int32_t* d_cnt_dst, int device,
                                     void* stream);

/* d_out[i] = c - c0 of the window of node d_nodes[i] at time d_ts[i] and lower end d_since[i]
 * (NULL: none) as defined for gf_graph_common_neighbors, without max_history: the number of live
 * edges of the node with lo <= ts < t, int64 [num].  A node that is negative (the -1 padding of
 * d_nodes above), past the node table or without live edges gives 0.  Every element is written.
 * One launch on `stream`, a lane per element, plain loads and stores.
 * A NULL graph, a NULL buffer other than d_since with num > 0, num >= 2^31:
 * GF_ERR_INVALID_ARGUMENT, nothing launched.  num == 0: GF_OK, nothing launched. */
GF_API int gf_graph_temporal_degree(const gf_graph* g, const int64_t* d_nodes, const float* d_ts,
                                    const float* d_since /* NULL: no lower end */, size_t num,
                                    int64_t* d_out, int device, void* stream);

/* The pair inputs of the sequence-based temporal models (DyGFormer, GraphMixer): the most recent
 * interactions of both ends of each of num_rows pairs as two padded sequences of node id, edge id
 * and time, and for every element of either sequence how often that node occurs in the source's
 * sequence and how often in the destination's (DyGFormer's neighbour co-occurrence encoding).
 * Row i has source s = d_src[i], destination d = d_dst[i], time t = d_ts[i] and, when d_since is
 * not NULL, lower end lo = d_since[i].  With L = length (slots per side) and self = 1 when
 * include_self != 0, else 0:
 *   H        = L - self, the bound of the window, 1 <= H <= GF_COOC_MAX_LENGTH - self
 *   W(v)     = the window of node v at (t, lo, H) exactly as defined for
 *              gf_graph_common_neighbors (strictly before t, lo inclusive, the newest H, a NaN t
 *              gives none, a NaN lo is no lower end; empty for v < 0, v >= table_len, no live
 *              edge or a store without a node), oldest first, n(v) = |W(v)| <= H
 *   seq(v)   = [v itself if self] followed by the dst of W(v)'s records; len(v) = self + n(v) <= L
 *   a(z), b(z) = how often z occurs in seq(s), in seq(d), for z >= 0
 * Side 0 is s's and side 1 is d's.  All outputs are row-major and contiguous, and every element
 * is written, so they need no initialisation:
 *   d_lengths int32   [num_rows, 2]        len(s), len(d)
 *   d_nodes   int64   [num_rows, 2, L]     seq(v), then -1
 *   d_eids    int64   [num_rows, 2, L]     the records' eid; -1 for the self slot and the padding
 *   d_times   float32 [num_rows, 2, L]     the records' ts, bits copied; t for the self slot (also
 *                                          when t is NaN); 0 in the padding
 *   d_counts  int32   [num_rows, 2, L, 2]  [.., p, 0] = a(d_nodes[.., p]), [.., p, 1] =
 *                                          b(d_nodes[.., p]); 0, 0 in the padding
 * - Self slot.  With include_self the self slot is present whatever the node is (negative,
 *   unknown to the graph, without edges): it is what DyGFormer puts at position 0, and it counts
 *   as one occurrence of v in seq(v).
 * - Negative ids.  A negative id, the self slot's or a stored destination's, is nobody's
 *   neighbour: it is not counted and its own counts are 0, 0, as in gf_graph_common_neighbors.
 *   d_lengths tells it apart from the padding.
 * - s == d is legal; both sides are then equal, and a == b.
 * - Channel 0 is "in the source's sequence" on BOTH sides.
 * - H == 0 does not exist: length >= 1 + self is required.
 * One launch on `stream`: a row's two sequences are inserted into an open-addressing table in LDS
 * (at most 2L keys in >= 4L slots; a probe that finds no place after as many trips as there are
 * slots drops its element, which cannot happen at that load) with LDS atomics on integers, then
 * every position of both sequences is written with its two counts, one writer per element, no
 * atomics on global memory: the same inputs give the same bits.  The cost is the 2H records read
 * twice per row.  d_counts must be 8-byte aligned (a position's two counts are one store).
 * Ordering against gf_graph_add_edges / gf_graph_offload_old_blocks: as gf_batch_hist_negatives.
 * A NULL graph, a NULL buffer other than d_since with num_rows > 0, length outside
 * [1 + self, GF_COOC_MAX_LENGTH], a misaligned d_counts, num_rows >= 2^31:
 * GF_ERR_INVALID_ARGUMENT, nothing launched.  num_rows == 0: GF_OK, nothing launched. */
#define GF_COOC_MAX_LENGTH 512
GF_API int gf_graph_neighbor_cooccurrence(const gf_graph* g, const int64_t* d_src,
                                          const int64_t* d_dst, const float* d_ts,
                                          const float* d_since /* NULL: no lower end */,
                                          size_t num_rows, size_t length, int include_self,
                                          int32_t* d_lengths, int64_t* d_nodes, int64_t* d_eids,
                                          float* d_times, int32_t* d_counts, int device,
                                          void* stream);

/* The features of what each of num_rows nodes met before the row's time, summed or averaged over
 * its history window: GraphMixer's node encoder input and windowed mean pooling.  Row i has node
 * v = d_nodes[i], time t = d_ts[i] and, when d_since is not NULL, lower end lo = d_since[i].  Its
 * considered records are the window of v at (t, lo, max_history) exactly as defined for
 * gf_graph_pair_history:
 * - e = table[v]; c = the number of x in ts_pool[e.start .. e.start + e.size) with x < t, strict
 *   and with the float < operator (a NaN t gives c = 0), over the live range only;
 * - c0 = 0, or with d_since min(c, the number of x with x < lo), the same operator: a NaN lo
 *   gives c0 = 0, and the lower end is inclusive;
 * - n = c - c0, or min(c - c0, max_history) when max_history > 0: the NEWEST n edges of the
 *   window, seg = nbr_pool[e.start + c - n .. e.start + c), oldest first;
 * - v < 0, v >= table_len, no live edge or a store without a node: n = 0.
 * With N = d_node_feats (float32 [node_rows, dn], row-major and contiguous), E = d_edge_feats
 * (float32 [edge_rows, de]) and N[id, :], E[id, :] the ZERO row for an id without a row in its
 * table (id < 0 or id >= node_rows / edge_rows):
 *   d_count[i]       = n                                                          int64 [num_rows]
 *   d_node_out[i, c] = (((+0.0f + N[seg[0].dst, c]) + N[seg[1].dst, c]) + ...) + N[seg[n-1].dst, c]
 *                                                                           float32 [num_rows, dn]
 *   d_edge_out[i, c] = the same over E[seg[x].eid, c]                       float32 [num_rows, de]
 * in float32, one addition per record in window order.  With mean != 0 that sum is then divided
 * once by (float)n with a correctly rounded IEEE division, not multiplied by a reciprocal; where
 * n == 0 the result is zeros.  A record without a row adds nothing and still counts in n (the
 * rule of unknown ids in the TGN memory's input).  Either table may be absent, as NULL with width
 * 0 (its output is then not touched and may be NULL), but not both.  Widths are
 * 1 .. GF_AGG_MAX_WIDTH.  Every element of d_count and of the outputs of the given tables is
 * written, the rows with an empty window too: they need no initialisation.  On a graph built
 * with reverse edges the window includes the edges that pointed at v.
 * One launch on `stream`: a wave per row, the lanes own columns (float4 columns when the width is
 * a multiple of 4 and the table and its output are 16-byte aligned), every output element is
 * written by one lane whose additions run in window order, plain loads and stores, no LDS, no
 * atomics: the same inputs give the same bits, and they are the bits of a sequential float32
 * loop.  The cost is the rows read (a hub's whole history when max_history == 0 and d_since ==
 * NULL, walked by one wave); max_history > 2^32 - 1 is no bound.  Ordering against
 * gf_graph_add_edges / gf_graph_offload_old_blocks: as gf_batch_hist_negatives (reads the store's
 * view NOW).
 * A NULL graph, no table at all, a NULL table with a width other than 0, a width outside
 * [1, GF_AGG_MAX_WIDTH] of a table that is given, num_rows >= 2^31, and with num_rows > 0 a NULL
 * d_nodes, d_ts, d_count or output of a given table: GF_ERR_INVALID_ARGUMENT, nothing launched.
 * num_rows == 0: GF_OK, nothing launched. */
#define GF_AGG_MAX_WIDTH 1024
GF_API int gf_graph_neighbor_aggregate(const gf_graph* g, const int64_t* d_nodes,
                                       const float* d_ts,
                                       const float* d_since /* NULL: no lower end */,
                                       size_t num_rows, size_t max_history,
                                       const float* d_node_feats /* NULL: no node table */,
                                       size_t node_rows, size_t dn,
                                       const float* d_edge_feats /* NULL: no edge table */,
                                       size_t edge_rows, size_t de, int mean, int64_t* d_count,
                                       float* d_node_out, float* d_edge_out, int device,
                                       void* stream);

/* The newest interactions of each of num_rows nodes as one padded sequence, and optionally the
 * finished tokens a sequence model reads from it (GraphMixer's link encoder, DyGFormer, TCL): the
 * per-node reader, where gf_graph_neighbor_cooccurrence reads the two ends of a pair.  Row i has
 * node v = d_nodes[i], time t = d_ts[i] and, when d_since is not NULL, lower end lo = d_since[i].
 * With L = length, its records are the window of v at (t, lo, L) exactly as defined for
 * gf_graph_neighbor_aggregate with max_history = L (strictly before t, lo inclusive, the newest L,
 * a NaN t gives none, a NaN lo is no lower end; empty for v < 0, v >= table_len, no live edge or
 * a store without a node): seg[0 .. n), oldest first, n <= L.  All outputs are row-major and
 * contiguous, and every element is written, so they need no initialisation:
 *   d_lengths   int32   [num_rows]        n
 *   d_out_nodes int64   [num_rows, L]     seg[p].dst for p < n, then -1
 *   d_eids      int64   [num_rows, L]     seg[p].eid for p < n, then -1
 *   d_times     float32 [num_rows, L]     seg[p].ts for p < n, bits copied, then 0
 *   d_delta_t   float32 [num_rows, L]     t - seg[p].ts for p < n, one float32 subtraction, then 0
 *   d_tokens    float32 [num_rows, L, de + dn + dim_time], for p < n
 *                 [0, de)            d_edge_feats[seg[p].eid, :]   (float32 [edge_rows, de])
 *                 [de, de + dn)      d_node_feats[seg[p].dst, :]   (float32 [node_rows, dn])
 *                 de + dn + j        cosf(d_weight[j] * d_delta_t[i, p] + d_bias[j]), j < dim_time
 *               and +0.0 in every element, the time part too, for p >= n
 * which is gf_graph_neighbor_cooccurrence's side 0 with include_self == 0, element for element,
 * in the first four.  The table parts are copies of the rows, bit for bit; an id without a row in
 * its table (id < 0 or id >= edge_rows / node_rows) gives a zero part, the rule of
 * gf_graph_neighbor_aggregate.  The time part is gf_time_encode_cat's expression evaluated by the
 * same code (one multiply, one add, the precise cosf): it equals that call on d_delta_t bit for
 * bit.  Each of the three parts may be absent, as NULL with width 0 (d_weight and d_bias are
 * given together); without any part d_tokens is not touched and may be NULL.  Tables are
 * row-major and contiguous; widths are 1 .. GF_SEQ_MAX_WIDTH, length is 1 .. GF_SEQ_MAX_LENGTH.
 * On a graph built with reverse edges the window includes the edges that pointed at v.
 * One launch on `stream`: a wave per row; the lanes stride over the L positions for the four
 * planes (one 32-byte record read per filled position) and over the flattened (position, column)
 * space of each part for the tokens (float4 columns when every given width is a multiple of 4 and
 * the tables and d_tokens are 16-byte aligned, scalar columns otherwise), one writer per element,
 * plain loads and stores, no LDS, no atomics: the same inputs give the same bits.  Index
 * arithmetic on [num_rows, L, width] is 64-bit.  Ordering against gf_graph_add_edges /
 * gf_graph_offload_old_blocks: as gf_batch_hist_negatives (reads the store's view NOW).
 * A NULL graph, length outside [1, GF_SEQ_MAX_LENGTH], a NULL part with a width other than 0, a
 * width outside [1, GF_SEQ_MAX_WIDTH] of a part that is given, only one of d_weight and d_bias,
 * num_rows >= 2^31, and with num_rows > 0 a NULL d_nodes, d_ts, d_lengths, d_out_nodes, d_eids,
 * d_times or d_delta_t, or a NULL d_tokens when a part is given: GF_ERR_INVALID_ARGUMENT, nothing
 * launched.  num_rows == 0: GF_OK, nothing launched. */
#define GF_SEQ_MAX_LENGTH 512
#define GF_SEQ_MAX_WIDTH 1024
GF_API int gf_graph_neighbor_sequence(const gf_graph* g, const int64_t* d_nodes, const float* d_ts,
                                      const float* d_since /* NULL: no lower end */,
                                      size_t num_rows, size_t length,
                                      const float* d_edge_feats /* NULL: no edge table */,
                                      size_t edge_rows, size_t de,
                                      const float* d_node_feats /* NULL: no node table */,
                                      size_t node_rows, size_t dn,
                                      const float* d_weight /* NULL: no time part */,
                                      const float* d_bias, size_t dim_time, int32_t* d_lengths,
                                      int64_t* d_out_nodes, int64_t* d_eids, float* d_times,
                                      float* d_delta_t, float* d_tokens, int device, void* stream);

/* Everything DyGFormer concatenates for each of num_rows pairs, finished, from one launch: the
 * pair reader with features, where gf_graph_neighbor_sequence is the per-node one.  Row i has
 * source s = d_src[i], destination d = d_dst[i], time t = d_ts[i] and, when d_since is not NULL,
 * lower end lo = d_since[i]; side 0 is s's sequence, side 1 d's, L = length slots each.  All
 * outputs are row-major and contiguous, and every element is written:
 *   d_lengths, d_nodes, d_eids, d_times, d_counts
 *               gf_graph_neighbor_cooccurrence's at (d_src, d_dst, d_ts, d_since, length,
 *               include_self = 1), element for element and bit for bit: the self slot is
 *               position 0 with eid -1 and time t and is counted, the window behind it has the
 *               bound L - 1, oldest first, the padding is -1, -1, 0, (0, 0)
 *   d_delta_t   float32 [num_rows, 2, L]   t - d_times[i, side, p], one float32 subtraction, on
 *               every filled slot, the self slot included (t - t); +0.0 in the padding
 *   d_node_out  float32 [num_rows, 2, L, dn]        d_node_feats[d_nodes[i, side, p], :]
 *   d_edge_out  float32 [num_rows, 2, L, de]        d_edge_feats[d_eids[i, side, p], :]
 *   d_time_out  float32 [num_rows, 2, L, dim_time]  cosf(d_weight[j] * d_delta_t[i, side, p] + d_bias[j])
 *               on a filled slot, and +0.0 in every element of a padded slot of the three
 * The table parts are copies of the rows, bit for bit; an id without a row in its table (id < 0
 * or id >= node_rows / edge_rows) gives a zero part, the rule of gf_graph_neighbor_aggregate: the
 * self slot has the node's own row in d_node_out and a zero row in d_edge_out.  The time part is
 * gf_time_encode_cat's expression evaluated by the same code (one multiply, one add, the precise
 * cosf): it equals that call on d_delta_t bit for bit, the self slot being the encoding of its
 * own delta.  Each of the three parts is its own tensor and may be absent, as NULL with width 0
 * (d_weight and d_bias are given together); the output of an absent part is not touched and may
 * be NULL.  Tables are row-major and contiguous; widths are 1 .. GF_PAIRSEQ_MAX_WIDTH, length is
 * 2 .. GF_PAIRSEQ_MAX_LENGTH.
 * One launch on `stream`: gf_graph_neighbor_cooccurrence's geometry, LDS table and phases (a wave
 * per row up to L = 128, four waves on a row above), the emit writing the six planes; behind it
 * the row's threads are spread over the flattened (side, position, column) space of each part
 * (float4 columns where that part's width is a multiple of 4 and its table and output are 16-byte
 * aligned, scalar columns otherwise, decided per part), one writer per element, plain loads and
 * stores, no atomics on global memory: the same inputs give the same bits.  Index arithmetic on
 * [num_rows, 2, L, width] is 64-bit.  d_counts must be 8-byte aligned.  Ordering against
 * gf_graph_add_edges / gf_graph_offload_old_blocks: as gf_batch_hist_negatives (reads the store's
 * view NOW).
 * A NULL graph, length outside [2, GF_PAIRSEQ_MAX_LENGTH], a NULL part with a width other than
 * 0, a width outside [1, GF_PAIRSEQ_MAX_WIDTH] of a part that is given, only one of d_weight and
 * d_bias, num_rows >= 2^31, and with num_rows > 0 a NULL d_src, d_dst, d_ts or plane, a
 * misaligned d_counts, or a NULL output of a part that is given: GF_ERR_INVALID_ARGUMENT, nothing
 * launched.  num_rows == 0: GF_OK, nothing launched. */
#define GF_PAIRSEQ_MAX_LENGTH 512
#define GF_PAIRSEQ_MAX_WIDTH 1024
GF_API int gf_graph_pair_sequence(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                                  const float* d_ts,
                                  const float* d_since /* NULL: no lower end */,
                                  size_t num_rows, size_t length,
                                  const float* d_node_feats /* NULL: no node table */,
                                  size_t node_rows, size_t dn,
                                  const float* d_edge_feats /* NULL: no edge table */,
                                  size_t edge_rows, size_t de,
                                  const float* d_weight /* NULL: no time part */,
                                  const float* d_bias, size_t dim_time, int32_t* d_lengths,
                                  int64_t* d_nodes, int64_t* d_eids, float* d_times,
                                  float* d_delta_t, int32_t* d_counts, float* d_node_out,
                                  float* d_edge_out, float* d_time_out, int device, void* stream);

/* Backward-in-time random walks over the temporal edge store: W = num_walks walks of L = length
 * steps from each of num_rows roots.  Walk (i, w) starts at v_0 = d_src[i], t_0 = d_ts[i];
 * d_nodes[i, w, 0] = d_src[i] always.  Step j = 0 .. L - 1:
 * - v_j outside [0, table_len): the walk has ended.
 * - e = table[v_j]; c = the number of x in ts_pool[e.start .. e.start + e.size) with x < t_j,
 *   strict and with the float < operator (a NaN t_j gives c = 0), over the live range only, as in
 *   gf_batch_hist_negatives.
 * - n = c, or min(c, max_history) when max_history > 0: the NEWEST n of those c edges.  n == 0:
 *   the walk has ended.
 * - u_a = gf_philox4x32_10_first(seed ^ (GF_WALK_SEED_TAG + a), tid, (epoch << 8) + j) for
 *   a < recency, tid = (first_row + i) * W + w; both words wrap mod 2^64.
 * - x = the maximum over a of (uint64(u_a) * n) >> 32, so 0 <= x < n.
 * - r = nbr_pool[e.start + (c - n) + x]: index 0 is the oldest edge considered, as in
 *   gf_batch_hist_negatives (the reverse of get_temporal_neighbors' order).
 * - d_nodes[i, w, j + 1] = r.dst, d_eids[i, w, j] = r.eid, d_times[i, w, j] = r.ts;
 *   v_{j+1} = r.dst, t_{j+1} = r.ts.
 * Every slot from the step a walk ends on holds d_nodes = -1, d_eids = -1, d_times = 0.  Every
 * element of d_nodes (int64 [num_rows, W, L + 1]), d_eids (int64 [num_rows, W, L]) and d_times
 * (float32 [num_rows, W, L]), row-major and contiguous, is written: they need no initialisation.
 *
 * Documented consequences.
 * - Time strictly decreases along a walk: no edge is taken twice, an edge at the current time
 *   (a tie) is never followed, and a walk from a NaN time ends on step 0.
 * - recency == 1 is a uniform draw from the n edges considered; recency == p is the maximum of
 *   p uniform draws, P(x <= k) = ((k + 1) / n)^p: a power-law preference for recent edges, in
 *   integer arithmetic only.
 * - A walk is keyed by its root's GLOBAL row first_row + i, not by its place in the call: rows
 *   [a, b) walked with first_row = a are rows a .. b of everything walked with first_row = 0.
 * - GF_WALK_SEED_TAG keeps the draws independent of gf_batch_assemble's and
 *   gf_batch_hist_negatives' draws of the same tid.
 * - The recency draws of a step are keyed seed ^ (GF_WALK_SEED_TAG + a).  Two seeds whose XOR is
 *   the XOR of two of those tags (it fits the low five bits) key the same draws in another order,
 *   and the maximum does not see the order: seeds that are meant to give independent walks must
 *   differ above their low five bits.
 * - On a graph built with reverse edges a walk also follows edges that pointed at its node.
 * - A store without a node gives walks that all end on step 0.
 *
 * One launch on `stream`, one lane per walk, plain loads and stores, no atomics: the same inputs
 * give the same bits.  Ordering against gf_graph_add_edges / gf_graph_offload_old_blocks: as
 * gf_batch_hist_negatives.
 * A NULL graph, a NULL buffer with num_rows > 0, length outside [1, GF_WALK_MAX_LENGTH],
 * num_walks outside [1, 65535], recency outside [1, GF_WALK_MAX_RECENCY], num_rows * num_walks
 * >= 2^31: GF_ERR_INVALID_ARGUMENT, nothing launched.  num_rows == 0: GF_OK, nothing launched. */
#define GF_WALK_MAX_LENGTH 32
#define GF_WALK_MAX_RECENCY 8
#define GF_WALK_SEED_TAG 0x54454D5057414C4BULL /* "TEMPWALK" */
GF_API int gf_graph_temporal_walks(const gf_graph* g, const int64_t* d_src, const float* d_ts,
                                   size_t num_rows, size_t num_walks, size_t length,
                                   size_t recency, size_t max_history, uint64_t seed,
                                   uint64_t epoch, uint64_t first_row, int64_t* d_nodes,
                                   int64_t* d_eids, float* d_times, int device, void* stream);

/* The position-count ("anonymous") encoding of walks.  d_nodes is int64 [rows, walks, len1], the
 * walks to encode (len1 = L + 1 nodes each); d_ref is int64 [rows, ref_walks, ref_len1], the walks
 * to count in, which may be d_nodes itself; d_out is int32 [rows, walks, len1, ref_len1]; all
 * row-major and contiguous:
 *   d_out[i, w, j, p] = #{w' < ref_walks : d_ref[i, w', p] == d_nodes[i, w, j]}
 *                       when d_nodes[i, w, j] >= 0, else 0.
 * A negative entry (an ended slot of gf_graph_temporal_walks) encodes to zeros and is never
 * counted.  Every element of d_out is written.  One launch on `stream`: a workgroup per row
 * holds d_ref[i] in LDS (ref_walks * ref_len1 <= GF_WALK_MAX_REF_ENTRIES ids, 32 KB) and compares
 * every entry of d_nodes[i] with every entry of it, walks * len1 * ref_walks * ref_len1 compares
 * per row.  No atomics: the same inputs give the same bits.
 * len1 or ref_len1 outside [1, GF_WALK_MAX_LENGTH + 1], ref_walks * ref_len1 >
 * GF_WALK_MAX_REF_ENTRIES, rows >= 2^31, walks * len1 * ref_len1 >= 2^31, a NULL buffer that is
 * needed: GF_ERR_INVALID_ARGUMENT, nothing launched.  rows == 0 or walks == 0: GF_OK, nothing
 * launched. */
#define GF_WALK_MAX_REF_ENTRIES 4096
GF_API int gf_walk_position_counts(const int64_t* d_nodes, const int64_t* d_ref, size_t rows,
                                   size_t walks, size_t len1, size_t ref_walks, size_t ref_len1,
                                   int32_t* d_out, int device, void* stream);

/* ---- measurement support (bench.py) ---------------------------------------- */
/* Accumulated device time of a kernel family since the last reset, measured with
 * HIP events recorded around each launch on the launching stream.
 * which: 0 = sampler search, 1 = sampler emit, 2 = feature gather, 3 = sampler scan,
 * 4 = LRU update (all bookkeeping kernels of one fetch as one interval).
 * gf_profile_enable takes a bit mask of the families to time (0 = off). */
GF_API int gf_profile_enable(int mask);
GF_API int gf_profile_reset(void);
GF_API int gf_profile_get(int which, double* total_ms, uint64_t* launches);
/* Time only every stride-th interval of a family (default 1 = all): an event pair costs
 * host time and a few microseconds of stream time per launch, which a latency-bound
 * workload feels; gf_profile_get then reports the sampled intervals. */
GF_API int gf_profile_set_stride(unsigned stride);
/* Host time the issuing thread spent per stage of the slotted partitioned chain since the last
 * reset: out[0..6] = begin, plan, request exchange, serve, reply exchange, merge, commit
 * (microseconds, summed over the samples), out[7] = samples.  Diagnostics: the chain is ~13
 * stream operations issued by one thread, which bounds its throughput at small batches. */
GF_API int gf_debug_part_host_us(double out[8], int reset);
/* Tiles of the fused partitioned merge whose look-back granule did not arrive within the polling
 * budget and were recounted by the waiting thread instead (current device, since the library
 * was loaded).  0 in normal operation; non-zero when the GPU is heavily oversubscribed (several
 * rank processes sharing one card).  Synchronises nothing but the copy itself. */
GF_API int gf_debug_merge_recounts(uint64_t* out);
/* Roots the plans of the shared partitioned chains did NOT request because the previous layer's
 * block already holds their edges (flags bit 1 of the group entry points), summed since the
 * library was loaded, current device.  Diagnostics / tests. */
GF_API int gf_debug_part_reused_roots(uint64_t* out);
/* d_out[i] = gf_philox4x32_10_first(seed, slot, call) of d_in[i] = {seed, slot, call}, evaluated by
 * a kernel: the Random123 known-answer vectors checked ON THE DEVICE (include/gnnflow_rng.h is
 * shared with the CPU oracle, so parity alone would not catch a device-side miscompile). */
GF_API int gf_debug_philox(const uint64_t* d_in, size_t n, uint32_t* d_out, void* stream);
/* The same for the one-launch LRU list update (lru_list_fused_kernel): granules {launch tag,
 * count} a waiting workgroup did not see within its polling budget and recomputed from the
 * launch's inputs.  0 in normal operation. */
GF_API int gf_debug_lru_recounts(uint64_t* out);
/* All launches of a family seen since the last reset while it was enabled, timed or not. */
GF_API int gf_profile_launches(int which, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* GNNFLOW_HIP_H_ */

// extern "C" entry points of include/gnnflow_hip.h over the transports of comm.hip (gf_comm_*,
// gf_ipc_comm_*, gf_loopback_comm_create); gf_streams_share_queue and gf_device_pci_bus_id.
#include <chrono>

#include "capi_handles.hpp"

extern "C" {

int gf_comm_unique_id(uint8_t* out) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_comm_unique_id: null output");
    gf::RcclComm::unique_id(out);
  });
}
int gf_comm_create(gf_comm** out, const uint8_t* id, int world_size, int rank, int device) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr && id != nullptr, "gf_comm_create: null argument");
    *out = new gf_comm(id, world_size, rank, device);
  });
}
int gf_comm_destroy(gf_comm* c) { return destroy_handle(c); }
int gf_ipc_comm_create(gf_comm** out, int world_size, int rank, int device, size_t mailbox_bytes,
                       const char* shm_name) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_ipc_comm_create: null output");
    *out = new gf_comm(new gf::IpcExchange(world_size, rank, device, mailbox_bytes, shm_name));
  });
}
int gf_ipc_comm_handle(gf_comm* c, uint8_t* out) {
  return guarded([&] {
    GF_REQUIRE(c != nullptr && c->ipc != nullptr && out != nullptr, "not an IPC communicator");
    c->ipc->handle(out);
  });
}
int gf_ipc_comm_open(gf_comm* c, const uint8_t* handles) {
  return guarded([&] {
    GF_REQUIRE(c != nullptr && c->ipc != nullptr, "not an IPC communicator");
    c->ipc->open_peers(handles);
  });
}
int gf_loopback_comm_create(gf_comm** out, int world_size, int device) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_loopback_comm_create: null output");
    auto ranks = gf::LoopbackExchange::create(world_size, device);
    for (int r = 0; r < world_size; ++r) out[r] = new gf_comm(ranks[r].release());
  });
}
int gf_comm_info(gf_comm* c, int32_t* out) {
  return guarded([&] {
    GF_REQUIRE(c != nullptr && out != nullptr, "gf_comm_info: null argument");
    int v[4];
    c->impl.info(v);
    if (v[3] < 0) v[3] = c->ipc ? 1 : 2;
    for (int i = 0; i < 4; ++i) out[i] = v[i];
  });
}
int gf_comm_abort(gf_comm* c) {
  return guarded([&] { GF_REQUIRE(c != nullptr, "null communicator"); c->impl.abort(); });
}
int gf_comm_all_to_all(gf_comm* c, const void* d_send, void* d_recv, size_t bytes_per_peer,
                       void* stream) {
  return guarded([&] {
    GF_REQUIRE(c != nullptr, "null communicator");
    c->impl.all_to_all(d_send, d_recv, bytes_per_peer, as_stream(stream));
  });
}
int gf_comm_all_to_all_v(gf_comm* c, const void* d_send, const size_t* send_bytes,
                         const size_t* send_offsets, void* d_recv, const size_t* recv_bytes,
                         const size_t* recv_offsets, void* stream) {
  return guarded([&] {
    GF_REQUIRE(c != nullptr, "null communicator");
    c->impl.all_to_all_v(d_send, send_bytes, send_offsets, d_recv, recv_bytes, recv_offsets,
                         as_stream(stream));
  });
}
// `iters` equal-split all-to-alls of bytes_per_peer bytes per peer on scratch buffers, one after
// the other on `stream`: device time per exchange from events around the batch, host time per
// exchange of the issuing thread.  Collective: every rank calls it with the same arguments.
int gf_comm_time_all_to_all(gf_comm* c, size_t bytes_per_peer, int iters, void* stream,
                            double* device_us, double* host_us) {
  return guarded([&] {
    GF_REQUIRE(c != nullptr && device_us != nullptr && host_us != nullptr && iters > 0,
               "gf_comm_time_all_to_all: bad argument");
    hipStream_t st = as_stream(stream);
    const size_t bytes = std::max<size_t>(bytes_per_peer, 8) * static_cast<size_t>(c->impl.world());
    gf::DeviceBuffer send, recv;
    send.reserve(bytes);
    recv.reserve(bytes);
    GF_HIP(hipMemsetAsync(send.data(), 0, bytes, st));
    hipEvent_t e0, e1;
    GF_HIP(hipEventCreate(&e0));
    GF_HIP(hipEventCreate(&e1));
    for (int w = 0; w < 3; ++w) c->impl.all_to_all(send.data(), recv.data(), bytes_per_peer, st);
    GF_HIP(hipStreamSynchronize(st));
    GF_HIP(hipEventRecord(e0, st));
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < iters; ++i) c->impl.all_to_all(send.data(), recv.data(), bytes_per_peer, st);
    const auto t1 = std::chrono::steady_clock::now();
    GF_HIP(hipEventRecord(e1, st));
    GF_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    GF_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *device_us = 1e3 * ms / iters;
    *host_us = std::chrono::duration<double, std::micro>(t1 - t0).count() / iters;
  });
}
namespace {
__global__ void probe_spin_kernel(unsigned long long ticks) {   // 100 MHz wall clock
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
__global__ void probe_touch_kernel(unsigned* out) { if (out) *out = 1u; }
}  // namespace
int gf_streams_share_queue(int device, void* a, void* b, unsigned spin_us, int* shared) {
  return guarded([&] {
    GF_REQUIRE(shared != nullptr, "gf_streams_share_queue: null output");
    GF_REQUIRE(spin_us >= 20 && spin_us <= 100000, "gf_streams_share_queue: spin_us out of range");
    gf::DeviceGuard dg(device);
    hipStream_t sa = as_stream(a), sb = as_stream(b);
    hipEvent_t ea = nullptr, eb = nullptr;
    GF_HIP(hipEventCreateWithFlags(&ea, hipEventDisableTiming));
    GF_HIP(hipEventCreateWithFlags(&eb, hipEventDisableTiming));
    GF_HIP(hipStreamSynchronize(sa));
    GF_HIP(hipStreamSynchronize(sb));
    int votes = 0;
    for (int round = 0; round < 3; ++round) {   // (a busy box may delay the small kernel once)
      probe_spin_kernel<<<dim3(1), dim3(64), 0, sa>>>(static_cast<unsigned long long>(spin_us) * 100ull);
      GF_HIP(hipEventRecord(ea, sa));
      probe_touch_kernel<<<dim3(1), dim3(1), 0, sb>>>(nullptr);
      GF_HIP(hipEventRecord(eb, sb));
      // b's kernel done while a's still spins -> the two run side by side
      bool beside = false;
      for (;;) {
        const hipError_t qb = hipEventQuery(eb);
        const hipError_t qa = hipEventQuery(ea);
        if (qb == hipSuccess && qa == hipErrorNotReady) { beside = true; break; }
        if (qa == hipSuccess) break;
        if (qa != hipErrorNotReady) GF_HIP(qa);
        if (qb != hipSuccess && qb != hipErrorNotReady) GF_HIP(qb);
      }
      (void)hipGetLastError();
      GF_HIP(hipStreamSynchronize(sa));
      GF_HIP(hipStreamSynchronize(sb));
      if (beside) ++votes;
    }
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    *shared = votes >= 2 ? 0 : 1;
  });
}
int gf_device_pci_bus_id(int device, char* out, size_t len) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr && len >= 16, "gf_device_pci_bus_id: output too small");
    GF_HIP(hipDeviceGetPCIBusId(out, static_cast<int>(len), device));
  });
}

}  // extern "C"

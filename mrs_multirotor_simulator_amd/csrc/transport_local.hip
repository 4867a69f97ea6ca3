// transport_local.hip — collectives that need no collective library: the in-process loopback group (`world` swarms of ONE
// process, one host thread each: virtual shards on one device — what the tests use on the one-GPU box — or several devices of a
// node without RCCL), a caller-supplied all-gather, and the measurement stand-in (ONE rank of `world` alone on a device).
#include "host_internal.h"
#include "collide_device.inc"  // wall_clock64

// ---- in-process collective: `world` swarms of one process, one host thread each -------------------------------------------------
struct mrs_loopback_group {
  int                      world = 0;
  std::atomic<int>         arrived{0};
  std::atomic<unsigned>    generation{0};
  std::vector<const void*> send;
  std::vector<Event>       ev_ready, ev_copied;  // (one per rank, created by the rank that joins; all freed with the group)
  std::atomic<int>         failed{0};
  // rendezvous mode (mrs_loopback_group_set_rendezvous): no barrier — a rank stages its block, publishes the index of the collective
  // and only waits until every peer has published the same index (it cannot enqueue copies of data a peer has not enqueued yet);
  // staging buffers and events alternate between two sets, so a fast rank never waits for a slow one to have COPIED
  int                                     rendezvous = 0;
  std::unique_ptr<std::atomic<unsigned>[]> seq;           // seq[q] = collectives rank q has published
  std::vector<DevBuf<void>>               stage[2];      // (count bytes)
  std::vector<Event>                      ev_ready2[2], ev_copied2[2];
  void barrier() {  // sense-reversing spin barrier (at most a handful of threads, all inside the same library call)
    const unsigned gen = generation.load(std::memory_order_acquire);
    if (arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == world) {
      arrived.store(0, std::memory_order_relaxed);
      generation.store(gen + 1, std::memory_order_release);
    } else {
      long spins = 0;
      const auto t0 = std::chrono::steady_clock::now();
      while (generation.load(std::memory_order_acquire) == gen) {
        if (++spins > 2000) std::this_thread::yield();
        // a peer that failed (or whose driver thread died) never arrives: give up instead of hanging the process
        if ((spins & 0xFFFF) == 0 && (failed.load() || std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))) {
          failed.store(1);
          return;
        }
      }
    }
  }
};

// ---- kernels of the measurement stand-in ------------------------------------------------------------------------------------------
// one wave that watches the 100 MHz wall clock for `microseconds` (mrs_debug_stream_delay: stands in for a collective's latency)
namespace {
__global__ void k_stream_delay(long long ticks) {
  const long long t0 = wall_clock64();
  unsigned        k  = 0;
  while (wall_clock64() - t0 < ticks && k < 400000000u) k++;
}

// The collective of the measurement stand-in as ONE kernel that lasts `ticks` of the 100 MHz clock (one wave watches it — a real
// collective keeps a few waves busy, not the chip): the rank's own block of `bytes` bytes is copied to the places
// of ranks rank-1, rank, rank+1 of `recv`; when the blocks are 48-byte records (`kind` 1), absent ranks read as NaN records and the
// two images are moved one slab width to either side.  Likewise the 64-byte entries of a halo exchange (kind 2; absent ranks: an
// empty header) and the search box at the tail of a slot map (kind 3, `aux` = its first 16-byte vector; absent ranks: NaN bounds).
__global__ void k_standin_gather(const uint4* send, uint4* recv, long long vec_per_rank, int rank, int world, int kind, long long aux, double width,
                                 long long ticks) {
  const long long t_start = wall_clock64();
  const long long total = vec_per_rank * (long long)world;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (long long)gridDim.x * blockDim.x) {
    const int       q = (int)(v / vec_per_rank);
    const long long j = v - (long long)q * vec_per_rank;
    const int       d = q - rank;
    if (d < -1 || d > 1) {
      if (kind == 1 || (kind == 3 && j >= aux && j < aux + 3)) recv[v] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
      if (kind == 2 && j < 4) recv[v] = make_uint4(0u, 0u, 0u, 0u);
      continue;
    }
    uint4 x = send[j];
    // a 48-byte record = three 16-byte vectors, a halo entry four, the first holds x and y; a box = xmin ymin | zmin xmax | ymax zmax
    const bool lo = d != 0 && ((kind == 1 && j % 3 == 0) || (kind == 2 && j % 4 == 0) || (kind == 3 && j == aux));
    const bool hi = d != 0 && kind == 3 && j == aux + 1;
    if (lo) {
      double px = __builtin_bit_cast(double, make_uint2(x.x, x.y));
      px += (double)d * width;
      const uint2 b = __builtin_bit_cast(uint2, px);
      x.x = b.x; x.y = b.y;
    }
    if (hi) {
      double px = __builtin_bit_cast(double, make_uint2(x.z, x.w));
      px += (double)d * width;
      const uint2 b = __builtin_bit_cast(uint2, px);
      x.z = b.x; x.w = b.y;
    }
    recv[v] = x;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // ONE wave keeps the kernel alive until the collective's latency is over
    unsigned k = 0;
    while (wall_clock64() - t_start < ticks && k < 400000000u) k++;
  }
}
}  // namespace
static hipError_t launch_standin_gather(const void* send, void* recv, size_t bytes, int rank, int world, double latency_us, int kind, long long aux, double width,
                                        hipStream_t st) {
  if (bytes % 16 != 0) return hipErrorInvalidValue;
  const long long vec = (long long)(bytes / 16);
  long long       blocks = (vec * world + 255) / 256;
  if (blocks > 512) blocks = 512;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_standin_gather, dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)send, (uint4*)recv, vec, rank, world, kind, aux, width,
                     (long long)(latency_us * 100.0));
  return hipGetLastError();
}
static hipError_t launch_stream_delay(hipStream_t st, double microseconds) {
  hipLaunchKernelGGL(k_stream_delay, dim3(1), dim3(64), 0, st, (long long)(microseconds * 100.0));
  return hipGetLastError();
}

namespace mrs_host {
// all-gather among the swarms of a loopback group: every rank copies every rank's send buffer into its own receive buffer, device
// to device on its own stream; events order the copies behind the producers and the producers' next writes behind the copies
static int loopback_allgather_rendezvous(mrs_loopback_group* g, int rank, const void* send, void* recv, size_t bytes, hipStream_t st) {
  const size_t   r = (size_t)rank;
  const unsigned k = g->seq[r].load(std::memory_order_relaxed);  // index of this collective (only this thread writes seq[rank])
  const int      par = (int)(k & 1u);
  hipError_t     e = hipSuccess;
  // the staging buffer of this parity was last read by the peers in collective k - 2: their "copied" events were recorded before they
  // published k - 1, which this rank waited for in collective k - 1
  for (int q = 0; q < g->world && e == hipSuccess && k >= 2u; q++) e = hipStreamWaitEvent(st, g->ev_copied2[par][(size_t)q], 0);
  if (e == hipSuccess && bytes > g->stage[par][r].capacity()) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = g->stage[par][r].reserve(bytes);
  if (e == hipSuccess && bytes) e = hipMemcpyAsync(g->stage[par][r], send, bytes, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipEventRecord(g->ev_ready2[par][r], st);
  if (e != hipSuccess) g->failed.store(1);
  g->seq[r].store(k + 1u, std::memory_order_release);
  const auto t0 = std::chrono::steady_clock::now();
  for (int q = 0; q < g->world; q++) {
    unsigned long spins = 0;
    while (g->seq[(size_t)q].load(std::memory_order_acquire) < k + 1u) {
      if (++spins > 2000) std::this_thread::yield();
      if ((spins & 0xFFFF) == 0 && (g->failed.load() || std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))) {
        g->failed.store(1);
        return fail(MRS_ERR_HIP, "loopback all-gather (rendezvous): a peer never arrived at collective " + std::to_string(k));
      }
    }
  }
  for (int q = 0; q < g->world && e == hipSuccess; q++) {
    e = hipStreamWaitEvent(st, g->ev_ready2[par][(size_t)q], 0);
    if (e == hipSuccess && bytes) e = hipMemcpyAsync((char*)recv + (size_t)q * bytes, g->stage[par][(size_t)q], bytes, hipMemcpyDeviceToDevice, st);
  }
  if (e == hipSuccess) e = hipEventRecord(g->ev_copied2[par][r], st);
  if (e != hipSuccess || g->failed.load()) {
    g->failed.store(1);
    return fail(MRS_ERR_HIP, std::string("loopback all-gather (rendezvous): ") + hipGetErrorString(e));
  }
  return MRS_OK;
}

int loopback_allgather(mrs_loopback_group* g, int rank, const void* send, void* recv, size_t bytes, hipStream_t st) {
  if (g->rendezvous) return loopback_allgather_rendezvous(g, rank, send, recv, bytes, st);
  const char* what = "record";
  hipError_t  e = hipGetLastError();  // (an error left behind by an earlier asynchronous launch belongs to that launch, not to this collective)
  if (e != hipSuccess) what = "an earlier launch on this thread";
  if (e == hipSuccess) e = hipEventRecord(g->ev_ready[(size_t)rank], st);
  g->send[(size_t)rank] = send;
  if (e != hipSuccess) g->failed.store(1);
  g->barrier();  // every rank has published its buffer and recorded "my send data is complete"
  for (int q = 0; q < g->world && e == hipSuccess; q++) {
    what = "wait for a peer's data";
    e = hipStreamWaitEvent(st, g->ev_ready[(size_t)q], 0);
    if (e == hipSuccess && bytes) {
      what = "copy";
      e = hipMemcpyAsync((char*)recv + (size_t)q * bytes, g->send[(size_t)q], bytes, hipMemcpyDeviceToDevice, st);
    }
  }
  if (e == hipSuccess) e = hipEventRecord(g->ev_copied[(size_t)rank], st);
  if (e != hipSuccess) g->failed.store(1);
  g->barrier();  // every rank has enqueued its copies
  for (int q = 0; q < g->world && e == hipSuccess; q++) e = hipStreamWaitEvent(st, g->ev_copied[(size_t)q], 0);  // nobody overwrites a buffer a peer still reads
  if (e != hipSuccess) return fail(MRS_ERR_HIP, std::string("loopback all-gather (") + what + ", " + std::to_string(bytes) + " bytes per rank): " + hipGetErrorString(e));
  if (g->failed.load()) return fail(MRS_ERR_HIP, "loopback all-gather: a peer of the group has failed");
  return MRS_OK;
}

// The collective of the measurement stand-in: ONE kernel that takes `standin_delay_us` of stream time (a collective's latency) and
// leaves the rank's own block in its own place and in the places of its two neighbours in the slab order — records (recognised by
// their size) moved one slab width to either side, slot maps and export blocks as they are: the neighbours are periodic images of
// this rank, so the export sets mirror each other as they do between real neighbours (positions of foreign partners are the
// images' only at a search; between searches they read as far away — fine for a time measurement, meaningless as a simulation).
int standin_allgather(mrs_swarm* s, const void* send, void* recv, size_t bytes) {
  // what travels is told by where it comes from: position records, halo entries of a search, slot maps (with the search box at the tail)
  const int       kind = send == (const void*)s->comm_send ? 1 : (s->cwork && send == mrs_collide_halo_send(s->cwork) ? 2 : (send == (const void*)s->x_map_send ? 3 : 0));
  const long long aux  = kind == 3 ? (long long)(map_boxw(s) / 4) : 0;
  if (bytes % 16 != 0) {  // (a block that is no whole number of 16-byte units — none of the library's own collectives any more) plain copies
    HIPCHK(hipMemsetAsync(recv, 0, bytes * (size_t)s->comm_world, s->cstream));
    for (int d = -1; d <= 1; d++)
      if (s->comm_rank + d >= 0 && s->comm_rank + d < s->comm_world)
        HIPCHK(hipMemcpyAsync((char*)recv + (size_t)(s->comm_rank + d) * bytes, send, bytes, hipMemcpyDeviceToDevice, s->cstream));
    return MRS_OK;
  }
  // MRS_STANDIN_GBPS (default 0: off): the collective also takes the time its bytes need on the links — (world - 1) blocks received
  // at that many GB/s — on top of the fixed latency; without it the 42 MB of a search tick's record gather cost as much as 54 KB
  const double gbps    = s->standin_gbps;  // (read when the stand-in communicator is bound)
  const double wire_us = gbps > 0.0 ? (double)bytes * (double)(s->comm_world - 1) / (gbps * 1e3) : 0.0;
  HIPCHK(launch_standin_gather(send, recv, bytes, s->comm_rank, s->comm_world, s->standin_delay_us + wire_us, kind, aux, s->standin_width, s->cstream));
  return MRS_OK;
}
}  // namespace mrs_host

extern "C" {

int mrs_swarm_comm_init_custom(mrs_swarm_t* s, int32_t world, int32_t rank, int64_t n_total, mrs_allgather_fn fn, void* user) {
  MRS_ENTER(s);
  if (!s || !fn) return fail(MRS_ERR_ARG, "null argument");
  int rc = comm_setup(s, world, rank, n_total);
  if (rc) return rc;
  HIPCHK(hipSetDevice(s->device));
  s->comm_fn   = fn;
  s->comm_user = user;
  return comm_buffers(s, world, rank, n_total);
}

int mrs_swarm_comm_init_standin(mrs_swarm_t* s, int32_t world, int32_t rank, int64_t n_total, double collective_latency_us, double slab_width) {
  MRS_ENTER(s);
  if (!s || !(collective_latency_us >= 0) || !(slab_width > 0)) return fail(MRS_ERR_ARG, "bad stand-in arguments");
  int rc = comm_setup(s, world, rank, n_total);
  if (rc) return rc;
  HIPCHK(hipSetDevice(s->device));
  s->comm_standin     = true;
  s->standin_delay_us = collective_latency_us;
  s->standin_width    = slab_width;
  s->standin_gbps     = getenv("MRS_STANDIN_GBPS") ? atof(getenv("MRS_STANDIN_GBPS")) : 0.0;
  return comm_buffers(s, world, rank, n_total);
}

int mrs_loopback_group_create(int32_t world, mrs_loopback_group_t** out) {
  if (!out || world < 1 || world > 64) return fail(MRS_ERR_ARG, "bad loopback group size");
  mrs_loopback_group* g = new mrs_loopback_group();
  g->world = world;
  g->send.assign((size_t)world, nullptr);
  g->ev_ready.resize((size_t)world);
  g->ev_copied.resize((size_t)world);
  g->seq.reset(new std::atomic<unsigned>[(size_t)world]);
  for (int q = 0; q < world; q++) g->seq[(size_t)q].store(0u);
  for (int par = 0; par < 2; par++) {
    g->stage[par].resize((size_t)world);
    g->ev_ready2[par].resize((size_t)world);
    g->ev_copied2[par].resize((size_t)world);
  }
  *out = g;
  return MRS_OK;
}

int mrs_loopback_group_set_rendezvous(mrs_loopback_group_t* g, int32_t on) {
  if (!g) return fail(MRS_ERR_ARG, "null group");
  for (int q = 0; q < g->world; q++)
    if (g->seq[(size_t)q].load() != 0u) return fail(MRS_ERR_ARG, "the mode of a loopback group is chosen before its first collective");
  g->rendezvous = on ? 1 : 0;
  return MRS_OK;
}

int mrs_loopback_group_destroy(mrs_loopback_group_t* g) {
  delete g;  // (events and staging blocks of every rank: hipEventDestroy and hipFree find the device of what they are given)
  return MRS_OK;
}

int mrs_swarm_comm_init_loopback(mrs_swarm_t* s, mrs_loopback_group_t* g, int32_t rank, int64_t n_total) {
  MRS_ENTER(s);
  if (!s || !g) return fail(MRS_ERR_ARG, "null argument");
  int rc = comm_setup(s, g->world, rank, n_total);
  if (rc) return rc;
  if (g->ev_ready[(size_t)rank]) return fail(MRS_ERR_ARG, "this rank of the loopback group is taken");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(g->ev_ready[(size_t)rank].create(hipEventDisableTiming));
  HIPCHK(g->ev_copied[(size_t)rank].create(hipEventDisableTiming));
  for (int par = 0; par < 2; par++) {
    HIPCHK(g->ev_ready2[par][(size_t)rank].create(hipEventDisableTiming));
    HIPCHK(g->ev_copied2[par][(size_t)rank].create(hipEventDisableTiming));
    HIPCHK(hipEventRecord(g->ev_copied2[par][(size_t)rank], s->stream));  // (an event that was never recorded must not be waited for)
  }
  s->comm_group           = g;
  return comm_buffers(s, g->world, rank, n_total);
}

int mrs_debug_stream_delay(void* stream, double microseconds) {
  if (!(microseconds >= 0) || microseconds > 1e6) return fail(MRS_ERR_ARG, "bad delay");
  HIPCHK(launch_stream_delay((hipStream_t)stream, microseconds));
  return MRS_OK;
}

}  // extern "C"

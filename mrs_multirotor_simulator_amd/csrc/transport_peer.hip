// transport_peer.hip — the peer-window exchange: the collectives of the sharded tick as direct writes into the peers' device memory
// over xGMI (k_peer_allgather below), no collective library and no host in the tick.  DESIGN §5.
#include "host_internal.h"
#include "collide_device.inc"  // wall_clock64, MRS_WAIT_TICKS

// ---- peer-window all-gather: the exchange of a sharded swarm WITHOUT a collective library in the tick ----
// Every rank owns a WINDOW in its own device memory (fine-grained, mapped into every peer: hipIpcOpenMemHandle across processes,
// plain pointers inside one): [world flag lines of 64 B | pad to 4096 | 2 parities x world slots of slot_bytes].  One kernel per
// rank and collective, no host in between.  A group of `bpp` blocks serves ONE peer q (the group of the own rank copies the own
// block into the receive buffer and is done):
//   1. push   — the group's shares of the rank's block go straight into slot [seq & 1][rank] of q's window (system-scope stores:
//               one hop over xGMI);
//   2. signal — every block fences its stores (system scope); the last block of the group (a ticket when bpp > 1) writes seq into
//               flag[rank] of q's window;
//   3. wait   — one lane polls flag[q] of the OWN window until q has signalled seq (bounded: 10 s, then the error word is set and
//               the kernel ends — the call reports it), acquire;
//   4. pull   — q's slot is copied from the own window into the receive buffer (system-scope loads: another device wrote the lines).
// On exit the receive buffer holds what an all-gather would have put there, so the caller's kernels do not know the difference;
// no block waits for another block of its own launch except through the ticket, which needs no residency (it is taken after the work).
// Two parities suffice: a peer can only be one collective ahead (it cannot finish seq+1 without this rank's flag for seq+1, which
// is written by this rank's kernel seq+1, i.e. after its kernel seq has ended), so what it writes while this rank still pulls seq
// goes to the other parity.
// Cost: one one-way latency + the copy, where a ring all-gather pays 2 (world - 1) hops behind a kernel launch of its own.
namespace {
typedef __attribute__((address_space(1))) unsigned long long peer_u64;
typedef __attribute__((address_space(1))) unsigned           peer_u32;
template <class U> struct PeerWord;
template <> struct PeerWord<unsigned long long> { typedef peer_u64 G; };
template <> struct PeerWord<unsigned>           { typedef peer_u32 G; };
#define MRS_PEER_THREADS 512

template <class U>
__global__ __launch_bounds__(MRS_PEER_THREADS) void k_peer_allgather(MrsPeerWindows pw, const U* __restrict__ send, U* __restrict__ recv, long long units,
                                                                     int rank, int bpp, unsigned seq, unsigned long long slot_bytes,
                                                                     unsigned* tickets, unsigned ticket_target, unsigned* err_host, int world) {
  typedef typename PeerWord<U>::G G;
  const int       q = (int)blockIdx.x / bpp, j = (int)blockIdx.x - q * bpp;
  const long long share = (units + bpp - 1) / bpp, lo = (long long)j * share, hi = lo + share < units ? lo + share : units;
  if (q == rank) {
    for (long long u = lo + threadIdx.x; u < hi; u += MRS_PEER_THREADS) recv[(long long)rank * units + u] = send[u];
    return;
  }
  // 1. push
  G* there = (G*)((char*)pw.win[q] + 4096ull + ((unsigned long long)(seq & 1u) * (unsigned)world + (unsigned)rank) * slot_bytes);
  for (long long u = lo + threadIdx.x; u < hi; u += MRS_PEER_THREADS) __hip_atomic_store(there + u, send[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // 2. signal
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    bool last = true;
    if (bpp > 1) last = __hip_atomic_fetch_add((peer_u32*)(tickets + q), 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u == ticket_target;
    if (last) __hip_atomic_store((peer_u32*)((char*)pw.win[q] + 64 * rank), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    // 3. wait
    const peer_u32* flag = (const peer_u32*)((const char*)pw.win[rank] + 64 * q);
    const long long t0   = wall_clock64();
    // (an exchange of this rank has given up before: the results are void already, the call will say so — what is still queued
    //  must not wait its 10 s again, launch after launch)
    //  (the mark is kept in device memory too — tickets[MRS_MAX_PEERS] —: the pinned host word is a PCIe round trip away)
    const bool dead = __hip_atomic_load((peer_u32*)(tickets + MRS_MAX_PEERS), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    while (!dead && (int)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - seq) < 0) {
      if (wall_clock64() - t0 > MRS_WAIT_TICKS) {
        // (pinned host words, plain stores — no PCIe atomic: [0] = set, [1] = the collective, [2] = the peer, [3] = what its flag said)
        __hip_atomic_store((peer_u32*)err_host + 1, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store((peer_u32*)err_host + 2, (unsigned)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store((peer_u32*)err_host + 3, __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store((peer_u32*)err_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store((peer_u32*)(tickets + MRS_MAX_PEERS), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  // 4. pull
  const G* here = (const G*)((const char*)pw.win[rank] + 4096ull + ((unsigned long long)(seq & 1u) * (unsigned)world + (unsigned)q) * slot_bytes);
  for (long long u = lo + threadIdx.x; u < hi; u += MRS_PEER_THREADS)
    recv[(long long)q * units + u] = __hip_atomic_load(here + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // namespace
// `ticket_total`: tickets every peer's word has seen from all earlier launches of this rank (the caller adds the returned `bpp`)
static hipError_t launch_peer_allgather(const MrsPeerWindows* pw, const void* send, void* recv, size_t bytes, int rank, int world, unsigned seq,
                                        size_t slot_bytes, unsigned* tickets, unsigned ticket_total, unsigned* err_host, unsigned* bpp_out, hipStream_t st) {
  if (bytes == 0 || bytes % 4 != 0 || bytes > slot_bytes || world < 1 || world > MRS_MAX_PEERS) return hipErrorInvalidValue;
  const bool      wide  = bytes % 8 == 0;
  const long long units = (long long)(bytes / (wide ? 8 : 4));
  long long       bpp   = ((long long)bytes + 131071) / 131072;  // one block per peer up to 128 KiB (the per-tick export blocks), then one per 128 KiB
  if (bpp > 16) bpp = 16;
  *bpp_out = bpp > 1 ? (unsigned)bpp : 0u;  // (a group of one block takes no ticket)
  const dim3 grid((unsigned)(bpp * world)), block(MRS_PEER_THREADS);
  if (wide)
    hipLaunchKernelGGL(k_peer_allgather<unsigned long long>, grid, block, 0, st, *pw, (const unsigned long long*)send, (unsigned long long*)recv, units, rank,
                       (int)bpp, seq, (unsigned long long)slot_bytes, tickets, ticket_total + (unsigned)bpp, err_host, world);
  else
    hipLaunchKernelGGL(k_peer_allgather<unsigned>, grid, block, 0, st, *pw, (const unsigned*)send, (unsigned*)recv, units, rank, (int)bpp, seq,
                       (unsigned long long)slot_bytes, tickets, ticket_total + (unsigned)bpp, err_host, world);
  return hipGetLastError();
}

namespace mrs_host {
// the peer-window exchange: every rank issues the same collectives in the same order, so the sequence number is the same everywhere
int peer_allgather(mrs_swarm* s, const void* send, void* recv, size_t bytes) {
  if (bytes > s->peer_slot_bytes) return fail(MRS_ERR_ARG, "peer-window exchange: a block of " + std::to_string(bytes) + " bytes does not fit the window's slots (" + std::to_string(s->peer_slot_bytes) + ")");
  unsigned taken = 0;
  HIPCHK(launch_peer_allgather(&s->peer_windows, send, recv, bytes, s->comm_rank, s->comm_world, ++s->peer_seq, s->peer_slot_bytes, s->peer_ticket, s->peer_tickets,
                               s->peer_err, &taken, s->cstream));
  s->peer_tickets += taken;
  return MRS_OK;
}

int peer_failed(mrs_swarm* s) {
  volatile unsigned* e = s->peer_err;
  return fail(MRS_ERR_HIP, "peer-window exchange: rank " + std::to_string(s->comm_rank) + " waited in vain for the block of rank " + std::to_string(e[2]) +
                               " in collective " + std::to_string(e[1]) + " (that rank's flag says " + std::to_string(e[3]) + "; this rank has issued " +
                               std::to_string(s->peer_seq) + " collectives, " + std::to_string(s->x_ticks) + " ticks, " + std::to_string(s->x_searches) +
                               " searches) — the results of this call are not valid and the windows are dead: use fresh processes");
}

void peer_release(mrs_swarm* s) {
  for (void* p : s->peer_opened) (void)hipIpcCloseMemHandle(p);
  s->peer_opened.clear();
  s->peer_window.reset();
  s->peer_ticket.reset();
  s->peer_err.reset();
  s->peer_world  = 0;
  s->comm_peer   = false;
}
}  // namespace mrs_host

extern "C" {

int mrs_swarm_peer_window_create(mrs_swarm_t* s, int32_t world, int32_t rank, int64_t n_total, void** window, uint8_t* ipc_handle64) {
  MRS_ENTER(s);
  if (!s || world > MRS_MAX_PEERS) return fail(MRS_ERR_ARG, "bad peer-window arguments (at most 64 ranks)");
  int rc = comm_setup(s, world, rank, n_total);
  if (rc) return rc;
  if (s->peer_window) return fail(MRS_ERR_ARG, "this swarm already has a peer window");
  HIPCHK(hipSetDevice(s->device));
  // the largest block any collective of the sharded tick sends: the full gather of a search (one record per UAV of the largest shard)
  const int64_t n_max = (n_total + world - 1) / world > 0 ? (n_total + world - 1) / world : 1;
  size_t slot = sizeof(PosRecord) * (size_t)n_max;
  if (slot < sizeof(uint32_t) * (size_t)(n_max + 20)) slot = sizeof(uint32_t) * (size_t)(n_max + 20);  // (the slot maps: n_max + 2 words padded to 16-byte units + the search box, map_stride)
  // (an export block is header + capacity records of 32 B, the capacity up to 1.5 x the largest export set + 127: export_search)
  if (slot < sizeof(Pos4) * ((size_t)n_max + (size_t)n_max / 2 + 129)) slot = sizeof(Pos4) * ((size_t)n_max + (size_t)n_max / 2 + 129);
  slot = (slot + 255) / 256 * 256;
  s->peer_slot_bytes   = slot;
  s->peer_window_bytes = 4096 + 2 * (size_t)world * slot;
  // Written by other devices WHILE kernels of this one poll and read it: uncached device memory ("extended-scope fine-grained" — on
  // this GPU family plain fine-grained memory is only guaranteed coherent across devices at kernel boundaries, and the flags are
  // polled inside a kernel; collective libraries allocate their flag and staging memory the same way).  MRS_PEER_WINDOW_MEMORY =
  // finegrained | coarse for runtimes that cannot export an uncached allocation (every access of the exchange kernel is
  // system-scope either way).
  struct Release {  // any failure below gives the window, the ticket words and the pinned error word back
    mrs_swarm* p;
    ~Release() {
      if (p) peer_release(p);
    }
  } release{s};
  const char* kind = getenv("MRS_PEER_WINDOW_MEMORY");
  static_assert(hipDeviceMallocDefault == 0, "DevBuf::alloc: kind 0 is plain hipMalloc");
  HIPCHK(s->peer_window.alloc(s->peer_window_bytes, kind && strcmp(kind, "coarse") == 0        ? hipDeviceMallocDefault
                                                    : kind && strcmp(kind, "finegrained") == 0 ? hipDeviceMallocFinegrained
                                                                                               : hipDeviceMallocUncached));
  HIPCHK(s->peer_ticket.alloc(MRS_MAX_PEERS + 1));  // (+ the give-up mark the exchange kernels read)
  HIPCHK(s->peer_err.alloc(16, hipHostMallocMapped));
  *s->peer_err = 0u;
  HIPCHK(hipMemsetAsync(s->peer_window, 0, 4096, s->stream));  // flags: no collective has happened
  HIPCHK(hipMemsetAsync(s->peer_ticket, 0, sizeof(unsigned) * (MRS_MAX_PEERS + 1), s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));  // ... before any peer can learn the address
  if (ipc_handle64) {
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the C ABI carries IPC handles as 64 bytes");
    hipIpcMemHandle_t h;
    const hipError_t  e = hipIpcGetMemHandle(&h, s->peer_window);
    if (e != hipSuccess) return fail(MRS_ERR_HIP, std::string("peer window: hipIpcGetMemHandle: ") + hipGetErrorString(e));
    memcpy(ipc_handle64, &h, 64);
  }
  release.p = nullptr;
  if (window) *window = s->peer_window;
  s->peer_world   = world;
  s->peer_rank    = rank;
  s->peer_n_total = n_total;
  return MRS_OK;
}

int mrs_swarm_comm_init_peer(mrs_swarm_t* s, void* const* windows, const uint8_t* ipc_handles) {
  MRS_ENTER(s);
  if (!s || s->peer_world == 0) return fail(MRS_ERR_ARG, "mrs_swarm_peer_window_create has not been called");
  if (!windows && !ipc_handles) return fail(MRS_ERR_ARG, "the peers' windows are needed as pointers or as IPC handles");
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "communicator already initialised");
  HIPCHK(hipSetDevice(s->device));
  for (int q = 0; q < s->peer_world; q++) {
    void* p = nullptr;
    if (q == s->peer_rank) {
      p = s->peer_window;
    } else if (windows && windows[q]) {
      p = windows[q];
    } else if (ipc_handles) {
      hipIpcMemHandle_t h;
      memcpy(&h, ipc_handles + 64 * (size_t)q, 64);
      const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) return fail(MRS_ERR_HIP, "peer window of rank " + std::to_string(q) + ": hipIpcOpenMemHandle: " + hipGetErrorString(e));
      s->peer_opened.push_back(p);
    } else {
      return fail(MRS_ERR_ARG, "no window given for rank " + std::to_string(q));
    }
    s->peer_windows.win[q] = p;
  }
  s->comm_peer = true;
  s->peer_seq = s->peer_tickets = 0u;
  const int rc = comm_buffers(s, s->peer_world, s->peer_rank, s->peer_n_total);
  if (rc) s->comm_peer = false;
  return rc;
}

}  // extern "C"

// collide_export.hip — the export-set exchange of sharded swarms (the searches it follows: collide.hip).
// ================================================================================================================================
// Export-set exchange (multi-GPU): between two searches a rank only needs the positions of the FOREIGN UAVs its neighbour lists
// name, and only has to publish the own UAVs some other rank lists.  Those two sets mirror each other — "j within the list radius
// of i" is decided by the same squared distance on both sides, from the same gathered records — so a rank finds its export set in
// its own lists: own UAV i is exported iff its list holds a foreign UAV.  A search tick (full gather, mrs_collide_run_lists_gathered)
// is followed by
//   k_export_mark      : export slot e_i for every own UAV with a foreign neighbour (any injective numbering will do)
//   all-gather         : the slot maps of all ranks (4 B per UAV), headed by each rank's count
//   k_export_translate : list entries (global record slots) -> local UAV index | FOREIGN + slot in the padded export collective;
//                        airframe constants and search-time positions of the foreign partners are copied next to those slots
// and every tick until the next search all-gathers 32 B per EXPORTED UAV instead of 48 B per UAV.
// ================================================================================================================================
#include <string.h>

#include "collide_work.h"

namespace {

__global__ void k_fill_positions(SwarmDev sw, Pos4* pos_now) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sw.n) return;
  const size_t np = (size_t)sw.npad;
  const Pos4   pp = {sw.S[(size_t)(F_X + 0) * np + i], sw.S[(size_t)(F_X + 1) * np + i], sw.S[(size_t)(F_X + 2) * np + i],
                     (double)(sw.F[i] >> FLAG_TYPE_SHIFT)};
  pos_now[i]      = pp;
}

// one launch: control words (the error word stays: it is reported at the end of the call), slot map (padding UAVs: no slot), block
// classes, and the export allocation — send block, gathered blocks, partner constants — zeroed (headers!)
__global__ void k_search_reset(uint32_t* fctl, uint32_t* map, long long n_map, uint32_t* blk_class, int n_blocks, uint4* xalloc, long long n_xvec) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_map) map[i] = MRS_NO_SLOT;
  if (i < n_blocks) blk_class[i] = 0u;
  if (i < CTL_WORDS && i != CTL_ERROR && i != CTL_BADSLOT) fctl[i] = 0u;  // (sticky: the host reads both once per call, a call may hold several searches)
  for (long long v = i; v < n_xvec; v += (long long)gridDim.x * blockDim.x) xalloc[v] = make_uint4(0u, 0u, 0u, 0u);
}

// map: [0] export count of this rank, [1] lanes over the list capacity so far, [2 + i] slot of own UAV i
// ... and the position records of the UAVs as the search found them (what the first fused launch after the search reads)
// ... and the displacement bound on the state the search found (pred_hdt >= 0): the lists are new, every UAV sits on its reference
// position — if nobody can leave its skin within MRS_PRED_HORIZON steps, no stall index <= MRS_PRED_HORIZON can exist and the ticks
// right after the search need no serial phase (CTL_PRED, sent to every rank with the head of the slot map)
__global__ void k_export_mark(SwarmDev sw, Pos4* pos_now, long long n_max, int rank, const uint32_t* nbr, const uint32_t* nbr_cnt, uint32_t* exp_slot,
                              uint32_t* map, uint32_t* fctl, uint32_t* blk_class, double pred_hdt, double pred_lim, double rebounce) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = sw.n;
  if (i >= n) return;
  const size_t   np = (size_t)sw.npad;
  const uint32_t fl = sw.F[i];
  double         y[18];
#pragma unroll
  for (int c = 0; c < 18; c++) y[c] = (pred_hdt >= 0.0 || c < 3) ? sw.S[(size_t)(c < 6 ? F_X + c : (c < 15 ? F_R + (c - 6) : F_W + (c - 15))) * np + i] : 0.0;
  {
    const Pos4 pp = {y[0], y[1], y[2], (double)(fl >> FLAG_TYPE_SHIFT)};
    pos_now[i]    = pp;
  }
  const uint32_t cnt = nbr_cnt[i];
  if (pred_hdt >= 0.0) {
    const TypeParams& P = sw.T[fl >> FLAG_TYPE_SHIFT];
    double            thrust = 0.0;  // allocation * rpm^2 with the motor speeds as they are (multirotor_model.hpp:332-335)
    for (int m = 0; m < P.n_motors; m++) {
      const double r = sw.S[(size_t)(F_RPM + m) * np + i];
      thrust += P.alloc[3 * MRS_MAXM + m] * (r * r);
    }
    const bool   takeoff = (fl & FLAG_TAKEOFF) != 0u;
    const double init_z  = takeoff ? sw.S[(size_t)F_INITZ * np + i] : 0.0;
    const bool   usable  = mrs_pos_usable(y[0], y[1], y[2]);
    if (usable && mrs_may_leave(y, 0.0, thrust, cnt, rebounce, pred_hdt, pred_lim, P.pred_a0, P.pred_thr, P.pred_drag, P.ground_enabled, P.ground_z, takeoff, init_z))
      fctl[CTL_PRED] = 1u;  // (same value from every lane that finds one)
  }
  bool           exported = false;
  for (uint32_t k = 0; k < cnt; k++) {
    const uint32_t g = nbr[(size_t)k * (size_t)n + (size_t)i];
    if ((long long)g / n_max != (long long)rank) exported = true;
  }
  uint32_t e = MRS_NO_SLOT;
  if (exported) e = atomicAdd(&fctl[CTL_EXPORTS], 1u);
  exp_slot[i] = e;
  map[2 + i]  = e;
  if (exported) atomicOr(&blk_class[i >> 6], MRS_BLK_BOUNDARY);  // the block is stepped by the boundary launch of a split tick
}

// Behind the marking launch (its block classes are complete): the boundary blocks in a list (any order) and their number; the interior
// blocks that list a UAV of a boundary block (MRS_BLK_LAYER1: they wait for that block's epoch word in a split tick) and their number
// (CTL_NL1: the residency bound of the split form); the head of the rank's slot map — export count (final), bit 31: some own UAV may
// leave its skin within the horizon; lanes over the list capacity.  One thread per own UAV; list entries are still global record slots.
__global__ void k_class_list(int n, long long n_max, int rank, const uint32_t* nbr, const uint32_t* nbr_cnt, uint32_t* blk_class, uint32_t* blk_list,
                             uint32_t* fctl, uint32_t* map, const uint32_t* ctl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    map[0] = fctl[CTL_EXPORTS] | (fctl[CTL_PRED] ? 0x80000000u : 0u);
    map[1] = ctl[6];  // lanes over the list capacity (cumulative, collide.hip k_query)
  }
  if (i >= n) return;
  const uint32_t mine = blk_class[i >> 6];
  if ((i & 63) == 0 && (mine & MRS_BLK_BOUNDARY)) blk_list[atomicAdd(&fctl[CTL_NBND], 1u)] = (uint32_t)(i >> 6);
  if (mine & MRS_BLK_BOUNDARY) return;
  const uint32_t cnt = nbr_cnt[i];
  bool           l1  = false;
  for (uint32_t k = 0; k < cnt; k++) {
    const long long g = (long long)nbr[(size_t)k * (size_t)n + (size_t)i], q = g / n_max;
    if (q == (long long)rank && (blk_class[(g - q * n_max) >> 6] & MRS_BLK_BOUNDARY)) l1 = true;
  }
  // (the layer-1 blocks are listed from the back of the block list — the boundary blocks fill it from the front, a block is never both)
  if (l1 && !(atomicOr(&blk_class[i >> 6], MRS_BLK_LAYER1) & MRS_BLK_LAYER1)) blk_list[(uint32_t)((n + 63) / 64) - 1u - atomicAdd(&fctl[CTL_NL1], 1u)] = (uint32_t)(i >> 6);
}

// start of a run of split ticks behind launch `tau`: every block counts as finished by that launch, nobody has arrived yet
__global__ void k_handoff_init(uint32_t* fctl, uint32_t* epoch, int n_blocks, uint32_t tau) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n_blocks) epoch[b] = tau;
  if (b == 0) fctl[CTL_I_STARTED] = tau;
}

__global__ void k_export_header(uint32_t* map, const uint32_t* fctl, const uint32_t* ctl) {  // (a rank without UAVs)
  map[0] = fctl[CTL_EXPORTS];
  map[1] = ctl[6];
}

__global__ void k_export_translate(int n, long long n_max, int rank, long long map_stride, int block, uint32_t* nbr, const uint32_t* nbr_cnt,
                                   const uint32_t* maps, const PosRecord* rec_all, Pos4* x_recv, PartnerConst* x_const, uint32_t* fctl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t cnt = nbr_cnt[i];
  for (uint32_t k = 0; k < cnt; k++) {
    const size_t    at = (size_t)k * (size_t)n + (size_t)i;
    const uint32_t  g  = nbr[at];
    const long long q  = (long long)g / n_max, j = (long long)g - q * n_max;
    if (q == (long long)rank) {
      nbr[at] = (uint32_t)j;
      continue;
    }
    const uint32_t e = maps[(size_t)q * (size_t)map_stride + 2 + (size_t)j];
    if (e == MRS_NO_SLOT || (long long)e + 1 >= (long long)block) {  // cannot happen (symmetry / capacity checked by the host): keep the entry harmless
      atomicAdd(&fctl[CTL_BADSLOT], 1u);
      nbr[at] = MRS_NBR_FOREIGN | (uint32_t)(q * block);  // the owner's header record: w = stall word, position (0,0,0) + zero constants
      continue;
    }
    const uint32_t slot = (uint32_t)(q * block + 1 + e);
    nbr[at] = MRS_NBR_FOREIGN | slot;
    const PosRecord r = rec_all[g];  // several lanes may write the same slot: same values
    const Pos4         pp = {r.x, r.y, r.z, 0.0};
    const PartnerConst cc = {r.mass, r.arm_length, r.prop_radius, 0.0};
    x_recv[slot]  = pp;
    x_const[slot] = cc;
  }
}

// handleCollisions of the tick after the most recent step, evaluated on its own from the lists (local partners: position records,
// foreign partners: gathered export buffer — both current): the settle step at the end of a run of sharded ticks
// own_from_records: the UAV's own position comes from the position records too (cd.p_in) and crash flags are left alone — the
// force a fused launch evaluated but did not latch (CollDev::write_force == 0), re-derived from the very positions it used
template <bool OWN_FROM_RECORDS>
__global__ void k_list_eval_cd(SwarmDev sw, CollDev cd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sw.n) return;
  const size_t      np = (size_t)sw.npad;
  const TypeParams& P  = sw.T[sw.F[i] >> FLAG_TYPE_SHIFT];
  PosRecord         me;
  if (OWN_FROM_RECORDS) {
    const Pos4 pp = cd.p_in[i];
    me.x = pp.x; me.y = pp.y; me.z = pp.z;
  } else {
    me.x = sw.S[(size_t)(F_X + 0) * np + i];
    me.y = sw.S[(size_t)(F_X + 1) * np + i];
    me.z = sw.S[(size_t)(F_X + 2) * np + i];
  }
  me.mass = P.mass; me.arm_length = P.arm_length; me.prop_radius = P.prop_radius;
  double f[3];
  bool   crashed;
  const uint32_t cnt = cd.nbr_cnt[i];
  double         ox, oy, oz, om, oa, op;
  mrs_partner_flat(cd, cnt ? cd.nbr[i] : (uint32_t)i, ox, oy, oz, om, oa, op);
  mrs_list_eval(cd, i, me.x, me.y, me.z, me.mass, me.arm_length, me.prop_radius, cnt, ox, oy, oz, om, oa, op, f, crashed);
  sw.S[(size_t)(F_FEXT + 0) * np + i] = f[0];
  sw.S[(size_t)(F_FEXT + 1) * np + i] = f[1];
  sw.S[(size_t)(F_FEXT + 2) * np + i] = f[2];
  if (crashed && !OWN_FROM_RECORDS) sw.F[i] |= FLAG_CRASHED;
}

// the stall words of all ranks (headers of the gathered export buffer) folded into this rank's control words: run at the end of a
// batch of ticks, whose last launch nobody has looked behind yet
// progress_tau != 0: also stands in for the fused launch of a rank that holds no UAVs (it reports progress and the warning word)
__global__ void k_fold_stall(const Pos4* x_recv, int world, int block, Pos4* x_send, uint32_t* fctl, volatile uint32_t* hostw, uint32_t progress_tau) {
  uint32_t* own   = (uint32_t*)x_send;  // the rank's own header words (MRS_HDR_*): what it knows, what its next collective carries
  uint32_t  stall = own[MRS_HDR_STALL], warn = own[MRS_HDR_WARN], herr = 0u;
  // (a communicator of ONE rank: the launches keep their words where a single GPU keeps them)
  if (fctl[CTL_STALL] != 0u && (stall == 0u || fctl[CTL_STALL] < stall)) stall = fctl[CTL_STALL];
  if (fctl[CTL_WARN] != 0u && (warn == 0u || fctl[CTL_WARN] < warn)) warn = fctl[CTL_WARN];
  for (int q = 0; q < world; q++) {
    const uint32_t* hq = (const uint32_t*)(x_recv + (size_t)q * (size_t)block);
    const uint32_t  h = hq[MRS_HDR_STALL], wq = hq[MRS_HDR_WARN];
    herr |= hq[MRS_HDR_ERROR];
    if (h != 0u && (stall == 0u || h < stall)) stall = h;
    if (wq != 0u && (warn == 0u || wq < warn)) warn = wq;
  }
  if ((herr & 3u) != 0u) fctl[CTL_ERROR] |= (herr & 3u) << 8;  // some rank's kernels reported an error: every rank's call fails
  own[MRS_HDR_STALL] = stall;
  own[MRS_HDR_WARN]  = warn;
  __hip_atomic_store(&hostw[CTL_STALL], stall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&hostw[CTL_WARN], warn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&hostw[CTL_STALL2], stall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // (nothing else runs: both chains' mirrors agree)
  __hip_atomic_store(&hostw[CTL_WARN2], warn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (progress_tau != 0u && (stall == 0u || progress_tau <= stall))
    __hip_atomic_store(&hostw[CTL_PROGRESS], progress_tau, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

// sizes of the export-set exchange for `world` ranks and `cap` export slots per rank; buffers zeroed (headers!)
// zero == 0: the caller's next launch is the search's reset kernel, which zeroes the allocation itself (one launch less per search)
extern "C" hipError_t mrs_collide_export_prepare(SwarmDev sw, CollideWork** work, int world, long long cap, int zero, hipStream_t st) {
  if (!*work) *work = new CollideWork();
  CollideWork* w = *work;
  CK(ensure_fused(w, sw.n > 0 ? sw.n : 1, st));
  const size_t n_own = sw.n > 0 ? (size_t)sw.n : 0;
  if (n_own > w->exp_slot.capacity()) CK(hipStreamSynchronize(st));
  CK(w->exp_slot.reserve(n_own));
  const size_t n_blocks = ((n_own ? n_own : 1) + 63) / 64;
  if (n_blocks > w->epoch.capacity()) {  // (the last of the three to be allocated)
    CK(hipStreamSynchronize(st));
    for (auto* b : {&w->blk_class, &w->blk_list, &w->epoch}) CK(b->alloc(n_blocks));
    CK(hipMemsetAsync(w->blk_class, 0, sizeof(uint32_t) * n_blocks, st));
    CK(hipMemsetAsync(w->epoch, 0, sizeof(uint32_t) * n_blocks, st));
  }
  if (cap > w->x_cap || world != w->x_world) {
    CK(hipStreamSynchronize(st));
    w->x_cap = 0, w->x_recv = nullptr, w->x_const = nullptr;
    const size_t block = (size_t)cap + 1;
    CK(w->x_send.alloc(block * (size_t)(1 + 2 * world)));  // (one allocation: send block, gathered blocks, partner constants — zeroed by one launch per search)
    w->x_recv  = w->x_send + block;
    w->x_const = (PartnerConst*)(w->x_recv + block * (size_t)world);
    w->x_cap   = cap;
    w->x_world = world;
  }
  const size_t block = (size_t)w->x_cap + 1;
  static_assert(sizeof(Pos4) == sizeof(PartnerConst), "one stride for the three parts of the export allocation");
  if (zero) CK(hipMemsetAsync(w->x_send, 0, sizeof(Pos4) * block * (size_t)(1 + 2 * world), st));
  return hipSuccess;
}

namespace {
__global__ void k_heads_to_host(const uint32_t* maps, long long stride, int world, const uint32_t* fctl, volatile uint32_t* host, const HaloEntry* halo,
                                unsigned hcap) {
  const int q = threadIdx.x;
  {  // the halo headers of a search that ran on a halo exchange: the largest number of entries any rank wanted to send, all flags
    unsigned long long cnt = 0ull, fl = 0ull;
    if (halo && q < world) {
      const HaloEntry h = halo[(size_t)q * (size_t)(1u + hcap)];
      cnt = h.j > 0xFFFFFFFFull ? 0xFFFFFFFFull : h.j;
      fl  = h.pad;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long c2 = __shfl_xor(cnt, o), f2 = __shfl_xor(fl, o);
      cnt = c2 > cnt ? c2 : cnt;
      fl |= f2;
    }
    if (q == 0) {
      __hip_atomic_store(&host[2 * world + 2], (uint32_t)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&host[2 * world + 3], (uint32_t)fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (q < world) {
    __hip_atomic_store(&host[2 * q], maps[(size_t)q * (size_t)stride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host[2 * q + 1], maps[(size_t)q * (size_t)stride + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (q == 0) {
    __hip_atomic_store(&host[2 * world], fctl[CTL_NBND], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host[2 * world + 1], fctl[CTL_NL1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
}  // namespace
// what the host needs of a search — every rank's export count and overflow counter, this rank's boundary-block count — in pinned host
// memory after ONE small launch (two device-to-host copies cost a search 30 us); valid after the stream has been synchronised
// halo != 0: the search ran on a halo exchange; words [2 world + 2] = most entries wanted by a rank, [2 world + 3] = the flags of all ranks
extern "C" hipError_t mrs_collide_heads_to_host(CollideWork* w, const uint32_t* maps, long long stride, int world, int halo, const uint32_t** out, hipStream_t st) {
  if (!w || world > 64) return hipErrorInvalidValue;
  CK(w->host_heads.reserve(160, hipHostMallocMapped | hipHostMallocCoherent));
  hipLaunchKernelGGL(k_heads_to_host, dim3(1), dim3(64), 0, st, maps, stride, world, w->fctl, w->host_heads, halo ? w->h_recv : nullptr, (unsigned)w->h_cap);
  *out = w->host_heads;
  return hipGetLastError();
}

extern "C" const uint32_t* mrs_collide_host_heads(const CollideWork* w) { return w ? w->host_heads : nullptr; }
// a search has replaced the lists: launch indices restart at 1, the pinned mirrors of the control words start from nothing
extern "C" void mrs_collide_host_words_reset(CollideWork* w) {
  if (!w || !w->hostw) return;
  w->hostw[CTL_STALL] = w->hostw[CTL_PROGRESS] = w->hostw[CTL_WARN] = w->hostw[CTL_STALL2] = w->hostw[CTL_WARN2] = 0u;
}
extern "C" long long mrs_collide_export_capacity(const CollideWork* w) { return w ? w->x_cap : 0; }
extern "C" void*     mrs_collide_export_send(const CollideWork* w) { return w ? (void*)w->x_send : nullptr; }
extern "C" void*     mrs_collide_export_recv(const CollideWork* w) { return w ? (void*)w->x_recv : nullptr; }

// after a search over gathered records: mark the export set, write this rank's slot map (2 + n_max words) for the all-gather
// pred_hdt >= 0: also the displacement bound over that time on the state the search found (k_export_mark)
extern "C" hipError_t mrs_collide_export_mark(SwarmDev sw, CollideWork* w, long long n_max, long long map_words, int rank, uint32_t* map_send, double pred_hdt,
                                              double rebounce, hipStream_t st) {
  // (the host mirrors of the control words are reset by the host once it has read what the old segment left in them: mrs_collide_host_words_reset)
  const long long n_xvec = (long long)(sizeof(Pos4) * ((size_t)w->x_cap + 1) * (size_t)(1 + 2 * w->x_world) / sizeof(uint4));
  long long       grid   = (map_words + 255) / 256;
  if (grid < 64) grid = 64;
  hipLaunchKernelGGL(k_search_reset, dim3((unsigned)grid), dim3(256), 0, st, w->fctl, map_send, map_words, w->blk_class, (sw.n + 63) / 64, (uint4*)w->x_send.get(), n_xvec);
  if (sw.n > 0) {
    hipLaunchKernelGGL(k_export_mark, dim3((sw.n + 255) / 256), dim3(256), 0, st, sw, w->P[w->pcur], n_max, rank, w->nbr, w->nbr_cnt, w->exp_slot, map_send,
                       w->fctl, w->blk_class, pred_hdt, skin_pred_lim(SKIN2), rebounce);
    hipLaunchKernelGGL(k_class_list, dim3((sw.n + 255) / 256), dim3(256), 0, st, sw.n, n_max, rank, w->nbr, w->nbr_cnt, w->blk_class, w->blk_list, w->fctl,
                       map_send, w->ctl ? w->ctl : w->fctl);
  } else {
    hipLaunchKernelGGL(k_export_header, dim3(1), dim3(1), 0, st, map_send, w->fctl, w->ctl ? w->ctl : w->fctl);  // (never searched: word 6 of fctl is 0)
  }
  return hipGetLastError();
}

// after the all-gather of the slot maps (and with buffers of sufficient capacity): rewrite the lists, seed the gathered export buffer
extern "C" hipError_t mrs_collide_export_translate(SwarmDev sw, CollideWork* w, long long n_max, long long map_stride, int rank, const uint32_t* maps,
                                                   const PosRecord* rec_all, hipStream_t st) {
  if (sw.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_export_translate, dim3((sw.n + 255) / 256), dim3(256), 0, st, sw.n, n_max, rank, map_stride, (int)(w->x_cap + 1), w->nbr, w->nbr_cnt,
                     maps, rec_all, w->x_recv, w->x_const, w->fctl);
  return hipGetLastError();
}

// CollDev of a sharded fused launch (export-set exchange); rec_own = this rank's records as of the search (gathered buffer + offset)
extern "C" hipError_t mrs_collide_export_dev(const SwarmDev* sw, CollideWork* w, long long my_offset, unsigned tau, int eval, int crash, double rebounce,
                                             CollDev* cd) {
  if (!w || !w->fctl || !w->P[0] || !w->x_send || !w->g_rec_build) return hipErrorInvalidValue;
  memset(cd, 0, sizeof *cd);
  cd->nbr      = w->nbr;
  cd->nbr_cnt  = w->nbr_cnt;
  cd->rec      = w->g_rec_build + my_offset;
  cd->p_in     = w->P[w->pcur];
  cd->p_out    = w->P[(w->pcur + 1) % 3];
  cd->ctl      = w->fctl;
  cd->hostw    = w->hostw;
  cd->g_pos    = w->x_recv;
  cd->g_const  = w->x_const;
  cd->send     = w->x_send;
  cd->exp_slot = w->exp_slot;
  cd->rebounce = rebounce;
  cd->lim2     = skin_lim2(SKIN2);
  cd->lim2_warn = cd->lim2 * (WARN_FRACTION * WARN_FRACTION);  // the warning travels in the collective's headers (tick_sharded.hip: export_ticks)
  cd->tau      = tau;
  cd->n        = sw->n;
  cd->eval     = eval;
  cd->crash    = crash;
  cd->world    = w->x_world;
  cd->block    = (int)(w->x_cap + 1);
  cd->part      = MRS_PART_FULL;
  cd->blk_class = w->blk_class;
  cd->blk_list  = w->blk_list;
  cd->epoch     = w->epoch;
  cd->pred_lim  = skin_pred_lim(SKIN2);
  cd->pred_hdt  = -1.0;  // (nothing announced unless the caller says so: mrs_collide_export_part)
  return hipSuccess;
}

// the part of a split tick this launch is (MRS_PART_*) and the step of the displacement bound
// announce: the protocol runs split ticks (on any rank), so "may leave its skin within MRS_PRED_HORIZON steps" has to be reported ahead
extern "C" void mrs_collide_export_part(CollDev* cd, int part, unsigned n_bnd, double dt, int announce) {
  cd->part          = part;
  cd->n_bnd         = n_bnd;
  cd->pred_hdt      = announce ? (double)MRS_PRED_HORIZON * dt : -1.0;
}

// a run of split ticks starts behind launch `tau` (everything before it has completed in stream order)
extern "C" hipError_t mrs_collide_handoff_init(CollideWork* w, int n, unsigned tau, hipStream_t st) {
  if (!w || !w->epoch) return hipErrorInvalidValue;
  const int n_blocks = (n + 63) / 64;
  hipLaunchKernelGGL(k_handoff_init, dim3((n_blocks + 255) / 256), dim3(256), 0, st, w->fctl, w->epoch, n_blocks, tau);
  return hipGetLastError();
}

extern "C" hipError_t mrs_collide_export_eval(SwarmDev sw, CollDev cd, hipStream_t st) {
  if (sw.n <= 0) return hipSuccess;
  cd.crash = mode_word(sw, cd.crash);
  hipLaunchKernelGGL(k_list_eval_cd<false>, dim3((sw.n + 255) / 256), dim3(256), 0, st, sw, cd);
  return hipGetLastError();
}

// the force of the collision tick a fused launch evaluated without latching it: same lists, same position records (index `pin`)
extern "C" hipError_t mrs_collide_latch_force(SwarmDev sw, CollideWork* w, int pin, int crash, double rebounce, hipStream_t st) {
  if (sw.n <= 0 || !w || !w->P[0]) return hipSuccess;
  CollDev cd;
  memset(&cd, 0, sizeof cd);
  cd.nbr = w->nbr; cd.nbr_cnt = w->nbr_cnt; cd.rec = w->rec_build; cd.p_in = w->P[pin % 3];
  cd.rebounce = rebounce; cd.n = sw.n; cd.eval = 1; cd.crash = mode_word(sw, crash); cd.world = 1;
  hipLaunchKernelGGL(k_list_eval_cd<true>, dim3((sw.n + 255) / 256), dim3(256), 0, st, sw, cd);
  return hipGetLastError();
}

extern "C" hipError_t mrs_collide_export_fold_stall(CollideWork* w, unsigned progress_tau, hipStream_t st) {
  hipLaunchKernelGGL(k_fold_stall, dim3(1), dim3(1), 0, st, w->x_recv, w->x_world, (int)(w->x_cap + 1), w->x_send, w->fctl, w->hostw, progress_tau);
  return hipGetLastError();
}

// collide_work.h — what the units of the collision pass share (collide.hip: searches and neighbour lists; collide_export.hip: the
// export-set exchange of sharded swarms): the geometry of cells, lists and skins, the work object, and the small host helpers both use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "hip_owned.h"
#include "swarm_layout.h"
#include "collide_device.inc"

#define MRS_INTERNAL __attribute__((visibility("hidden")))  // shared by the collision units, no dynamic symbol of the library

// cells are floor(pos * INV_CELL): any consistent assignment with an edge above the search radius works, and the multiply
// avoids three ~70-cycle IEEE divisions per cell_of
constexpr double INV_CELL      = 1.0 / 1.75;  // plain search: edge 1.75 m > sqrt(3.0) = 1.7320508
#ifndef MRS_SKIN
#define MRS_SKIN 0.5  // (compile-time so that the cell arithmetic stays in constants; tools/build_variants.sh sweeps it)
#endif
constexpr double SKIN          = MRS_SKIN;    // neighbour lists: how far apart beyond sqrt(3) a listed pair may be
constexpr double SQRT3_UP      = 1.7320508075688775;                      // >= sqrt(3)
constexpr double INV_CELL_WIDE = 1.0 / (SQRT3_UP + SKIN + 0.0179491924);  // list rebuild: edge 2.25 m > sqrt(3) + SKIN = 2.2320508 (SKIN 0.5)
constexpr double LIST_R2       = (SQRT3_UP + SKIN) * (SQRT3_UP + SKIN) * (1.0 + 1e-9) + 1e-5;  // > (sqrt(3) + SKIN)^2 (4.98206 at SKIN 0.5)
// Sharded swarms keep their lists longer: a search there is two collectives, a host synchronisation and a dozen launches (~200 us
// against 37 us on one GPU), so the wider skin — half as many searches, 1.3 instead of 0.7 listed partners per UAV at 64 m^3 — pays
// (one GPU, SKIN swept: 0.5 m 22.9 us per tick, 1.0 m 23.6).  Mode 2 of the WIDE / LISTS template arguments in collide.hip.
#ifndef MRS_SKIN_SHARDED
#define MRS_SKIN_SHARDED 1.0
#endif
constexpr double SKIN2          = MRS_SKIN_SHARDED;
constexpr double INV_CELL_WIDE2 = 1.0 / (SQRT3_UP + SKIN2 + 0.0179491924);
constexpr double LIST_R2_2      = (SQRT3_UP + SKIN2) * (SQRT3_UP + SKIN2) * (1.0 + 1e-9) + 1e-5;
constexpr double POS_LIMIT     = MRS_POS_LIMIT;  // |coordinate| beyond this (or non-finite) never collides here
// fused evaluation: a UAV beyond this fraction of the distance that invalidates the lists makes the host queue the next search in
// stream order (no stall, no replay); the remaining 25 % (6 cm) are ten ticks at 6 m/s — more than the host runs ahead of the device
MRS_INTERNAL inline const double WARN_FRACTION = getenv("MRS_WARN_FRACTION") ? atof(getenv("MRS_WARN_FRACTION")) : 0.75;
constexpr int    LIST_CAP      = 24;          // listed neighbours per UAV (0.7 expected at 64 m^3 per UAV, 4.6 at 10 m^3: P(> 24) ~ 1e-11;
                                              // with 8, one UAV in 10^4 overflowed at 30 m^3 per UAV and kept a 100 k swarm searching)

// A search is due once a UAV is farther than half the skin from where the lists were built: the squared limit of the skin test ...
constexpr double skin_lim2(double skin) { return (0.5 * skin) * (0.5 * skin) * (1.0 - 1e-9); }
// ... and the limit of the displacement bound that announces it ahead (mrs_may_leave, collide_device.inc)
constexpr double skin_pred_lim(double skin) { return 0.5 * skin * (1.0 - 1e-9); }

// Every buffer is an owner (hip_owned.h) that knows its own size; the capacities kept beside them say how the buffers are laid out
// (cap_n / cap_T: UAVs and slots of the hash tables; h_cap / x_cap: entries per block of the halo and export allocations).
struct CollideWork {
  long long cap_n = 0;
  uint32_t  cap_T = 0;
  int       cur   = 0;  // which head table the next tick fills; the other one is being wiped by that tick's query
  DevBuf<uint2> head[2], next;
  // neighbour lists (single-GPU ticks)
  DevBuf<PosRecord> rec_build;     // records of the last rebuild: reference positions of the skin test + airframe constants
  DevBuf<uint32_t>  nbr, nbr_cnt, ctl;
  int        fcur = 0;             // which of ctl[0..1] the next tick reads
  bool       lists_live = false;   // rec_build / nbr describe this swarm as of some earlier tick
  DevBuf<double>    g_bbox;          // gathered mode: this rank's bounding box widened by the list radius (6 doubles)
  DevBuf<PosRecord> g_rec_build;     // gathered mode: all records as of this rank's last rebuild
  bool       g_lists_live = false;
  // halo exchange of a search tick (mrs_collide_halo_*): instead of every rank's ALL records, the records that can be within the list
  // radius of another rank's UAVs travel — [header | entries] of 64 B, the header's `j` = count, `pad` = flags
  DevBuf<HaloEntry> h_send;      // [1 + h_cap], then h_recv (one allocation for all blocks together, headers included)
  HaloEntry* h_recv = nullptr;   // [world][1 + h_cap]
  long long  h_cap = 0;          // entries per block in use
  int        h_world = 0;
  DevBuf<uint32_t> h_ctl;        // [0] entries appended, [1] flags (MRS_HALO_*)
  double*    g_box_out = nullptr;  // where a search of the export-set exchange also leaves its box (mrs_collide_set_box_out): borrowed
  DevBuf<double> h_part;           // partial boxes of k_halo_select, 6 doubles per block
  bool       g_export_form = false;  // the last gathered search was one of the export-set exchange: lists end up in slot form, and of
                                     // the record copy only this rank's own range (the skin references) is kept
  // fused step + collision evaluation (step_device.inc *_coll): double-buffered positions, control words, pinned host mirror
  // (three buffers: in a split sharded tick the interior launch of tick t+1 writes its output while the boundary launch of tick t
  //  still reads its input — with two buffers those would be the same array)
  DevBuf<Pos4> P[3];
  int       pcur  = 0;        // P[pcur] holds the positions after the most recent step (when the host says they are valid)
  DevBuf<uint32_t>    fctl;   // CTL_WORDS device words
  PinnedBuf<uint32_t> hostw;  // CTL_WORDS pinned host words (stall, progress mirrored by the kernels)
  // export-set exchange (multi-GPU ticks between searches): own UAVs listed by another rank, their slots in the padded collective
  DevBuf<uint32_t> exp_slot;          // [n_local]
  // split sharded ticks: class of every 64-UAV block, list of the boundary blocks, epoch word per block (swarm_layout.h)
  DevBuf<uint32_t>    blk_class, blk_list, epoch;
  PinnedBuf<uint32_t> host_heads;     // heads of the slot maps + boundary-block count of the last search
  DevBuf<Pos4>  x_send;               // [1 + x_cap]: header + exported positions of this rank, then x_recv and x_const (one allocation)
  Pos4*         x_recv = nullptr;     // [world][1 + x_cap]
  PartnerConst* x_const = nullptr;    // [world][1 + x_cap]
  long long     x_cap = 0;            // export slots per rank in the collective
  int           x_world = 0;
};

// the mode word the collision code passes around as `crash` (collide_device.inc): the flavour of the force expression follows the swarm
static inline int mode_word(const SwarmDev& sw, int crash) { return (crash ? MRS_MODE_CRASH : 0) | (sw.fast ? MRS_MODE_FAST : 0); }

#define CK(e)                        \
  do {                               \
    hipError_t _e = (e);             \
    if (_e != hipSuccess) return _e; \
  } while (0)

// buffers of the fused step + collision evaluation for n local UAVs (collide.hip)
MRS_INTERNAL hipError_t ensure_fused(CollideWork* w, long long n, hipStream_t st);

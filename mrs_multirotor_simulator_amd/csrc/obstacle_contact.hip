// obstacle_contact.hip — obstacle contacts (include/mrs_swarm.h, "obstacle contacts"): which UAVs touch a static obstacle, as a sphere of
// radius arm_length + prop_radius (+ a margin) against the signed distances of the static obstacles, reported in dense device vectors and,
// under MRS_CONTACT_CRASH, marked crashed as UavSystem::crash() marks them (uav_system.hpp:278) — the one producer of FLAG_CRASHED that
// looks at the scenery.  One lane per UAV reads the ONE grid cell that contains its position (obstacle_grid.h; the contacts' own cache
// entry of the set, built for R = fl(rmax + margin) >= every UAV's threshold), tests every obstacle listed there literally (world rule,
// sd < thr_i) and folds it into three registers: count, best sd, best index (obstacle_contact.h, the functions the host-side test
// compiles).  No list, no LDS, no atomics: a lane owns its UAV's outputs and its flag word.  The walk is mrs_obst::walk_cell, the
// callable form both range scans use.
// Without MRS_CONTACT_CRASH nothing here writes simulation state and the call enters like mrs_swarm_obstacle_cost_device (a pending
// collision tick stays pending); with it the flag word is written and the call enters like mrs_swarm_crash (the tick is evaluated first).
#include "host_internal.h"
#include "obstacle_contact.h"
#include "obstacle_set.h"

namespace {

constexpr int OC_BLOCK = 256;

struct ContactArgs {
  const double*      S;
  uint32_t*          F;
  const TypeParams*  T;
  const uint32_t*    wlab;  // null: every UAV is in world 0
  int32_t            npad, first, count;
  uint32_t           crash;  // FLAG_CRASHED under MRS_CONTACT_CRASH, else 0
  double             margin, hit_cost;
  mrs_obst::GridView v;
  uint8_t*           hit;     // every output may be null
  int32_t*           index;
  double*            sd;
  int32_t*           counts;
  double*            cost;
};

__global__ void __launch_bounds__(OC_BLOCK) k_obst_contact(ContactArgs a) {
  const int q = blockIdx.x * OC_BLOCK + threadIdx.x;
  if (q >= a.count) return;
  const int         i    = a.first + q;
  const size_t      np   = (size_t)a.npad;
  const double      p[3] = {a.S[(size_t)F_X * np + i], a.S[(size_t)(F_X + 1) * np + i], a.S[(size_t)(F_X + 2) * np + i]};
  const uint32_t    myw  = a.wlab ? a.wlab[i] : 0u;
  const uint32_t    f    = a.F[i];
  const TypeParams& tp   = a.T[f >> FLAG_TYPE_SHIFT];
  const double      thr  = mrs_obst::contact_threshold(mrs_obst::contact_radius(tp.arm_length, tp.prop_radius), a.margin);
  const mrs_obst::Contact c   = mrs_obst::contact_search(a.v, p, myw, thr);
  const bool              hit = c.count > 0;
  if (a.hit) a.hit[q] = hit ? 1 : 0;
  if (a.index) a.index[q] = mrs_obst::contact_index(c);
  if (a.sd) a.sd[q] = mrs_obst::contact_sd(c);
  if (a.counts) a.counts[q] = c.count;
  if (hit) {  // (a UAV that touches nothing has no byte of its cost element or of its state rewritten)
    if (a.cost) a.cost[q] = a.cost[q] + a.hit_cost;
    if (a.crash) a.F[i] = f | a.crash;
  }
}

}  // namespace

extern "C" {

int mrs_swarm_obstacle_contacts_device(mrs_swarm_t* s, int32_t first, int32_t count, double margin, uint32_t flags, uint8_t* dev_hit,
                                       int32_t* dev_index, double* dev_sd, int32_t* dev_count, double* dev_cost, double hit_cost, void* ext_stream) {
  // the marking form writes the flag word: a pending collision tick is evaluated first (mrs_swarm_crash); the read-only form leaves it
  // pending (mrs_swarm_obstacle_cost_device)
  MRS_LOCK(s);
  if (s && (flags & (uint32_t)MRS_CONTACT_CRASH)) {
    int rc = settle(s);
    if (rc) return rc;
  } else if (s && !s->log.empty()) {
    if (hipSetDevice(s->device) != hipSuccess) return fail(MRS_ERR_HIP, "hipSetDevice");
    int rc = mrs_host::drain(s);
    if (rc) return rc;
  }
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_obstacle_contacts_device: not on a sharded swarm");
  if (flags & ~(uint32_t)MRS_CONTACT_CRASH) return fail(MRS_ERR_ARG, "unknown contact flag bits");
  if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(MRS_ERR_ARG, "margin must be finite and >= 0");
  if (dev_cost && !std::isfinite(hit_cost)) return fail(MRS_ERR_ARG, "hit_cost must be finite");
  if (!dev_hit && !dev_index && !dev_sd && !dev_count && !dev_cost && !(flags & (uint32_t)MRS_CONTACT_CRASH))
    return fail(MRS_ERR_ARG, "nothing to do (no output given and no MRS_CONTACT_CRASH)");
  // the grid's radius: the largest finite body radius of the airframe table, and the margin — every UAV's threshold is at most that
  double rmax = 0.0;
  for (const TypeParams& tp : s->tparams) {
    const double rad = mrs_obst::contact_radius(tp.arm_length, tp.prop_radius);
    if (std::isfinite(rad) && rad > rmax) rmax = rad;
  }
  const double R = mrs_obst::contact_threshold(rmax, margin);
  if (!(R > 0.0) || !std::isfinite(R)) return fail(MRS_ERR_ARG, "the largest body radius + margin must be finite and > 0");
  if (count == 0) return MRS_OK;
  if (dev_hit && (rc = check_device_ptr(s, dev_hit, (size_t)count, "dev_hit"))) return rc;
  if (dev_index && (rc = check_device_ptr(s, dev_index, index_rows_bytes(count, 1, 1), "dev_index"))) return rc;
  if (dev_sd && (rc = check_device_ptr(s, dev_sd, (size_t)count * sizeof(double), "dev_sd"))) return rc;
  if (dev_count && (rc = check_device_ptr(s, dev_count, index_rows_bytes(count, 1, 1), "dev_count"))) return rc;
  if (dev_cost && (rc = check_device_ptr(s, dev_cost, (size_t)count * sizeof(double), "dev_cost"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  // the body radii are read from the airframe table: current before the launch
  if ((rc = upload_types(s, s->table_dt > 0 ? s->table_dt : 0.001))) return rc;
  if ((rc = contact_grid(s, R))) return rc;
  if ((rc = fence_in(s, ext))) return rc;
  ContactArgs a;
  memset(&a, 0, sizeof a);
  a.S        = s->dS;
  a.F        = s->dF;
  a.T        = s->dT;
  a.wlab     = s->dWorld;
  a.npad     = s->npad;
  a.first    = first;
  a.count    = count;
  a.crash    = (flags & (uint32_t)MRS_CONTACT_CRASH) ? FLAG_CRASHED : 0u;
  a.margin   = margin;
  a.hit_cost = hit_cost;
  a.v        = grid_view(*s->obst, s->obst->contact);
  a.hit      = dev_hit;
  a.index    = dev_index;
  a.sd       = dev_sd;
  a.counts   = dev_count;
  a.cost     = dev_cost;
  hipLaunchKernelGGL(k_obst_contact, dim3((unsigned)((count + OC_BLOCK - 1) / OC_BLOCK)), dim3(OC_BLOCK), 0, s->stream, a);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

}  // extern "C"

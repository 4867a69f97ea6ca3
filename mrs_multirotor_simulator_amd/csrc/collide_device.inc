// collide_device.inc — device functions shared by collide.hip (searches), collide_export.hip (standalone list evaluation) and step_device.inc (the
// collision evaluation fused into the step kernels): the literal predicate and force expression of
// MultirotorSimulator::handleCollisions, src/multirotor_simulator.cpp:321-358.
// Contraction is switched off inside these functions and the FAST force expression is spelled out in explicit fma / rsq / rcp
// operations, so every translation unit evaluates a flavour with the same operations: a tick gives the same bits whichever
// kernel happens to evaluate it (a fused step launch, the stand-alone pass, mrs_collide_latch_force).  The flavour follows the
// SWARM: the step kernels know it at compile time (MRS_FAST), collide*.hip get it at run time in bit 1 of the `crash` mode word
// (MRS_MODE_FAST, set at its extern "C" boundary from SwarmDev::fast) — a FAST swarm's stand-alone passes use the FAST expression too,
// so get_external_force reports the force the step consumed and a run does not depend on which path evaluated which tick.
#pragma once
#include "swarm_layout.h"
#include "pose_math.h"  // mrs_unfused

#define CDEV static __device__ __forceinline__

// mode word passed as `crash` through the collision code: bit 0 = collisions_crash, bit 1 = FAST force expression
#define MRS_MODE_CRASH 1
#define MRS_MODE_FAST  2

// ---- words shared between launches that run CONCURRENTLY (split sharded ticks: interior launches on one stream, boundary launches
// and the collective on another — DESIGN §5).  cdna_hip_programming.md §6 Guideline 16: every shared word is an agent-scope access
// to global memory, never a plain load or store; payload that another running launch reads (the position records) is stored
// write-through (sc1) and drained before the word that announces it; a consumer polls relaxed, then ONE agent-scope acquire.
typedef __attribute__((address_space(1))) uint32_t           mrs_gu32;
typedef __attribute__((address_space(1))) unsigned long long mrs_gu64;
#define MRS_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
CDEV uint32_t word_load(const uint32_t* p) { return __hip_atomic_load((mrs_gu32*)p, MRS_RLX_AGENT); }
CDEV void     word_store(uint32_t* p, uint32_t v) { __hip_atomic_store((mrs_gu32*)p, v, MRS_RLX_AGENT); }
// *p = the smaller non-zero of (*p, v); 0 stands for "none".  Rare path (a UAV near the edge of its skin).
CDEV void word_min_nz(uint32_t* p, uint32_t v) {
  uint32_t old = word_load(p);
  while (old == 0u || v < old)
    if (__hip_atomic_compare_exchange_strong((mrs_gu32*)p, &old, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
}
// the same on a header field of the export block (a tick index kept as a double: positive doubles order like their bit patterns)
CDEV void header_min_nz(double* p, uint32_t v) {
  const unsigned long long nv  = (unsigned long long)__builtin_bit_cast(long long, (double)v);
  unsigned long long       old = __hip_atomic_load((mrs_gu64*)p, MRS_RLX_AGENT);
  while (old == 0ull || nv < old)
    if (__hip_atomic_compare_exchange_strong((mrs_gu64*)p, &old, nv, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
}
// Bounded wait of ONE lane for *word >= val (10 s of the 100 MHz wall clock — a rank's boundary chain stands still while a PEER is
// late for the collective, and a peer's host can be descheduled for a long time; the bound is only there so that a lost launch
// ends in an error instead of a hung device): on a timeout bit 0 of the error word is set — the host turns it into MRS_ERR_HIP —
// and every later wait gives up at once, so the grid drains.
#ifndef MRS_WAIT_TICKS  // (throw-away measurement builds set 0: every wait gives up at once — wrong results, the timing of launches that wait for nobody)
#define MRS_WAIT_TICKS 1000000000ll
#endif
// err_hdr (may be null): the error word in the header of the rank's export block — what the next collective shows the other ranks
CDEV void raise_error(uint32_t* err, uint32_t* err_hdr, uint32_t bits) {
  __hip_atomic_fetch_or((mrs_gu32*)err, bits, MRS_RLX_AGENT);
  if (err_hdr) __hip_atomic_fetch_or((mrs_gu32*)err_hdr, bits, MRS_RLX_AGENT);
}
CDEV bool word_wait_ge(const uint32_t* word, uint32_t val, uint32_t* err, uint32_t* err_hdr = nullptr) {
  if (word_load(word) >= val) return true;
  const long long t0 = wall_clock64();
  for (;;) {
    __builtin_amdgcn_s_sleep(2);
    if (word_load(word) >= val) return true;
    if ((word_load(err) & 1u) != 0u || wall_clock64() - t0 > MRS_WAIT_TICKS) {
      raise_error(err, err_hdr, 1u);
      return false;
    }
  }
}
constexpr double MRS_POS_LIMIT = 1.0e9;  // |coordinate| beyond this (or non-finite) never collides here

CDEV bool mrs_pos_usable(double x, double y, double z) {
  return (fabs(x) < MRS_POS_LIMIT) && (fabs(y) < MRS_POS_LIMIT) && (fabs(z) < MRS_POS_LIMIT);  // false for NaN/inf
}

// The displacement bound behind the announced stall indices of a sharded swarm (DESIGN §5): may the UAV be farther than `lim` from
// its reference position (squared distance now: dd) within the next h steps, hdt = h * dt?  Over h steps of RK4 from this state it
// moves at most hdt |v| + hdt^2 / 2 * A with |acceleration| <= A = a0 + drag (|v| + hdt a0)^2, a0 = g + 1.5 (thrust cap + thrust now) / m
// + (listed partners) |rebounce| (tests/test_displacement_bound.py) — valid while R stays near a rotation, the rates stay moderate and
// neither the ground nor the take-off patch can lift the UAV; whoever fails those tests counts as "may leave".  y: x v R(row-major) omega.
// Thrust over the horizon: every motor's low-pass moves its speed towards an input within [min_rpm, max_rpm], so a speed stays below
// max(its value now, max_rpm) and, the thrust column being non-negative, allocation * rpm^2 <= (thrust now) + sum_m alloc[3][m] max_rpm^2
// — also for motor speeds the host SET beyond max_rpm (a non-finite thrust makes the bound non-finite: "may leave").
// Used by the step kernels' epilogue (every launch, h = MRS_PRED_HORIZON) and by the search (collide_export.hip k_export_mark: the ticks right
// after a search need no serial phase when nobody can leave within the horizon).
CDEV bool mrs_may_leave(const double y[18], double dd, double thrust_now, uint32_t listed, double rebounce, double hdt, double lim, double pa0, double pthr,
                        double pdrag, int ground_enabled, double ground_z, bool takeoff, double init_z) {
  const double vv  = (y[3] * y[3] + y[4] * y[4]) + y[5] * y[5];
  const double vn  = (double)__builtin_sqrtf((float)vv) * 1.000001 + 1e-30;  // >= |v| (float rounding covered)
  const double a0  = (pa0 + pthr * fabs(thrust_now)) + (double)listed * fabs(rebounce);
  const double vm  = vn + hdt * a0;
  const double A   = a0 + pdrag * (vm * vm);
  const double disp = hdt * vn + 0.5 * (hdt * hdt) * A;
  const double room = lim - disp;
  bool ok = room > 0.0 && dd <= room * room;
  // R near a rotation: its third column at a good angle to the other two (the re-orthonormalised body z is c3 / sin of that angle)
  const double n1 = (y[6] * y[6] + y[9] * y[9]) + y[12] * y[12], n2 = (y[7] * y[7] + y[10] * y[10]) + y[13] * y[13],
               n3 = (y[8] * y[8] + y[11] * y[11]) + y[14] * y[14];
  const double d13 = (y[6] * y[8] + y[9] * y[11]) + y[12] * y[14], d23 = (y[7] * y[8] + y[10] * y[11]) + y[13] * y[14];
  ok = ok && n3 > 0.25 && n3 < 4.0 && d13 * d13 <= 0.05 * (n1 * n3) && d23 * d23 <= 0.05 * (n2 * n3);
  const double ww = (y[15] * y[15] + y[16] * y[16]) + y[17] * y[17];
  ok = ok && (hdt * hdt) * ww <= 0.64;  // |omega| h dt <= 0.8 rad over the horizon
  if (ground_enabled) ok = ok && y[2] >= ground_z;  // (a UAV below the ground is lifted onto it)
  if (takeoff) ok = ok && y[2] >= init_z;           // (... or onto its spawn height)
  return !ok;
}

// nanoflann's squared distance (L2_Adaptor::evalMetric, nanoflann.hpp:443-486), ((0 + d0^2) + d1^2) + d2^2, every product rounded on its
// own: the neighbour set and the contacts hang on strict comparisons of this number, and one fused product moves a pair that sits
// on a threshold across it.  The pragma keeps the sum apart in the units compiled with -ffp-contract=off; in the FAST step unit
// (-ffp-contract=fast) the backend fuses every multiply-add whatever the pragma says, so there the products go through mrs_unfused
// (pose_math.h).  tests/test_collision_thresholds_gpu.py holds every kernel to it.
CDEV double mrs_dist2(double d0, double d1, double d2) {
#pragma clang fp contract(off)
  return ((0.0 + mrs_unfused(d0 * d0)) + mrs_unfused(d1 * d1)) + mrs_unfused(d2 * d2);
}

// Scalar forms (the struct forms below forward to them): the fused evaluation keeps the partner in registers, and a struct-valued
// loop variable made of values from two address spaces ends up in scratch memory behind a generic pointer.
// nanoflann RadiusResultSet(3.0) on the SQUARED distance (:326, nanoflann.hpp:273-305), then the reference's d^2 < crit (:346);
// crash mode is evaluated from the partner's side (this UAV is crashed iff some j has it as a qualifying partner)
CDEV bool mrs_qualifies_s(double mx, double my, double mz, double marm, double mprop, double ox, double oy, double oz, double oarm, double oprop,
                          int crash) {
#pragma clang fp contract(off)
  const double d0 = mx - ox, d1 = my - oy, d2 = mz - oz;
  const double dist = mrs_dist2(d0, d1, d2);
  if (!(dist < 3.0)) return false;
  const double crit_ij = ((marm + mprop) + oarm) + oprop;
  const double crit_ji = ((oarm + oprop) + marm) + mprop;
  return dist < crit_ij || ((crash & MRS_MODE_CRASH) && dist < crit_ji);
}

// accumulate one partner into the force / crash state of a UAV (literal predicate and force expression, :342-350)
CDEV void mrs_apply_partner_s(double mx, double my, double mz, double mmass, double marm, double mprop, double ox, double oy, double oz, double omass,
                              double oarm, double oprop, int crash, double rebounce, double& fx, double& fy, double& fz, bool& crashed) {
#pragma clang fp contract(off)
  const double d0 = mx - ox, d1 = my - oy, d2 = mz - oz;
  const double dist    = mrs_dist2(d0, d1, d2);
  const double crit_ij = ((marm + mprop) + oarm) + oprop;
  const double crit_ji = ((oarm + oprop) + marm) + mprop;
#if defined(MRS_FAST)
  const bool fastf = MRS_FAST != 0;  // step kernels: the flavour of the translation unit
#else
  const bool fastf = (crash & MRS_MODE_FAST) != 0;
#endif
  if (crash & MRS_MODE_CRASH) {
    if (dist < crit_ji) crashed = true;
  } else if (dist < crit_ij) {
    double r0 = d0, r1 = d1, r2 = d2;
    const double z = (r0 * r0 + r1 * r1) + r2 * r2;  // Eigen normalized()
    double       ratio;
    if (fastf) {
      // FAST swarms: reciprocal square root / reciprocal with one third-order correction step each (~1 ulp) instead of an IEEE
      // sqrt and four IEEE divisions — the evaluation runs in nearly every wave (some lane touches somebody) and those five macro
      // sequences are most of its instructions.  LITERAL swarms keep the literal form.
      if (z > 0) {
        const double y = __builtin_amdgcn_rsq(z), e = __builtin_fma(-z * y, y, 1.0);
        const double inv = __builtin_fma(y * e, __builtin_fma(0.375, e, 0.5), y);
        r0 *= inv; r1 *= inv; r2 *= inv;
      }
      const double ms = mmass + omass, yr = __builtin_amdgcn_rcp(ms), er = __builtin_fma(-ms, yr, 1.0);
      ratio = omass * __builtin_fma(yr, __builtin_fma(er, er, er), yr);
    } else {
      if (z > 0) {
        const double nn = sqrt(z);
        r0 /= nn; r1 /= nn; r2 /= nn;
      }
      ratio = omass / (mmass + omass);
    }
    fx += ((rebounce * r0) * mmass) * ratio;
    fy += ((rebounce * r1) * mmass) * ratio;
    fz += ((rebounce * r2) * mmass) * ratio;
  }
}

CDEV bool mrs_qualifies(const PosRecord& me, const PosRecord& o, int crash) {
  return mrs_qualifies_s(me.x, me.y, me.z, me.arm_length, me.prop_radius, o.x, o.y, o.z, o.arm_length, o.prop_radius, crash);
}
CDEV void mrs_apply_partner(const PosRecord& me, const PosRecord& o, int crash, double rebounce, double& fx, double& fy, double& fz,
                            bool& crashed) {
  mrs_apply_partner_s(me.x, me.y, me.z, me.mass, me.arm_length, me.prop_radius, o.x, o.y, o.z, o.mass, o.arm_length, o.prop_radius, crash, rebounce, fx,
                      fy, fz, crashed);
}

// partner of a neighbour-list entry as the fused evaluation sees it: position after the previous step (local: the double-buffered
// position records; foreign: the gathered export buffer), airframe constants as of the last search
template <class CD>
CDEV PosRecord mrs_partner_record(CD& cd, uint32_t e) {
  PosRecord o;
  if (e & MRS_NBR_FOREIGN) {
    const uint32_t     slot = e & ~MRS_NBR_FOREIGN;
    const Pos4         p    = cd.g_pos[slot];
    const PartnerConst c    = cd.g_const[slot];
    o.x = p.x; o.y = p.y; o.z = p.z;
    o.mass = c.mass; o.arm_length = c.arm_length; o.prop_radius = c.prop_radius;
  } else {
    const Pos4 p = cd.p_in[e];
    o            = cd.rec[e];
    o.x = p.x; o.y = p.y; o.z = p.z;
  }
  return o;
}

// the same as six scalars, with both loads issued unconditionally from addresses that are valid for every lane (no divergent
// branch around a load: the step kernel issues this early and consumes it long after)
template <class CD>
CDEV void mrs_partner_flat(CD& cd, uint32_t e, double& ox, double& oy, double& oz, double& om, double& oa, double& op) {
  const bool     foreign = (e & MRS_NBR_FOREIGN) != 0u;
  const uint32_t k       = e & ~MRS_NBR_FOREIGN;
  const Pos4*    pp      = foreign ? cd.g_pos + k : cd.p_in + k;
  const double*  cc      = foreign ? &cd.g_const[k].mass : &cd.rec[k].mass;  // {mass, arm_length, prop_radius} in both layouts
  ox = pp->x; oy = pp->y; oz = pp->z;
  om = cc[0]; oa = cc[1]; op = cc[2];
}

// handleCollisions for UAV i from its neighbour list (ascending partner order); (mx, my, mz) = the UAV's own CURRENT position;
// o1*: the partner of the first entry, fetched by the caller (mrs_partner_flat)
template <class CD>
CDEV void mrs_list_eval(CD& cd, int i, double mx, double my, double mz, double mmass, double marm, double mprop, uint32_t cnt, double o1x,
                        double o1y, double o1z, double o1m, double o1a, double o1p, double f[3], bool& crashed) {
  double fx = 0.0, fy = 0.0, fz = 0.0;
  bool   hit = false;
  if (cnt != 0 && mrs_pos_usable(mx, my, mz)) {
    double ox = o1x, oy = o1y, oz = o1z, om = o1m, oa = o1a, op = o1p;
    for (uint32_t k = 0;;) {
      if (mrs_pos_usable(ox, oy, oz) && mrs_qualifies_s(mx, my, mz, marm, mprop, ox, oy, oz, oa, op, cd.crash))
        mrs_apply_partner_s(mx, my, mz, mmass, marm, mprop, ox, oy, oz, om, oa, op, cd.crash, cd.rebounce, fx, fy, fz, hit);
      if (++k >= cnt) break;
      mrs_partner_flat(cd, cd.nbr[(size_t)k * (size_t)cd.n + (size_t)i], ox, oy, oz, om, oa, op);
    }
  }
  f[0] = fx; f[1] = fy; f[2] = fz;
  crashed = hit;
}

// ---- wide form used by the fused step kernels ---------------------------------------------------------------------------------
// The first MRS_NPRE listed partners of a UAV are fetched in two rounds of INDEPENDENT loads — entries (rows of the list, addresses
// known from the UAV index alone) with the state, position records once the entries are in — and evaluated from registers; a
// partner-by-partner walk pays two dependent memory round trips per list level, and with 0.7 listed partners per UAV (64 m^3 per
// UAV) almost every wave holds a lane with three of them (+3.4 us per launch at 100 k UAVs).  A position record carries the
// airframe type of its UAV in .w, so the constants of a LOCAL partner come from the type table (or are the UAV's own when the
// types agree: no load at all in a single-airframe swarm); a FOREIGN partner's constants sit next to its export slot.
#define MRS_NPRE 4

// position record (+ type id) of list entry e; `live` false: record 0 (one broadcast load for the lanes that have no such entry)
// COHERENT: the record may have been written by a launch that runs beside this one (split sharded ticks) — agent-scope (sc1) loads,
// which bypass this CU's L1, in place of an acquire fence per wave (the fence invalidates the whole L1 once per polling wave: with
// eight single-wave blocks per CU that cost the boundary launch 13 of its 20 us; the records were stored sc1 and drained before
// their block's epoch word was: cdna_hip_programming.md §6 Guideline 16, R1 with every load of the handed-off bytes sc1)
template <bool COHERENT = false, class CD>
CDEV void mrs_partner_pos(CD& cd, uint32_t e, bool live, double& ox, double& oy, double& oz, double& ow) {
  const bool     foreign = live && (e & MRS_NBR_FOREIGN) != 0u;
  const uint32_t k       = live ? (e & ~MRS_NBR_FOREIGN) : 0u;
  const Pos4*    pp      = foreign ? cd.g_pos + k : cd.p_in + k;
  if (COHERENT) {
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    const gu64* q = (const gu64*)(const void*)pp;
    ox = __builtin_bit_cast(double, __hip_atomic_load(q + 0, MRS_RLX_AGENT));
    oy = __builtin_bit_cast(double, __hip_atomic_load(q + 1, MRS_RLX_AGENT));
    oz = __builtin_bit_cast(double, __hip_atomic_load(q + 2, MRS_RLX_AGENT));
    ow = __builtin_bit_cast(double, __hip_atomic_load(q + 3, MRS_RLX_AGENT));
  } else {
    ox = pp->x; oy = pp->y; oz = pp->z; ow = pp->w;
  }
}

// one partner whose position is in registers: nanoflann's radius filter first (positions only), constants on demand
template <class CD>
CDEV void mrs_eval_partner(CD& cd, const TypeParams* T, uint32_t my_type, uint32_t e, double mx, double my, double mz, double mmass, double marm,
                           double mprop, double ox, double oy, double oz, double ow, double& fx, double& fy, double& fz, bool& hit) {
  if (!mrs_pos_usable(ox, oy, oz)) return;
  {
#pragma clang fp contract(off)
    const double d0 = mx - ox, d1 = my - oy, d2 = mz - oz;
    if (!(mrs_dist2(d0, d1, d2) < 3.0)) return;
  }
  double om = mmass, oa = marm, op = mprop;
  if (e & MRS_NBR_FOREIGN) {
    const PartnerConst c = cd.g_const[e & ~MRS_NBR_FOREIGN];
    om = c.mass; oa = c.arm_length; op = c.prop_radius;
  } else {
    const uint32_t ot = (uint32_t)ow;
    if (ot != my_type) {
      const TypeParams& Q = T[ot];
      om = Q.mass; oa = Q.arm_length; op = Q.prop_radius;
    }
  }
  if (mrs_qualifies_s(mx, my, mz, marm, mprop, ox, oy, oz, oa, op, cd.crash))
    mrs_apply_partner_s(mx, my, mz, mmass, marm, mprop, ox, oy, oz, om, oa, op, cd.crash, cd.rebounce, fx, fy, fz, hit);
}

// handleCollisions for UAV i from its list: entries / positions of the first MRS_NPRE partners in registers, the rest fetched one by one
template <class CD>
CDEV void mrs_list_eval_wide(CD& cd, const TypeParams* T, uint32_t my_type, int i, double mx, double my, double mz, double mmass, double marm, double mprop,
                             uint32_t cnt, const uint32_t (&e)[MRS_NPRE], const double (&ox)[MRS_NPRE], const double (&oy)[MRS_NPRE],
                             const double (&oz)[MRS_NPRE], const double (&ow)[MRS_NPRE], double f[3], bool& crashed) {
  double fx = 0.0, fy = 0.0, fz = 0.0;
  bool   hit = false;
  if (cnt != 0 && mrs_pos_usable(mx, my, mz)) {
#pragma unroll
    for (int k = 0; k < MRS_NPRE; k++)
      if ((uint32_t)k < cnt) mrs_eval_partner(cd, T, my_type, e[k], mx, my, mz, mmass, marm, mprop, ox[k], oy[k], oz[k], ow[k], fx, fy, fz, hit);
    for (uint32_t k = MRS_NPRE; k < cnt; k++) {  // dense neighbourhoods only
      const uint32_t ek = cd.nbr[(size_t)k * (size_t)cd.n + (size_t)i];
      double         px, py, pz, pw;
      if (cd.part != MRS_PART_FULL) {  // split sharded tick: the partner may be stepped by the launch on the other stream
        if (!(ek & MRS_NBR_FOREIGN)) word_wait_ge(&cd.epoch[ek >> 6], cd.tau - 1u, &cd.ctl[CTL_ERROR], (uint32_t*)cd.send + MRS_HDR_ERROR);
        mrs_partner_pos<true>(cd, ek, true, px, py, pz, pw);
      } else {
        mrs_partner_pos(cd, ek, true, px, py, pz, pw);
      }
      mrs_eval_partner(cd, T, my_type, ek, mx, my, mz, mmass, marm, mprop, px, py, pz, pw, fx, fy, fz, hit);
    }
  }
  f[0] = fx; f[1] = fy; f[2] = fz;
  crashed = hit;
}

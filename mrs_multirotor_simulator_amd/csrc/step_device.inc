// step_device.inc — the fused UAV step: controller cascade -> mixer -> RK4 rigid body -> post-step.
//
// Included twice: step_kernel_literal.hip (MRS_FAST 0, compiled -ffp-contract=off) and
// step_kernel_fast.hip (MRS_FAST 1, -ffp-contract=fast).  One lane = one UAV; a wavefront handles 64
// consecutive UAVs of the SoA state (coalesced 512-B field loads).  Per-type constants are read through
// the scalar cache with the block's type id (64-UAV blocks that mix airframes go to the *_mixed kernels).
// Kernel family (see the end of the file): {cascade, model-only, mixed} x {single step, fused sub-steps} x
// {pointer-, buffer-addressed columns} + three-wave (160-register) builds of the buffer-addressed single-step kernels.
//
// Replaces (paths relative to /root/reference/include/mrs_multirotor_simulator/uav_system):
//   uav_system.hpp:304-380 (UavSystem::makeStep), multirotor_model.hpp:220-286,301-366,392-410,
//   controllers/{pid,mixer,rate_controller,attitude_controller,acceleration_controller,
//   velocity_controller,position_controller}.hpp, and odeint's runge_kutta4 (generic_rk_algorithm.hpp:190-216).
//
// LITERAL flavour: every floating-point operation of the reference is performed in the reference's
// order, with these bit-preserving shortcuts (finite inputs; only the sign of an exact zero can differ):
//   * products with structural zeros are skipped (0*x + y == y): R*omega_tensor, cofactors of the
//     lower-triangular Cholesky factor, the B-matrix products of the acceleration controller, the
//     zero-weight RK4 terms (a non-finite k_i still poisons the stage value with NaN like 0*inf does);
//   * stage-invariant values are computed once per step: allocation*rpm^2, J^-1, F_ext/mass.
// FAST flavour additionally: FMA contraction, x/mass -> x*(1/mass), 1/dt hoisted in the PIDs,
// triangular inverse of the Cholesky factor via reciprocals, normalisation by reciprocal.

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>
#include "swarm_layout.h"
#include "collide_device.inc"

#ifndef MRS_FAST
#error "define MRS_FAST to 0 or 1"
#endif

#if MRS_FAST
#define KNAME(x) x##_fast
#else
#define KNAME(x) x##_literal
#endif

#define DEV static __device__ __forceinline__

// The per-type constants are read-only for the lifetime of a launch.  Reading them through the constant address space
// lets the compiler fetch them with scalar loads into SGPRs (a generic pointer cannot be proven unclobbered once the
// kernel has stored to HBM, and the table would come in through vector loads into ~160 VGPRs).
typedef const __attribute__((address_space(4))) TypeParams CParams;

// Column access: a wave-uniform 64-bit column base (scalar registers) plus ONE 32-bit per-lane byte offset, which is the
// `global_load v, v_off, s[base]` addressing form — no 64-bit VALU address arithmetic and no VGPR pair per access.
// (byte offsets are 32-bit: a swarm shard holds fewer than 2^28 UAVs)
#define MRS_COL(S, np, f) ((char*)(S) + (size_t)(f) * (size_t)(np) * sizeof(double))
#define MRS_AT(S, np, f, off8) (*(double*)(MRS_COL(S, np, f) + (off8)))

// The compiler re-associates the address above into one 64-bit VGPR address per column (36 VGPRs held across the kernel and a
// 64-bit vector add per column).  Buffer instructions take the column offset in an SGPR and ONE 32-bit per-lane offset
// for all columns: `buffer_load_dwordx2 v, v_off, s[rsrc], s_col offen`.  Their offsets are 32-bit, so this form serves
// swarms whose state array is below 4 GiB (5.7 M UAVs); larger ones use the generic form (BUF = false).
typedef unsigned int mrs_v2u __attribute__((ext_vector_type(2)));
// Cache policy of the state accesses (buffer instruction aux bits on gfx950: 1 = sc0, 2 = nt, 16 = sc1).  NT kernels mark
// loads and stores non-temporal: the L2s then hold no dirty state lines when the kernel ends, and the next launch does not wait
// for their write-back.  That pays while the whole state sits in the 256 MB Infinity Cache anyway and a launch is short
// (model-only step, <= 121 k UAVs: 8.2-8.5 -> 7.4-7.7 us per step at 100 k, 6.56 -> 6.00 us at 50 k, 8.84 -> 8.32 at 120 k) and costs once the L2s'
// own hits matter (131 k: 8.5 -> 9.35 us, 200 k: 13.9 -> 14.4 us, 1 M: 63 -> 72 us; position cascade: a gain up to 56 k UAVs, 10.4 -> 10.0 us,
// a loss from 62 k on, at 100 k 14.3 -> 16.1 us — the cascade variant is launched up to 900 blocks) — tools/tune_step.py
// aux_<load>_<store> variants, which override the policy of the plain kernels through these macros:
#ifndef MRS_LD_AUX
#define MRS_LD_AUX 0
#endif
#ifndef MRS_ST_AUX
#define MRS_ST_AUX 0
#endif
#ifndef MRS_NT_LD_AUX  // what "non-temporal" means for loads / stores of the *_nt kernels (2 = nt)
#define MRS_NT_LD_AUX 2
#endif
#ifndef MRS_NT_ST_AUX
#define MRS_NT_ST_AUX 2
#endif
template <bool BUF, bool NT = false>
struct SwarmAcc : SwarmDev {
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned               np8;
  __device__ __forceinline__ explicit SwarmAcc(const SwarmDev& s) : SwarmDev(s) {
    np8 = (unsigned)s.npad * 8u;
    if (BUF) rsrc = __builtin_amdgcn_make_buffer_rsrc(s.S, 0, (int)((unsigned)F_COUNT * np8), 0x00020000);
  }
  __device__ __forceinline__ double ld(int f, unsigned off8) const {
    if (BUF) {
      const mrs_v2u t = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off8, (unsigned)f * np8, NT ? MRS_NT_LD_AUX : MRS_LD_AUX);
      return __builtin_bit_cast(double, t);
    }
    return MRS_AT(S, npad, f, off8);
  }
  __device__ __forceinline__ void st(int f, unsigned off8, double v) const {
    if (BUF)
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(mrs_v2u, v), rsrc, off8, (unsigned)f * np8, NT ? MRS_NT_ST_AUX : MRS_ST_AUX);
    else
      MRS_AT(S, npad, f, off8) = v;
  }
};

// Ablation aids for tools/variant_bench.sh ("-DMRS_ABL=<bits>"; timing experiments only — results are WRONG with any bit set):
// 1 no position-record store, 2 no collision evaluation / partner prefetch, 4 no stall check / progress word, 8 no skin test,
// 16 no list / record loads in the prologue
#ifndef MRS_ABL
#define MRS_ABL 0
#endif
#ifndef MRS_WAVES_PER_SIMD
#define MRS_WAVES_PER_SIMD 2  // register budget 256/lane: two resident waves per SIMD hide each other's FP64 latencies
#endif

namespace {

enum {
  M_UNKNOWN = 0, M_ACTUATOR, M_CONTROL_GROUP, M_ATTITUDE_RATE, M_ATTITUDE, M_TILT_HDG_RATE,
  M_ACC_HDG_RATE, M_ACC_HDG, M_VEL_HDG_RATE, M_VEL_HDG, M_POSITION
};
enum { FF_VEL_HDG_RATE = 0, FF_VEL_HDG, FF_ACC_HDG_RATE, FF_ACC_HDG };

DEV double sqnorm3(const double v[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }
DEV double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

#if MRS_FAST
// 1/sqrt(x): v_rsq_f64 (~5e-8 relative) + one third-order (Halley) step -> ~1 ulp; measured in tools/rsq_precision.hip.
// Four dependent FP64 ops instead of the ~25 of IEEE sqrt followed by IEEE divide (each dependent op costs ~36 cycles
// on gfx950, tools/fp64_rate.hip), and it is on the critical path of every RK4 stage three times.
DEV double rsqrt_h(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  const double e = __builtin_fma(-x * y, y, 1.0);
  const double p = __builtin_fma(0.375, e, 0.5);
  return __builtin_fma(y * e, p, y);
}
// 1/x: v_rcp_f64 + one third-order step
DEV double rcp_h(double x) {
  const double y = __builtin_amdgcn_rcp(x);
  const double e = __builtin_fma(-x, y, 1.0);
  return __builtin_fma(y, __builtin_fma(e, e, e), y);
}
#endif

// Eigen normalize(): z = squaredNorm(); if (z > 0) v /= sqrt(z)
DEV void normalize3(double v[3]) {
  double z = sqnorm3(v);
#if MRS_FAST
  if (z > 0) {
    const double r = rsqrt_h(z);
    v[0] *= r; v[1] *= r; v[2] *= r;
  }
  return;
#endif
  if (z > 0) {
    double n = sqrt(z);
    v[0] /= n; v[1] /= n; v[2] /= n;
  }
}

DEV void cross3(const double a[3], const double b[3], double o[3]) {
  double t0 = a[1] * b[2] - a[2] * b[1];
  double t1 = a[2] * b[0] - a[0] * b[2];
  double t2 = a[0] * b[1] - a[1] * b[0];
  o[0] = t0; o[1] = t1; o[2] = t2;
}

// R * inverse(matrixL(LLT(R^T R)))  — multirotor_model.hpp:249-253 / :314-316.  R row-major.
// Cholesky as Eigen's llt_inplace<Lower>::unblocked (a pivot x <= 0 stops the factorisation and the
// remaining entries stay those of R^T R); inverse as Eigen's 3x3 cofactor formula restricted to the
// non-zero entries of the lower-triangular factor.
DEV void reorth(const double R[9], double o[9]) {
  double a00 = (R[0] * R[0] + R[3] * R[3]) + R[6] * R[6];
  double a10 = (R[1] * R[0] + R[4] * R[3]) + R[7] * R[6];
  double a11 = (R[1] * R[1] + R[4] * R[4]) + R[7] * R[7];
  double a20 = (R[2] * R[0] + R[5] * R[3]) + R[8] * R[6];
  double a21 = (R[2] * R[1] + R[5] * R[4]) + R[8] * R[7];
  double a22 = (R[2] * R[2] + R[5] * R[5]) + R[8] * R[8];
#if MRS_FAST
  // L = [[a,0,0],[b,c,0],[d,e,f]];  L^-1 = [[1/a,0,0],[-b/(ac),1/c,0],[(be/c - d)/(af),-e/(cf),1/f]].
  // The pivots come from the leading minors d0 = a00, d1 = a00 a11 - a10^2, d2 = det(A):
  //   a = sqrt(d0), c = sqrt(d1/d0), f = sqrt(d2/d1)  =>  1/a = r0, 1/c = (d0 r0) r1, 1/f = (d1 r1) r2  with ri = rsqrt(di),
  // so the three rsqrt chains run in parallel instead of one after the other (the sequential form has ~27 dependent FP64
  // ops per RK stage, this one ~20).  R^T R is within O(dt) of the identity, so the minors carry no cancellation.
  // A non-positive minor (singular R) gives NaN here, which the NaN guards of the RHS / step absorb.
  const double m01 = a10 * a22 - a21 * a20;  // cofactor terms of det(A) along the first row
  const double m02 = a10 * a21 - a11 * a20;
  const double m00 = a11 * a22 - a21 * a21;
  const double d1  = a00 * a11 - a10 * a10;
  const double d2  = (a00 * m00 - a10 * m01) + a20 * m02;
  const double r0 = rsqrt_h(a00), r1 = rsqrt_h(d1), r2 = rsqrt_h(d2);
  const double ra = r0;
  const double rc = (a00 * r0) * r1;
  const double rf = (d1 * r1) * r2;
  const double b = a10 * ra, d = a20 * ra;
  const double e = (a21 - d * b) * rc;
  const double i00 = ra, i11 = rc, i22 = rf;
  const double erc = e * rc;
  const double i10 = -(b * ra) * rc;
  const double i21 = -erc * rf;
  const double i20 = ((b * erc - d) * ra) * rf;
#else
  double a, b, c, d, e, f;  // P = [[a,0,0],[b,c,0],[d,e,f]]
  const bool ok0 = !(a00 <= 0);
  a = ok0 ? sqrt(a00) : a00;
  b = ok0 ? a10 / a : a10;
  d = ok0 ? a20 / a : a20;
  const double x1  = a11 - b * b;
  const bool   ok1 = ok0 && !(x1 <= 0);
  c = ok1 ? sqrt(x1) : a11;
  e = ok1 ? (a21 - d * b) / c : a21;
  const double x2  = a22 - (d * d + e * e);
  const bool   ok2 = ok1 && !(x2 <= 0);
  f = ok2 ? sqrt(x2) : a22;
  const double cf     = c * f;
  const double det    = cf * a;
  const double invdet = 1.0 / det;
  const double i00 = cf * invdet;
  const double i10 = (-(b * f)) * invdet;
  const double i11 = (f * a) * invdet;
  const double i20 = (b * e - c * d) * invdet;
  const double i21 = (-(e * a)) * invdet;
  const double i22 = (a * c) * invdet;
#endif
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double r0 = R[3 * i], r1 = R[3 * i + 1], r2 = R[3 * i + 2];
    o[3 * i + 0] = (r0 * i00 + r1 * i10) + r2 * i20;
    o[3 * i + 1] = r1 * i11 + r2 * i21;
    o[3 * i + 2] = r2 * i22;
  }
}

// PIDController::update — controllers/pid.hpp:67-96
DEV double pid_update(double kp, double kd, double ki, double sat, double aw, double& last_error, double& integral,
                      double error, double dt, double inv_dt) {
#if MRS_FAST
  double difference = (error - last_error) * inv_dt;
#else
  (void)inv_dt;
  double difference = (error - last_error) / dt;
#endif
  last_error = error;
  double p   = kp * error;
  double d   = kd * difference;
  double i   = ki * integral;
  double sum = (p + d) + i;
  if (sat > 0) {
    if (sum >= sat) {
      sum = sat;
    } else if (sum <= -sat) {
      sum = -sat;
    }
  }
  if (aw > 0) {
    if (fabs(sum) < aw) integral += error * dt;
  }
  return sum;
}

// Eigen's SSE2 redux order for VectorXd::sum() (n uniform per wave) — used by .mean() in mixer.hpp:130 and
// multirotor_model.hpp:267
DEV double dyn_sum(const double v[MRS_MAXM], int n) {
  switch (n) {
    case 1: return v[0];
    case 2: return v[0] + v[1];
    case 3: return (v[0] + v[1]) + v[2];
    case 4: return (v[0] + v[2]) + (v[1] + v[3]);
    case 5: return ((v[0] + v[2]) + (v[1] + v[3])) + v[4];
    case 6: return ((v[0] + v[2]) + v[4]) + ((v[1] + v[3]) + v[5]);
    case 7: return (((v[0] + v[2]) + v[4]) + ((v[1] + v[3]) + v[5])) + v[6];
    default: return ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
  }
}

// Mixer::getControlSignal — controllers/mixer.hpp:107-144
// NM = compile-time motor count (0: read it from the type table — every `i < n` then stays a run-time predicate)
template <int NM, class PT>
DEV void mixer(PT& P, const double cg_in[4], double m[MRS_MAXM]) {
  const int n = NM ? NM : P.n_motors;
  double    cg[4] = {cg_in[0], cg_in[1], cg_in[2], cg_in[3]};
#pragma unroll
  for (int i = 0; i < MRS_MAXM; i++) {
    m[i] = 0.0;
    if (i < n)
      m[i] = ((P.alloc_inv[4 * i] * cg[0] + P.alloc_inv[4 * i + 1] * cg[1]) + P.alloc_inv[4 * i + 2] * cg[2]) +
             P.alloc_inv[4 * i + 3] * cg[3];
  }
  if (P.desaturation) {
    double mn = m[0];
#pragma unroll
    for (int i = 1; i < MRS_MAXM; i++)
      if (i < n && m[i] < mn) mn = m[i];
    if (mn < 0.0) {
      const double amn = fabs(mn);
#pragma unroll
      for (int i = 0; i < MRS_MAXM; i++)
        if (i < n) m[i] += amn;
    }
    double mx = m[0];
#pragma unroll
    for (int i = 1; i < MRS_MAXM; i++)
      if (i < n && m[i] > mx) mx = m[i];
    if (mx > 1.0) {
      if (cg_in[3] > 1e-2) {
        const double mean = dyn_sum(m, n) / (double)n;
        const double q    = mean / cg_in[3];
        cg[0] = cg[0] / q;
        cg[1] = cg[1] / q;
        cg[2] = cg[2] / q;
#pragma unroll
        for (int i = 0; i < MRS_MAXM; i++)
          if (i < n)
            m[i] = ((P.alloc_inv[4 * i] * cg[0] + P.alloc_inv[4 * i + 1] * cg[1]) + P.alloc_inv[4 * i + 2] * cg[2]) +
                   P.alloc_inv[4 * i + 3] * cg[3];
      } else {
#pragma unroll
        for (int i = 0; i < MRS_MAXM; i++)
          if (i < n) m[i] /= mx;
      }
    }
  }
}

// orientation error -> three attitude PIDs — attitude_controller.hpp:81-97 / :117-133.  pid = {le,in} x 3
template <class PT>
DEV void attitude_error_pids(PT& P, const double R[9], const double Rd[9], double pid[6], double dt,
                             double inv_dt, double rate[3]) {
  // A = Rd^T R, B = R^T Rd; only the six off-diagonal entries are needed
#define A_(i, j) ((Rd[0 + i] * R[0 + j] + Rd[3 + i] * R[3 + j]) + Rd[6 + i] * R[6 + j])
#define B_(i, j) ((R[0 + i] * Rd[0 + j] + R[3 + i] * Rd[3 + j]) + R[6 + i] * Rd[6 + j])
#define E_(i, j) (0.5 * (A_(i, j) - B_(i, j)))
  const double e0 = (E_(1, 2) - E_(2, 1)) / 2.0;
  const double e1 = (E_(2, 0) - E_(0, 2)) / 2.0;
  const double e2 = (E_(0, 1) - E_(1, 0)) / 2.0;
#undef A_
#undef B_
#undef E_
  rate[0] = pid_update(P.att_kp, P.att_kd, P.att_ki, P.att_sat_rp, 0.1, pid[0], pid[1], e0, dt, inv_dt);
  rate[1] = pid_update(P.att_kp, P.att_kd, P.att_ki, P.att_sat_rp, 0.1, pid[2], pid[3], e1, dt, inv_dt);
  rate[2] = pid_update(P.att_kp, P.att_kd, P.att_ki, P.att_sat_yaw, 0.1, pid[4], pid[5], e2, dt, inv_dt);
}

// ODE right-hand side — MultirotorModel::operator(), multirotor_model.hpp:301-366.
// y/k component order here: x(3) v(3) R row-major(9) omega(3); RK4 is component-wise so the order is free.
struct StepConst {
  double tt0, tt1, tt2, thrust;  // allocation * rpm^2 (stage-invariant, :332-335)
  double fm[3];                  // external_force / mass
};

// Re-reading the handful of per-type constants a stage needs through the scalar cache is cheaper than keeping them in
// SGPRs across the whole kernel, where they get spilled to VGPR lanes and cost v_readlane (vector) instructions.
// Passing the (wave-uniform) table pointer through an empty asm makes every stage's reads independent loads.
DEV CParams& fresh(CParams& P) {
  CParams* q = &P;
  asm volatile("" : "+s"(q));
  return *q;
}
DEV const TypeParams& fresh(const TypeParams& P) { return P; }
// The same for the collision view of the *_coll kernels: it is read through the kernel-argument segment (constant address space)
// at the three places that use it — prologue, evaluation, epilogue — instead of living in ~30 scalar registers across the whole
// kernel, where the allocator had to spill (620 v_readlane / v_writelane in the cascade kernel, 12 without).
typedef const __attribute__((address_space(4))) CollDev CCollDev;
DEV CCollDev& fresh(CCollDev& c) {
  CCollDev* q = &c;
  asm volatile("" : "+s"(q));
  return *q;
}
DEV const CollDev& fresh(const CollDev& c) { return c; }
struct CollKernArgs {  // layout of the *_coll kernels' argument segment
  SwarmDev sw;
  double   dt, inv_dt;
  CollDev  cd;
};

// position record of UAV i, written through (sc1): a launch running beside this one may read it as soon as the block's epoch word says so
typedef unsigned int mrs_v4u __attribute__((ext_vector_type(4)));
DEV void store_pos_sc1(Pos4* base, int n, int i, const Pos4& pp) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)((unsigned)n * 32u), 0x00020000);
  mrs_v4u a, b;
  const mrs_v2u x = __builtin_bit_cast(mrs_v2u, pp.x), y = __builtin_bit_cast(mrs_v2u, pp.y), z = __builtin_bit_cast(mrs_v2u, pp.z),
                w = __builtin_bit_cast(mrs_v2u, pp.w);
  a.x = x.x; a.y = x.y; a.z = y.x; a.w = y.y;
  b.x = z.x; b.y = z.y; b.z = w.x; b.w = w.y;
  __builtin_amdgcn_raw_buffer_store_b128(a, r, (unsigned)i * 32u, 0, 16);
  __builtin_amdgcn_raw_buffer_store_b128(b, r, (unsigned)i * 32u + 16u, 0, 16);
}
// The stall / warning index a sharded rank knows of lives IN the header of its export block (MRS_HDR_*): whatever a lane reports
// is what the next collective carries, with no copy in between; one GPU: the control words.
// SHARD (here and in step_kernel_body): the kernel serves sharded swarms.  The *_coll kernels of ONE GPU are compiled without all of
// it (the extra words, branches and scalar loads cost the 50 k collision tick 1.1 us when they were only skipped at run time).
template <bool SHARD, class CD>
DEV uint32_t* stall_word_of(CD& cd) { return (SHARD && cd.world > 1) ? (uint32_t*)cd.send + MRS_HDR_STALL : &cd.ctl[CTL_STALL]; }
template <bool SHARD, class CD>
DEV uint32_t* warn_word_of(CD& cd) { return (SHARD && cd.world > 1) ? (uint32_t*)cd.send + MRS_HDR_WARN : &cd.ctl[CTL_WARN]; }
// ONE lane reports "the lists are not good for evaluating a tick on state T" (T = this launch: a UAV HAS left its skin — exact;
// T = this launch + horizon: it may by then — announced).  One GPU: the word and its host mirror.  Sharded: the word keeps the
// smallest T (it travels with the next collective).  In a split tick an exact report that nobody announced means the
// displacement bound was violated: the error word says so.
template <bool SHARD, class CD>
DEV void report_stall(CD& cd, int part, uint32_t T, bool exact) {
  if (SHARD && cd.world > 1) {
    if (exact && part != MRS_PART_FULL) {
      const uint32_t known = word_load(stall_word_of<SHARD>(cd));
      if (known == 0u || known > T) raise_error(&cd.ctl[CTL_ERROR], (uint32_t*)cd.send + MRS_HDR_ERROR, 2u);
    }
    word_min_nz(stall_word_of<SHARD>(cd), T);
    // (every exact reporter of a full launch stores the same value; announced ones reach the host through the next launch's first block)
    if (exact && part == MRS_PART_FULL) __hip_atomic_store(&cd.hostw[CTL_STALL], T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  } else {
    cd.ctl[CTL_STALL] = T;
    __hip_atomic_store(&cd.hostw[CTL_STALL], T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
template <bool SHARD, class CD>
DEV void report_warning(CD& cd, int part, uint32_t W) {
  if (SHARD && cd.world > 1) {
    word_min_nz(warn_word_of<SHARD>(cd), W);  // sharded: the warning travels in the header of the next all-gather
  } else if (cd.ctl[CTL_WARN] != W) {
    cd.ctl[CTL_WARN] = W;
    __hip_atomic_store(&cd.hostw[CTL_WARN], W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

template <bool GUARD, class PT>
DEV void model_rhs(PT& P0, const StepConst& sc, const double y[18], double k[18]) {
  PT& P = fresh(P0);
  const double* v = &y[3];
  const double* w = &y[15];
  double Rh[9];
  reorth(&y[6], Rh);

  k[0] = v[0]; k[1] = v[1]; k[2] = v[2];
#if MRS_FAST
  {
    // drag: resistance * vnorm / mass = (resist_k/mass) * |v| * v   (|v| = sq * rsqrt(sq))
    const double sq = sqnorm3(v);
    const double vn = (sq > 0) ? sq * rsqrt_h(sq) : sq;  // sq is +0 or NaN here, and sqrt() of either is the value itself
    const double dk = (P.resist_k * P.inv_mass) * vn;
    const double tm = sc.thrust * P.inv_mass;
    k[3] = (tm * Rh[2] + sc.fm[0]) - dk * v[0];
    k[4] = (tm * Rh[5] + sc.fm[1]) - dk * v[1];
    k[5] = ((tm * Rh[8] - P.g) + sc.fm[2]) - dk * v[2];
  }
#else
  {
    const double sq = sqnorm3(v);
    const double vn = sqrt(sq);
    const double resistance = (P.resist_k * vn) * vn;
    double vnorm[3] = {v[0], v[1], v[2]};
    if (vn != 0) {  // :340-342 (normalize() re-checks squaredNorm() > 0)
      if (sq > 0) {
        vnorm[0] /= vn; vnorm[1] /= vn; vnorm[2] /= vn;
      }
    }
    k[3] = ((-0.0 + (sc.thrust * Rh[2]) / P.mass) + sc.fm[0]) - (resistance * vnorm[0]) / P.mass;
    k[4] = ((-0.0 + (sc.thrust * Rh[5]) / P.mass) + sc.fm[1]) - (resistance * vnorm[1]) / P.mass;
    k[5] = ((-P.g + (sc.thrust * Rh[8]) / P.mass) + sc.fm[2]) - (resistance * vnorm[2]) / P.mass;
  }
#endif
  // R_dot = Rh * omega_tensor (:323-330,:348); zero entries of the tensor skipped
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double r0 = Rh[3 * i], r1 = Rh[3 * i + 1], r2 = Rh[3 * i + 2];
    k[6 + 3 * i + 0] = r1 * w[2] + r2 * (-w[1]);
    k[6 + 3 * i + 1] = r0 * (-w[2]) + r2 * w[0];
    k[6 + 3 * i + 2] = r0 * w[1] + r1 * (-w[0]);
  }
  // omega_dot = J^-1 (tau - omega x (J omega) + M_ext),  M_ext == 0 through UavSystem (:350)
  double Jw[3], c[3], rhs3[3];
#pragma unroll
  for (int i = 0; i < 3; i++) Jw[i] = (P.J[3 * i] * w[0] + P.J[3 * i + 1] * w[1]) + P.J[3 * i + 2] * w[2];
  cross3(w, Jw, c);
  rhs3[0] = sc.tt0 - c[0];
  rhs3[1] = sc.tt1 - c[1];
  rhs3[2] = sc.tt2 - c[2];
#pragma unroll
  for (int i = 0; i < 3; i++)
    k[15 + i] = (P.Jinv[3 * i] * rhs3[0] + P.Jinv[3 * i + 1] * rhs3[1]) + P.Jinv[3 * i + 2] * rhs3[2];
  if (GUARD) {
#pragma unroll
    for (int i = 0; i < 18; i++)
      if (k[i] != k[i]) k[i] = 0;  // :361-365
  }
}

DEV bool not_finite(double x) { return !(fabs(x) <= 1.79769313486231570815e308); }

// one UavSystem::makeStep for the calling lane; state vectors live in registers across sub-steps
struct Lane {
  double y[18];        // x v R omega
  double vp[3];        // v_prev
  double imu[3];
  uint32_t flags;
  // issued with the state loads of the prologue (single-step kernels): the first four command and rpm columns — every input
  // mode reads at least the former, every airframe has at least four motors — and the external force
  double pre_cmd[4], pre_rpm[4], pre_fe[3];
  double xb[3];  // position at the last neighbour-list rebuild (skin test at the end of the step), also fetched up front
  // *_coll kernels: the UAV's neighbour list (length, first entry) and export slot, fetched with the state
  uint32_t ncnt, ne0, eslot;
  double   rc_mass, rc_arm, rc_prop;  // airframe constants in the UAV's record of the last search (what its partners use)
  bool     stale;                     // ... which no longer are the UAV's constants: the lists have to be rebuilt
  uint32_t ne[MRS_NPRE];                                           // the first list entries ...
  double   pox[MRS_NPRE], poy[MRS_NPRE], poz[MRS_NPRE], pow_[MRS_NPRE];  // ... and their position records (x, y, z, type), fetched ahead of the evaluation
  bool     fe_live;  // the external force of this step is held in pre_fe (latched column, or just evaluated from the lists)
  double   pid_pre[24];  // boundary kernels of a split sharded tick: the PID state, fetched with the state (see PIDPRE)
};

// Phase 1 of UavSystem::makeStep for one UAV: controller cascade (uav_system.hpp:314-373) -> actuator throttles ->
// MultirotorModel::setInput (multirotor_model.hpp:392-410) -> motor low-pass, allocation*rpm^2, F_ext/m.
// Reads the start-of-step state in L; writes PID columns and the new motor rpm straight back to HBM.
// The part of control_and_motors that depends on the motor count: ACTUATOR_CMD payload or mixer -> throttles ->
// MultirotorModel::setInput -> motor low-pass, allocation*rpm^2, F_ext/m.  NM > 0 fixes the count at compile time (no
// predicated work on absent motors, and only the used columns of the allocation table are fetched).
// CARRY (the fused plain step kernels): the new rpm of the first four motors stays in L.pre_rpm for the next step of the launch
// instead of going to HBM; the launch's epilogue stores it.
template <int NM, bool PRE, bool CARRY, class SW, class PT>
DEV void motors_stage(const SW& sw, PT& P0, const int i, Lane& L, const int src, const double (&cg)[4], StepConst& sc, double& mean_in) {
  PT&       P    = fresh(P0);
  const int n    = NM ? NM : P.n_motors;
  const unsigned off8 = (unsigned)i * 8u;
#define LD(f) sw.ld(f, off8)
#define ST(f, val) sw.st(f, off8, val)
  double motors[MRS_MAXM];
#pragma unroll
  for (int m = 0; m < MRS_MAXM; m++) motors[m] = 0.0;
  if (src == 1) {
#pragma unroll
    for (int m = 0; m < MRS_MAXM; m++)
      if (m < n) motors[m] = (PRE && m < 4) ? L.pre_cmd[m < 4 ? m : 0] : LD(F_CMD + m);
  } else if (src == 2) {
    mixer<NM>(P, cg, motors);
  }

  // ---- MultirotorModel::setInput, multirotor_model.hpp:392-410 ----
  // The motor low-pass of step() (:244-246) only needs the old rpm and this input, and the ODE only needs the old
  // rpm through allocation*rpm^2, so both are finished here and the new rpm goes straight back to HBM: nothing of
  // the motor state stays live across the RK4 stages.  mean(input) is kept for the take-off patch (:267).
  {
    double input[MRS_MAXM], rsq[MRS_MAXM];
#pragma unroll
    for (int m = 0; m < MRS_MAXM; m++) {
      double val = motors[m];
      if (not_finite(val)) val = 0;
#if MRS_FAST
      val = fmin(fmax(val, 0.0), 1.0);  // two instructions instead of two branches (the sign of a zero may differ)
#else
      if (val < 0.0) {
        val = 0.0;
      } else if (val > 1.0) {
        val = 1.0;
      }
#endif
      input[m] = P.min_rpm + (P.max_rpm - P.min_rpm) * val;
      rsq[m]   = 0.0;
      if (m < n) {
        const double rpm = (PRE && m < 4) ? L.pre_rpm[m < 4 ? m : 0] : LD(F_RPM + m);
        rsq[m]           = rpm * rpm;                                  // :332
        if (CARRY && PRE && m < 4)
          L.pre_rpm[m < 4 ? m : 0] = P.filt_c * rpm + P.filt_1mc * input[m];
        else
          ST(F_RPM + m, P.filt_c * rpm + P.filt_1mc * input[m]);       // :246
      }
    }
    mean_in = dyn_sum(input, n) / (double)n;
    double tt[4];  // allocation_matrix * rpm^2, :334
#pragma unroll
    for (int r = 0; r < 4; r++) {
      double s = P.alloc[r * MRS_MAXM] * rsq[0];
#pragma unroll
      for (int m = 1; m < MRS_MAXM; m++)
        if (m < n) s += P.alloc[r * MRS_MAXM + m] * rsq[m];
      tt[r] = s;
    }
    sc.tt0 = tt[0]; sc.tt1 = tt[1]; sc.tt2 = tt[2]; sc.thrust = tt[3];
    double fe[3] = {0.0, 0.0, 0.0};
    if (PRE ? L.fe_live : (sw.opts & 1u) != 0u) {  // wave-uniform: nobody ever applied a force to this swarm -> the columns are all zero
      if (PRE) {
        fe[0] = L.pre_fe[0]; fe[1] = L.pre_fe[1]; fe[2] = L.pre_fe[2];
      } else {
        fe[0] = LD(F_FEXT + 0); fe[1] = LD(F_FEXT + 1); fe[2] = LD(F_FEXT + 2);
      }
    }
#if MRS_FAST
    sc.fm[0] = fe[0] * P.inv_mass; sc.fm[1] = fe[1] * P.inv_mass; sc.fm[2] = fe[2] * P.inv_mass;
#else
    sc.fm[0] = fe[0] / P.mass; sc.fm[1] = fe[1] / P.mass; sc.fm[2] = fe[2] / P.mass;
#endif
  }
#undef LD
#undef ST
}

// ---- the controllers of the cascade, one device function each (uav_system.hpp:314-373 chains them; the component probe kernel at
//      the end of this file runs them one at a time) ----

// PositionController::getControlSignal — position_controller.hpp:73-86.  pid = {last_error, integral} x {x, y, z}
template <class PT>
DEV void position_controller(PT& P, const double x[3], const double ref[3], double pid[6], double dt, double inv_dt, double out[3]) {
  const double e0 = ref[0] - x[0], e1 = ref[1] - x[1], e2 = ref[2] - x[2];
  out[0] = pid_update(P.pos_kp, P.pos_kd, P.pos_ki, P.pos_sat, 1.0, pid[0], pid[1], e0, dt, inv_dt);
  out[1] = pid_update(P.pos_kp, P.pos_kd, P.pos_ki, P.pos_sat, 1.0, pid[2], pid[3], e1, dt, inv_dt);
  out[2] = pid_update(P.pos_kp, P.pos_kd, P.pos_ki, P.pos_sat, 1.0, pid[4], pid[5], e2, dt, inv_dt);
}

// VelocityController::getControlSignal (both overloads share the PIDs) — velocity_controller.hpp:68-102
template <class PT>
DEV void velocity_controller(PT& P, const double v[3], const double ref[3], double pid[6], double dt, double inv_dt, double out[3]) {
  const double e0 = ref[0] - v[0], e1 = ref[1] - v[1], e2 = ref[2] - v[2];
  out[0] = pid_update(P.vel_kp, P.vel_kd, P.vel_ki, P.vel_sat, 1.0, pid[0], pid[1], e0, dt, inv_dt);
  out[1] = pid_update(P.vel_kp, P.vel_kd, P.vel_ki, P.vel_sat, 1.0, pid[2], pid[3], e1, dt, inv_dt);
  out[2] = pid_update(P.vel_kp, P.vel_kd, P.vel_ki, P.vel_sat, 1.0, pid[4], pid[5], e2, dt, inv_dt);
}

// AccelerationController, the part both overloads share: desired force direction fdn and throttle — acceleration_controller.hpp:46-48,89-94
template <class PT>
DEV double acceleration_thrust(PT& P, const double R[9], const double acc[3], double fdn[3]) {
  double fd[3];
  fd[0] = (acc[0] + 0.0) * P.mass;
  fd[1] = (acc[1] + 0.0) * P.mass;
  fd[2] = (acc[2] + P.g) * P.mass;
  fdn[0] = fd[0]; fdn[1] = fd[1]; fdn[2] = fd[2];
  normalize3(fdn);
  const double col2[3]      = {R[2], R[5], R[8]};
  const double thrust_force = dot3(fd, col2);
#if MRS_FAST
  // sqrt(x) = x * rsqrt(x); x < 0 -> NaN (the reference's NaN-throttle path), x == 0 -> 0
  const double xq = thrust_force * P.inv_kf_n;
  const double sq = (xq == 0.0) ? 0.0 : xq * rsqrt_h(xq);
  return (sq - P.min_rpm) * P.inv_rpm_range;
#else
  return (sqrt(thrust_force / P.kf_n) - P.min_rpm) / (P.max_rpm - P.min_rpm);
#endif
}

// AccelerationController::getControlSignal(AccelerationHdg): desired attitude from fdn and the heading — acceleration_controller.hpp:50-87
DEV void acceleration_attitude(const double fdn[3], const double hdg, double Rd[9]) {
#if MRS_FAST
  double bx, by;
  sincos(hdg, &by, &bx);  // one argument reduction for both
#else
  const double bx = cos(hdg), by = sin(hdg);
#endif
  // A = first two columns of (I - fdn fdn^T); B^T A = its top 2x2 block (:58-71)
  const double A00 = 1.0 - fdn[0] * fdn[0], A01 = 0.0 - fdn[0] * fdn[1];
  const double A10 = 0.0 - fdn[1] * fdn[0], A11 = 1.0 - fdn[1] * fdn[1];
  const double A20 = 0.0 - fdn[2] * fdn[0], A21 = 0.0 - fdn[2] * fdn[1];
  double p00, p01, p10, p11;  // pseudo-inverse of B^T A (:72)
#if MRS_FAST
  {  // (M^T M)^-1 M^T == M^-1 for the 2x2 block
    const double rdet = 1.0 / (A00 * A11 - A01 * A10);
    p00 = A11 * rdet; p01 = -A01 * rdet; p10 = -A10 * rdet; p11 = A00 * rdet;
  }
#else
  {
    // M^T M, then Eigen's dynamic inverse(): partial-pivot LU + solve against the identity
    double l00 = A00 * A00 + A10 * A10, l01 = A00 * A01 + A10 * A11;
    double l10 = A01 * A00 + A11 * A10, l11 = A01 * A01 + A11 * A11;
    const bool swp = fabs(l10) > fabs(l00);
    if (swp) {
      double t = l00; l00 = l10; l10 = t;
      t = l01; l01 = l11; l11 = t;
    }
    l10 /= l00;
    l11 -= l10 * l01;
    // column 0 of the identity (after the row permutation), then column 1
    double b0 = swp ? 0.0 : 1.0, b1 = swp ? 1.0 : 0.0;
    b1 -= l10 * b0; b1 /= l11; b0 -= l01 * b1; b0 /= l00;
    const double n00 = b0, n10 = b1;
    b0 = swp ? 1.0 : 0.0; b1 = swp ? 0.0 : 1.0;
    b1 -= l10 * b0; b1 /= l11; b0 -= l01 * b1; b0 /= l00;
    const double n01 = b0, n11 = b1;
    p00 = n00 * A00 + n01 * A01; p01 = n00 * A10 + n01 * A11;
    p10 = n10 * A00 + n11 * A01; p11 = n10 * A10 + n11 * A11;
  }
#endif
  double c0[3], c1[3];
  c0[0] = ((A00 * p00 + A01 * p10) * bx + (A00 * p01 + A01 * p11) * by) + 0.0;
  c0[1] = ((A10 * p00 + A11 * p10) * bx + (A10 * p01 + A11 * p11) * by) + 0.0;
  c0[2] = ((A20 * p00 + A21 * p10) * bx + (A20 * p01 + A21 * p11) * by) + 0.0;
  normalize3(c0);
  cross3(fdn, c0, c1);
  normalize3(c1);
#pragma unroll
  for (int q = 0; q < 3; q++) {
    Rd[3 * q + 0] = c0[q]; Rd[3 * q + 1] = c1[q]; Rd[3 * q + 2] = fdn[q];
  }
}

// AttitudeController::getControlSignal(TiltHdgRate), first part: desired attitude from the tilt vector and the body x axis — attitude_controller.hpp:108-115
DEV void tilt_attitude(const double R[9], const double tilt[3], double Rd[9]) {
  double c2[3] = {tilt[0], tilt[1], tilt[2]}, c1[3], c0[3];
  const double Rc0[3] = {R[0], R[3], R[6]};
  normalize3(c2);
  cross3(c2, Rc0, c1);
  normalize3(c1);
  cross3(c1, c2, c0);
  normalize3(c0);
#pragma unroll
  for (int q = 0; q < 3; q++) {
    Rd[3 * q + 0] = c0[q]; Rd[3 * q + 1] = c1[q]; Rd[3 * q + 2] = c2[q];
  }
}

// ... last part: intrinsic yaw rate that gives the commanded heading rate — intrinsicBodyRateToHeadingRate :177-206 and
// getYawRateIntrinsic :212-251; the three std::cout warnings are counted in diag[0..2]
DEV double tilt_yaw_rate(unsigned long long* diag, const double R[9], const double rate[3], const double tilt_hr) {
  // only R_d(0,0), R_d(1,0) of R*W are used
  const double Rd00 = (R[0] * 0.0 + R[1] * rate[2]) + R[2] * (-rate[1]);
  const double Rd10 = (R[3] * 0.0 + R[4] * rate[2]) + R[5] * (-rate[1]);
  const double rx = R[0], ry = R[3];
  const double denom = rx * rx + ry * ry;
  double ax = 0, ay = 0;
  if (fabs(denom) <= 1e-5) {
    atomicAdd(&diag[0], 1ull);
  } else {
    ax = -ry / denom;
    ay = rx / denom;
  }
  const double parasitic = ax * Rd00 + ay * Rd10;
  const double hr = tilt_hr - parasitic;
  double yaw = 0;
  if (!(fabs(hr) < 1e-3)) {
    const double hv[3] = {R[0], R[3], 0.0};
    const double hrv[3] = {0.0, 0.0, hr}, ez[3] = {0.0, 0.0, 1.0};
    double ov[3], bo[3], pr[3];
    cross3(hrv, hv, ov);
    cross3(ez, hv, bo);
    normalize3(bo);
    const double col1[3] = {R[1], R[4], R[7]};
#pragma unroll
    for (int q = 0; q < 3; q++) pr[q] = ((bo[q] * bo[0]) * col1[0] + (bo[q] * bo[1]) * col1[1]) + (bo[q] * bo[2]) * col1[2];
    const double ovn = sqrt(sqnorm3(ov)), prn = sqrt(sqnorm3(pr));
    if (fabs(prn) < 1e-5) {
      atomicAdd(&diag[1], 1ull);
    } else {
      const double dd  = dot3(ov, pr);
      const int    dir = (0.0 < dd) - (dd < 0.0);
      const double out = dir * (ovn / prn);
      if (not_finite(out)) {
        atomicAdd(&diag[2], 1ull);
      } else {
        yaw = out;
      }
    }
  }
  return yaw;
}

// RateController::getControlSignal — rate_controller.hpp:67-81 (gains pre-multiplied by J(i,i), :56-65)
template <class PT>
DEV void rate_controller(PT& P, const double w[3], const double rate[3], const double throttle, double pid[6], double dt, double inv_dt, double cg[4]) {
  const double e0 = rate[0] - w[0], e1 = rate[1] - w[1], e2 = rate[2] - w[2];
  cg[0] = pid_update(P.rate_kp[0], P.rate_kd[0], P.rate_ki[0], -1.0, 1.0, pid[0], pid[1], e0, dt, inv_dt);
  cg[1] = pid_update(P.rate_kp[1], P.rate_kd[1], P.rate_ki[1], -1.0, 1.0, pid[2], pid[3], e1, dt, inv_dt);
  cg[2] = pid_update(P.rate_kp[2], P.rate_kd[2], P.rate_ki[2], -1.0, 1.0, pid[4], pid[5], e2, dt, inv_dt);
  cg[3] = throttle;
}

// The cascade and the motor stage are two calls: the fused collision evaluation sits between them (the force is not needed earlier,
// and the loads it waits for have the whole cascade to arrive).
// src: where the actuator throttles come from: 0 zeros (crashed / no input yet), 1 ACTUATOR_CMD payload, 2 mixer (control group cg)
// PIDPRE: the PID state comes from L.pid_pre (the prologue fetched all 24 columns with the state) instead of being loaded where
// each controller needs it.  The big launches load at the point of use — staggered loads beat one burst while two waves interleave
// on a SIMD —, but a boundary launch of a split sharded tick is a few waves whose duration IS one wave's dependent chain, with the
// interior launch streaming beside it: four exposed round trips of 2-3 us each.
template <bool CASCADE, bool PRE, bool PIDPRE = false, class SW, class PT>
DEV void control_cascade(const SW& sw, PT& P, const int i, const Lane& L, const double dt, const double inv_dt, int& src, double (&cg)[4]) {
#ifdef MRS_ASSUME_POSITION  // measurement only (tools/build_variants.sh stepflag -DMRS_ASSUME_POSITION=1): every UAV follows a position reference
  const int mode = (L.flags & FLAG_CRASHED) ? M_UNKNOWN : M_POSITION;
#else
  const int mode = (L.flags & FLAG_MODE_MASK) >> FLAG_MODE_SHIFT;
#endif
  src   = 0;
  cg[0] = cg[1] = cg[2] = cg[3] = 0.0;
  const unsigned off8 = (unsigned)i * 8u;
#define LD(f) sw.ld(f, off8)
#define ST(f, val) sw.st(f, off8, val)
#define CMD4(q) (PRE ? L.pre_cmd[q] : LD(F_CMD + (q)))

  const double* x = &L.y[0];
  const double* v = &L.y[3];
  const double* R = &L.y[6];
  const double* w = &L.y[15];

  if ((L.flags & FLAG_CRASHED) || mode == M_UNKNOWN) {
    // uav_system.hpp:308-310: actuators = 0
  } else if (mode == M_ACTUATOR) {
    src = 1;
  } else if (CASCADE) {
    // ---- controller cascade, uav_system.hpp:314-373 ----
    int    active = mode;
    double vec[3] = {0, 0, 0}, hdg = 0;          // velocity / acceleration reference + heading or heading rate
    double Rd[9]  = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // attitude reference
    double throttle = 0, tilt[3] = {0, 0, 0}, tilt_hr = 0;
    double rate[3] = {0, 0, 0};
    const uint32_t ff = (L.flags & FLAG_FF_MASK) >> FLAG_FF_SHIFT;

    if (mode == M_CONTROL_GROUP) {
      cg[0] = CMD4(0); cg[1] = CMD4(1); cg[2] = CMD4(2); cg[3] = CMD4(3);
    } else if (mode == M_ATTITUDE_RATE) {
      rate[0] = CMD4(0); rate[1] = CMD4(1); rate[2] = CMD4(2); throttle = CMD4(3);
    } else if (mode == M_ATTITUDE) {
#pragma unroll
      for (int q = 0; q < 9; q++) Rd[q] = LD(F_CMD + q);
      throttle = LD(F_CMD + 9);
    } else if (mode == M_TILT_HDG_RATE) {
      tilt[0] = CMD4(0); tilt[1] = CMD4(1); tilt[2] = CMD4(2);
      tilt_hr = CMD4(3); throttle = LD(F_CMD + 4);
    } else {
      vec[0] = CMD4(0); vec[1] = CMD4(1); vec[2] = CMD4(2); hdg = CMD4(3);
    }

    if (active == M_POSITION) {
      double pid[6];
#pragma unroll
      for (int q = 0; q < 6; q++) pid[q] = PIDPRE ? L.pid_pre[0 + q] : LD(F_PID + 0 + q);
      const double ref[3] = {vec[0], vec[1], vec[2]};
      position_controller(P, x, ref, pid, dt, inv_dt, vec);
#pragma unroll
      for (int q = 0; q < 6; q++) ST(F_PID + 0 + q, pid[q]);
      active = M_VEL_HDG;
      if (ff & (1u << FF_VEL_HDG)) {  // uav_system.hpp:318-322
        vec[0] += LD(F_FF + 4 * FF_VEL_HDG + 0); vec[1] += LD(F_FF + 4 * FF_VEL_HDG + 1); vec[2] += LD(F_FF + 4 * FF_VEL_HDG + 2);
      } else if (ff & (1u << FF_VEL_HDG_RATE)) {
        vec[0] += LD(F_FF + 4 * FF_VEL_HDG_RATE + 0); vec[1] += LD(F_FF + 4 * FF_VEL_HDG_RATE + 1); vec[2] += LD(F_FF + 4 * FF_VEL_HDG_RATE + 2);
      }
    }
    if (active == M_VEL_HDG || active == M_VEL_HDG_RATE) {
      double pid[6];
#pragma unroll
      for (int q = 0; q < 6; q++) pid[q] = PIDPRE ? L.pid_pre[6 + q] : LD(F_PID + 6 + q);
      const double ref[3] = {vec[0], vec[1], vec[2]};
      velocity_controller(P, v, ref, pid, dt, inv_dt, vec);
#pragma unroll
      for (int q = 0; q < 6; q++) ST(F_PID + 6 + q, pid[q]);
      if (active == M_VEL_HDG) {
        active = M_ACC_HDG;
        if (ff & (1u << FF_ACC_HDG)) {  // uav_system.hpp:330-334
          vec[0] += LD(F_FF + 4 * FF_ACC_HDG + 0); vec[1] += LD(F_FF + 4 * FF_ACC_HDG + 1); vec[2] += LD(F_FF + 4 * FF_ACC_HDG + 2);
        } else if (ff & (1u << FF_ACC_HDG_RATE)) {
          vec[0] += LD(F_FF + 4 * FF_ACC_HDG_RATE + 0); vec[1] += LD(F_FF + 4 * FF_ACC_HDG_RATE + 1); vec[2] += LD(F_FF + 4 * FF_ACC_HDG_RATE + 2);
        }
      } else {
        active = M_ACC_HDG_RATE;
        if (ff & (1u << FF_ACC_HDG_RATE)) {  // uav_system.hpp:341-346
          vec[0] += LD(F_FF + 4 * FF_ACC_HDG_RATE + 0); vec[1] += LD(F_FF + 4 * FF_ACC_HDG_RATE + 1); vec[2] += LD(F_FF + 4 * FF_ACC_HDG_RATE + 2);
          hdg += LD(F_FF + 4 * FF_ACC_HDG_RATE + 3);
        } else if (ff & (1u << FF_ACC_HDG)) {
          vec[0] += LD(F_FF + 4 * FF_ACC_HDG + 0); vec[1] += LD(F_FF + 4 * FF_ACC_HDG + 1); vec[2] += LD(F_FF + 4 * FF_ACC_HDG + 2);
        }
      }
    }
    if (active == M_ACC_HDG || active == M_ACC_HDG_RATE) {  // AccelerationController, acceleration_controller.hpp:44-122
      double fdn[3];
      throttle = acceleration_thrust(P, R, vec, fdn);
      if (active == M_ACC_HDG) {
        acceleration_attitude(fdn, hdg, Rd);
        active = M_ATTITUDE;
      } else {
        tilt[0] = fdn[0]; tilt[1] = fdn[1]; tilt[2] = fdn[2];
        tilt_hr = hdg;
        active  = M_TILT_HDG_RATE;
      }
    }
    if (active == M_ATTITUDE || active == M_TILT_HDG_RATE) {  // AttitudeController, attitude_controller.hpp:79-145
      double pid[6];
#pragma unroll
      for (int q = 0; q < 6; q++) pid[q] = PIDPRE ? L.pid_pre[12 + q] : LD(F_PID + 12 + q);
      if (active == M_TILT_HDG_RATE) tilt_attitude(R, tilt, Rd);
      attitude_error_pids(P, R, Rd, pid, dt, inv_dt, rate);
#pragma unroll
      for (int q = 0; q < 6; q++) ST(F_PID + 12 + q, pid[q]);
      if (active == M_TILT_HDG_RATE) rate[2] += tilt_yaw_rate(sw.diag, R, rate, tilt_hr);
      active = M_ATTITUDE_RATE;
    }
    if (active == M_ATTITUDE_RATE) {
      double pid[6];
#pragma unroll
      for (int q = 0; q < 6; q++) pid[q] = PIDPRE ? L.pid_pre[18 + q] : LD(F_PID + 18 + q);
      rate_controller(P, w, rate, throttle, pid, dt, inv_dt, cg);
#pragma unroll
      for (int q = 0; q < 6; q++) ST(F_PID + 18 + q, pid[q]);
      active = M_CONTROL_GROUP;
    }
    src = 2;
  }
#undef LD
#undef ST
#undef CMD4
  (void)x; (void)v; (void)R; (void)w; (void)dt; (void)inv_dt;
}

template <bool UNIFORM, bool PRE, bool CARRY = false, class SW, class PT>
DEV void motors_dispatch(const SW& sw, PT& P, const int i, Lane& L, const int src, const double (&cg)[4], StepConst& sc, double& mean_in,
                         const int n_block) {
  // the motor count is wave-uniform in single-type blocks: branch once into the code specialised for it
  if (UNIFORM) {
    const int n = n_block;  // from the block-type word the prologue already holds: no extra scalar load before the branch
    if (n == 4)
      motors_stage<4, PRE, CARRY>(sw, P, i, L, src, cg, sc, mean_in);
    else if (n == 6)
      motors_stage<6, PRE, CARRY>(sw, P, i, L, src, cg, sc, mean_in);
    else if (n == 8)
      motors_stage<8, PRE, CARRY>(sw, P, i, L, src, cg, sc, mean_in);
    else
      motors_stage<0, PRE, CARRY>(sw, P, i, L, src, cg, sc, mean_in);
  } else {
    motors_stage<0, PRE, CARRY>(sw, P, i, L, src, cg, sc, mean_in);
  }
}

// Phase 2: one classical RK4 step exactly as odeint's generic_rk_algorithm evaluates it (scale_sumN, left to right):
//   t2 = 1*y + (.5dt)k1;  t3 = 1*y + (0dt)k1 + (.5dt)k2;  t4 = 1*y + (0dt)k1 + (0dt)k2 + (1dt)k3
//   y' = 1*y + (dt/6)k1 + (dt/3)k2 + (dt/3)k3 + (dt/6)k4        (acc accumulates it left to right)
// for NU independent UAVs held by the same lane.  The four stages are one loop whose unroll factor is a tuning knob
// (k is iteration-local, live state = base, acc, t).  NU = 2 (two UAVs per lane for instruction-level parallelism) was measured 35 % SLOWER than NU = 1 at
// 100 k UAVs (422 registers, AGPR copies) and is not instantiated.
// The position rows are special: dx/dt = v does not feed back into the RHS, so no stage value is formed for them.
// The four stages; acc receives y'.  GUARD = the RHS's per-component NaN -> 0 (multirotor_model.hpp:361-365).
template <bool GUARD, int SU, int NU, class PT>
DEV void rk4_stages(PT& P, const StepConst (&sc)[NU], const Lane (&L)[NU], const double dt, double (&acc)[NU][18]) {
  const double a_half = (1.0 / 2.0) * dt, a_one = 1.0 * dt;
  const double b16 = (1.0 / 6.0) * dt, b13 = (1.0 / 3.0) * dt;
  double       t[NU][18];
#if !MRS_FAST
  uint32_t     poison[NU];  // components whose zero-weight terms are NaN (0 * non-finite)
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
#endif
#pragma unroll
  for (int u = 0; u < NU; u++) {
#if !MRS_FAST
    poison[u] = 0;
#endif
#pragma unroll
    for (int c = 0; c < 18; c++) {
      acc[u][c] = 1.0 * L[u].y[c];
      t[u][c]   = L[u].y[c];
    }
  }
// SU = unroll factor of the stage loop.  Measured (tools/variant_bench.sh): fully unrolled stages are 2-6 % faster while at most
// two waves per SIMD are resident (no loop-carried register copies, ~225 VGPRs); the rolled loop needs 160 VGPRs, which
// buys a third resident wave — worth +12 % once the swarm has more than two waves per SIMD (1 M UAVs: 86.6 -> 77.5 us).
#pragma unroll SU
  for (int stage = 0; stage < 4; stage++) {
    double k[NU][18];
#pragma unroll
    for (int u = 0; u < NU; u++) model_rhs<GUARD>(P, sc[u], t[u], k[u]);
    const double bw = (stage == 0 || stage == 3) ? b16 : b13;
    const double aw = (stage == 2) ? a_one : a_half;
#pragma unroll
    for (int u = 0; u < NU; u++) {
#pragma unroll
      for (int c = 0; c < 18; c++) {
        acc[u][c] = acc[u][c] + bw * k[u][c];
        if (c >= 3) {
          double base = 1.0 * L[u].y[c];
#if !MRS_FAST
          if (GUARD) {  // (without non-finite derivatives — the unguarded pass — there is nothing to poison)
            if (poison[u] & (1u << c)) base = qnan;
            if (stage < 2 && not_finite(k[u][c])) poison[u] |= 1u << c;
          }
#endif
          t[u][c] = base + aw * k[u][c];  // (unused after the last stage)
        }
      }
    }
  }
}

template <int NU>
DEV bool any_nan18(const double (&acc)[NU][18], const int u) {
  bool any_nan = false;
#pragma unroll
  for (int c = 0; c < 18; c++) any_nan |= (acc[u][c] != acc[u][c]);
  return any_nan;
}

template <int NU, int SU, class SW, class PT>
DEV void rk4_integrate(const SW& sw, PT& P, const StepConst (&sc)[NU], Lane (&L)[NU], const int (&idx)[NU], const double dt,
                       const double* backup) {
  double acc[NU][18];
  bool   bad[NU];
  // A non-finite derivative component always reaches y' (every stage weight is non-zero), so the per-component NaN guards of
  // the RHS — and LITERAL's bookkeeping for the reference's 0 * inf terms — only matter for steps whose unguarded result is
  // not finite.  The stages therefore run without them (-12 % vector instructions in FAST); a wave in which any lane ends up
  // with such a value repeats the step with everything in place — lanes without one get the identical result again, the
  // others get the reference's zeroed components.  (FAST has no 0 * inf terms: only a NaN triggers the repeat there.)
  rk4_stages<false, SU>(P, sc, L, dt, acc);
  bool redo = false;
#pragma unroll
  for (int u = 0; u < NU; u++) {
#if MRS_FAST
    redo |= any_nan18(acc, u);
#else
#pragma unroll
    for (int c = 0; c < 18; c++) redo |= not_finite(acc[u][c]);
#endif
  }
  if (__builtin_amdgcn_ballot_w64(redo) != 0ull) rk4_stages<true, SU>(P, sc, L, dt, acc);
#pragma unroll
  for (int u = 0; u < NU; u++) bad[u] = any_nan18(acc, u);
#pragma unroll
  for (int u = 0; u < NU; u++) {
#pragma unroll
    for (int c = 0; c < 18; c++) L[u].y[c] = acc[u][c];
    if (bad[u]) {  // :228-233 whole-state rollback (rare path)
      atomicAdd(&sw.diag[3], 1ull);
      if (backup) {  // fused sub-steps: HBM still holds the state of the launch start; this sub-step's start is in LDS
#pragma unroll
        for (int c = 0; c < 18; c++) L[u].y[c] = backup[c * 64 + threadIdx.x];
      } else {       // the start-of-step values are still in HBM
        const int i = idx[u];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          L[u].y[c]      = sw.ld(F_X + c, (unsigned)i * 8u);
          L[u].y[3 + c]  = sw.ld(F_V + c, (unsigned)i * 8u);
          L[u].y[15 + c] = sw.ld(F_W + c, (unsigned)i * 8u);
        }
#pragma unroll
        for (int c = 0; c < 9; c++) L[u].y[6 + c] = sw.ld(F_R + c, (unsigned)i * 8u);
      }
    }
  }
}

// Phase 3: MultirotorModel::step after the integrator (multirotor_model.hpp:249-281): re-orthonormalisation, ground,
// take-off patch, IMU, v_prev.
template <class SW, class PT>
DEV void post_step(const SW& sw, PT& P, const int i, Lane& L, const double mean_in, const double dt, const double inv_dt) {
  const unsigned off8 = (unsigned)i * 8u;
#define LD(f) sw.ld(f, off8)
  // re-orthonormalise, :249-253
  {
    double Rn[9];
    reorth(&L.y[6], Rn);
#pragma unroll
    for (int q = 0; q < 9; q++) L.y[6 + q] = Rn[q];
  }
  // ground, :256-262
  if (P.ground_enabled) {
    if (L.y[2] < P.ground_z && L.y[5] < 0) {
      L.y[2] = P.ground_z;
      L.y[3] = L.y[4] = L.y[5] = 0.0;
      L.y[15] = L.y[16] = L.y[17] = 0.0;
    }
  }
  // take-off patch, :264-277
  if (L.flags & FLAG_TAKEOFF) {
    if (mean_in <= P.hover_thr) {
      const double iz = LD(F_INITZ);
      if (L.y[2] < iz && L.y[5] < 0) {
        L.y[2] = iz;
        L.y[3] = L.y[4] = L.y[5] = 0.0;
        L.y[15] = L.y[16] = L.y[17] = 0.0;
      }
    } else {
      L.flags &= ~FLAG_TAKEOFF;
    }
  }
  // IMU, :280-281
  {
    double a[3];
#if MRS_FAST
    a[0] = (L.y[3] - L.vp[0]) * inv_dt;
    a[1] = (L.y[4] - L.vp[1]) * inv_dt;
    a[2] = (L.y[5] - L.vp[2]) * inv_dt + P.g;
#else
    a[0] = ((L.y[3] - L.vp[0]) / dt) + 0.0;
    a[1] = ((L.y[4] - L.vp[1]) / dt) + 0.0;
    a[2] = ((L.y[5] - L.vp[2]) / dt) + P.g;
#endif
    const double* Rn = &L.y[6];
#pragma unroll
    for (int q = 0; q < 3; q++) L.imu[q] = (Rn[q] * a[0] + Rn[3 + q] * a[1]) + Rn[6 + q] * a[2];
    L.vp[0] = L.y[3]; L.vp[1] = L.y[4]; L.vp[2] = L.y[5];
  }
#undef LD
  (void)inv_dt;
  (void)dt;
}


}  // namespace

// -DMRS_TS=1 (tools/build_variants.sh stepflag): wall-clock stamps of the first 128 blocks of the boundary launches at the joints
// of the kernel, read back with mrs_debug_ts_read (tools/boundary_phases.py) — where a lone wave's 20 us go
#ifdef MRS_TS
#ifndef MRS_TS_PART  // which launches are stamped: MRS_PART_BOUNDARY (2, default) | MRS_PART_INTERIOR (1) | MRS_PART_FULL (0: serial form)
#define MRS_TS_PART 2
#endif
// (boundary launches: their first 128 blocks; the big launches: every 15th block)
#define MRS_TS_ROW(b) ((MRS_TS_PART) == 2 ? (int)(b) : ((int)(b) % 15 == 7 ? (int)(b) / 15 : 9999))
__device__ unsigned long long mrs_ts_buf[128 * 16];
#define MRS_STAMP(k)                                                                                              \
  if (COLL && part == (MRS_TS_PART) && MRS_TS_ROW(blockIdx.x) < 128 && threadIdx.x == 0 && (fresh(cd0).tau & 15u) == 9u) { \
    asm volatile("" ::: "memory");                                                                                \
    mrs_ts_buf[MRS_TS_ROW(blockIdx.x) * 16 + (k)] = (unsigned long long)wall_clock64();                           \
  }
#else
#define MRS_STAMP(k)
#endif
namespace {
// Start of a fused step + collision launch: what the launch knows of stale lists.  Lists that stopped being usable after tick T (some
// UAV left its skin during step T, on any rank) turn every later launch into a no-op until the host has repeated the search and replays
// those ticks (tick_single.hip, tick_sharded.hip).  Folds the headers of the gathered export blocks into the rank's own words (sharded,
// not for interior launches), mirrors words for the host (first lane of the launch) and returns true when this launch is a no-op.
// Wave-uniform.
template <bool SHARD, bool UNIFORM, class CDT>
DEV bool coll_fold_and_decide(CDT& cd0, const int part, const uint32_t stall_own) {
  CDT& cd = fresh(cd0);
  // Lists that stopped being usable after tick T (some UAV left its skin during step T, on any rank) turn every later launch
  // into a no-op until the host has repeated the search and replays those ticks (tick_single.hip, tick_sharded.hip).  Wave-uniform.
  uint32_t stall = (SHARD && cd.world > 1) ? stall_own : cd.ctl[CTL_STALL];
  const bool lead_lane = blockIdx.x == 0 && threadIdx.x == 0 && UNIFORM;
  if ((SHARD && cd.world > 1) && part != MRS_PART_INTERIOR) {
    // (an interior launch runs beside the collective that fills these headers: it knows what the boundary launches folded into the
    //  rank's own header words — by the time a launch after T starts, every report of a stall T has got there: DESIGN §5)
    uint32_t warn = 0u, herr = 0u;  // the headers also carry every rank's warning and error words: all ranks learn of them in the same launch
    // (the gathered buffer was filled by the collective before this launch and nobody writes it while the launch runs: scalar loads)
    typedef const __attribute__((address_space(4))) uint32_t CU32;
    for (int q = 0; q < cd.world; q++) {
      CU32*          hq = (CU32*)(uintptr_t)(cd.g_pos + (size_t)q * (size_t)cd.block);
      const uint32_t h = hq[MRS_HDR_STALL], wq = hq[MRS_HDR_WARN];
      herr |= hq[MRS_HDR_ERROR];
      if (h != 0u && (stall == 0u || h < stall)) stall = h;
      if (wq != 0u && (warn == 0u || wq < warn)) warn = wq;
    }
    if (lead_lane) {
      // an error reported by ANY rank's kernels makes every rank's call fail (the results of the whole swarm are void)
      if ((herr & 3u) != 0u) __hip_atomic_fetch_or((mrs_gu32*)&cd.ctl[CTL_ERROR], (herr & 3u) << 8, MRS_RLX_AGENT);
      if (stall != 0u) word_min_nz(stall_word_of<SHARD>(cd), stall);
      if (warn != 0u) word_min_nz(warn_word_of<SHARD>(cd), warn);
      // host mirrors: a full launch is alone on the device, a boundary launch writes the mirrors of its own chain
      if (stall != 0u) __hip_atomic_store(&cd.hostw[part == MRS_PART_FULL ? CTL_STALL : CTL_STALL2], stall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (warn != 0u) __hip_atomic_store(&cd.hostw[part == MRS_PART_FULL ? CTL_WARN : CTL_WARN2], word_load(warn_word_of<SHARD>(cd)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (lead_lane && part == MRS_PART_INTERIOR) {
    // the interior chain's host mirrors have ONE writer at any time: the first block of the launch that has started last
    const uint32_t ws = word_load(warn_word_of<SHARD>(cd));
    if (stall != 0u) __hip_atomic_store(&cd.hostw[CTL_STALL], stall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (ws != 0u) __hip_atomic_store(&cd.hostw[CTL_WARN], ws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // (also by a launch that turns out to be a no-op: a boundary launch that has not heard of the stall yet must not wait in vain)
  if (lead_lane && part == MRS_PART_INTERIOR) word_store(&cd.ctl[CTL_I_STARTED], cd.tau);
  if (stall != 0u && cd.tau > stall) {
    if (lead_lane && part == MRS_PART_FULL && (!SHARD || cd.world == 1) && cd.ctl[CTL_STALL] == 0u) {
      cd.ctl[CTL_STALL] = stall;
      __hip_atomic_store(&cd.hostw[CTL_STALL], stall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return true;
  }
  if (lead_lane && part != MRS_PART_BOUNDARY)
    __hip_atomic_store(&cd.hostw[CTL_PROGRESS], cd.tau, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return false;
}

// One single-wavefront workgroup steps 64*NU UAVs; lane l owns UAVs blk*64*NU + u*64 + l (u < NU), so every field access
// stays a coalesced 512-B row.
// UNIFORM: all UAVs of the workgroup have the same airframe type (the host keeps `type | n_motors<<16` per 64-UAV block,
// 0xFFFF = mixed); the constants are then read through the scalar cache into SGPRs.  Mixed blocks are skipped here and
// handled by the MIXED launch over the (normally empty) list of mixed blocks, with per-lane constants.
// COLL: the launch also evaluates the collision tick that followed the previous step (see CollDev in swarm_layout.h) — single-step
// kernels only (collisions act between any two steps).
// `took_part` (COLL kernels of a split sharded tick): set once the wave-uniform exits are behind the block — the block then owes its
// epoch word / ticket to the launches that run beside this one (step_kernel_publish), whatever its lanes do afterwards.
// HK: what a launch does around each fused sub-step besides stepping (MULTI only; rollout_device.inc).  enter() runs once per lane
// after the wave-uniform exits and may finish the lane itself (true); cmd(s) runs at the top of sub-step s, before the controller
// cascade, cmd_lane(s) behind it with the lane (the state BEFORE the sub-step: the feedback hook of rollout_cost_device.inc), and obs(s) after post_step.  The default does nothing: every kernel of this file compiles as it did without the hook.
// The tick hooks (rollout_tick_device.inc) ride on the single-GPU COLL kernels instead: one step per launch, and held(), the last
// thing a held lane does — in COLL kernels a held lane takes part in the collisions and leaves inside MRS_COLLIDE_THEN, so enter()
// cannot finish it.  A hook type says which it is: kOnCollKernels.
struct NoStepHook {
  static constexpr bool kOnCollKernels = false;
  template <class SW>
  __device__ __forceinline__ bool enter(const SW&, int, Lane&, int) const { return false; }
  template <class SW>
  __device__ __forceinline__ void cmd(const SW&, int, int) const {}
  template <class SW, class PT>
  __device__ __forceinline__ void cmd_lane(const SW&, PT&, int, const Lane&, int) const {}
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW&, PT&, int, const Lane&, int) const {}
  template <class SW>
  __device__ __forceinline__ void held(const SW&, int, const Lane&, uint32_t) const {}
};
// The joints between the steps of a fused launch (FUSE > 0 in step_kernel_body).  At the top of every step the carried values pass
// an empty asm in the form a buffer load hands them out (two dwords, bit-cast to a double): the step's code then sees its inputs as
// the single-step kernel sees the state it has loaded - opaque values of the same kind -, so that the compiler orders and contracts
// the step's arithmetic as it does there, and nothing is contracted or reassociated across a step boundary.  At the end of every step
// the IMU goes out under the branch the single-step kernel has around its IMU stores: the IMU arithmetic of every step has the uses
// it has there.  A launch that is not the run's last leaves the columns alone; the run's last launch writes them FUSE times, the
// last step's stores last in program order - 24 B per UAV and earlier step beyond what the result needs, once per run.
DEV void fused_opaque(double& v) {
  mrs_v2u t = __builtin_bit_cast(mrs_v2u, v);
  asm volatile("" : "+v"(t));
  v = __builtin_bit_cast(double, t);
}
DEV void fused_step_entry(Lane& L) {
#pragma unroll
  for (int c = 0; c < 18; c++) fused_opaque(L.y[c]);
#pragma unroll
  for (int c = 0; c < 3; c++) fused_opaque(L.vp[c]);
#pragma unroll
  for (int m = 0; m < 4; m++) fused_opaque(L.pre_rpm[m]);
}
template <class SW>
DEV void fused_step_exit(const SW& sw, const int i, const Lane& L) {
  if (!(sw.opts & MRS_OPT_IMU_DEAD)) {
#pragma unroll
    for (int c = 0; c < 3; c++) sw.st(F_IMU + c, (unsigned)i * 8u, L.imu[c]);
  }
}
// FUSE = D > 0 (the *_fuseD kernels of a plain run of steps): D consecutive single steps of the block in one launch.  The per-step code
// is the single-step kernel's (commands, rpm and force fetched in the prologue), the loop is kept rolled, and x, v, R, w, v_prev and the
// rpm of the first four motors are carried in registers from one step to the next (fused_step_entry); the rpm of further motors goes
// through its columns every step, as in the MULTI kernels.
template <bool CASCADE, bool UNIFORM, int NU, bool MULTI, int SU, bool COLL, bool PIDPRE = false, bool SHARD = false, class HK = NoStepHook,
          int FUSE = 0, class SW, class CDT>
DEV void step_kernel_body(const SW& sw, const double dt, const double inv_dt, const int substeps_arg, CDT& cd0, int& blk_out, bool& took_part,
                          const HK& hk = HK()) {
  static_assert(!COLL || (NU == 1 && !MULTI), "fused collision evaluation: one UAV per lane, one step per launch");
  static_assert(FUSE == 0 || (FUSE >= 2 && NU == 1 && !MULTI && !COLL && !CASCADE && UNIFORM && __is_same(HK, NoStepHook)),
                "fixed-depth fused steps: the plain model-step family, single-type blocks");
  constexpr bool LOOPED = MULTI || FUSE > 0;  // more than one step per launch: start-of-step backup in LDS for the NaN rollback
  static_assert(__is_same(HK, NoStepHook) || (NU == 1 && MULTI && !COLL) || (HK::kOnCollKernels && NU == 1 && !MULTI && COLL && !SHARD),
                "sub-step hooks: one UAV per lane, fused sub-steps, no collisions (the tick hooks: one step, single-GPU collisions)");
  // MULTI = false compiles the substep loop away: with the loop the state is loop-carried and the per-type constants are
  // hoisted in front of it, which costs the fused kernel ~120 registers (350 vs 227) and with them its second wave per SIMD
  const int substeps = MULTI ? substeps_arg : (FUSE > 0 ? FUSE : 1);
  // the launches of a plain run of steps may be told to leave the IMU columns alone (epilogue).  The collision / sharded ticks never
  // are (a stall and its replay change after the fact which launch was the last one), nor the rollouts (hooked kernels)
  constexpr bool IMU_OPT = !COLL && __is_same(HK, NoStepHook);
  // Prologue: every load the step starts from is issued BEFORE the first data-dependent exit (mixed block, tail lane, UAV on
  // hold), from addresses that are valid for every lane, and an asm memory barrier keeps the compiler from sinking them below
  // those exits — otherwise the block-type word, the flag word and the state would be three dependent memory round trips
  // at the head of every wave.
  int blk = ((int)blockIdx.x + sw.blk0) * NU;
  if (!UNIFORM) blk = sw.MB[blockIdx.x];
  // split sharded tick: the boundary launch walks its block list (an empty list: ONE block that only keeps the protocol going),
  // the interior launch covers all blocks and leaves the boundary ones alone
  int      part = MRS_PART_FULL;
  bool     idle = false, bnd_fast = false, l1_again = false;
  uint32_t cls  = 0u;
  if (COLL && SHARD) {
    CDT& cd = fresh(cd0);
    part    = cd.part;
    // (block list and classes are written by the search and constant between two searches: read through the scalar cache)
    typedef const __attribute__((address_space(4))) uint32_t CU32;
    if (part == MRS_PART_BOUNDARY) {
      idle = cd.n_bnd == 0u;
      blk  = idle ? 0 : (int)((CU32*)(uintptr_t)cd.blk_list)[blockIdx.x];
    }
    // the interior launch may hand out its layer-1 blocks FIRST (cd.n_l1 > 0: they sit at the back of the block list): the next
    // boundary launch waits for exactly those blocks, and a block dispatched first is its SIMD's first wave.  The rest of the grid
    // walks all blocks in index order; the layer-1 blocks it meets again leave at once, as the boundary blocks do.
    if (part == MRS_PART_INTERIOR && cd.n_l1 > 0u) {
      const uint32_t b = blockIdx.x, nbk = gridDim.x - cd.n_l1;
      l1_again = b >= cd.n_l1;
      blk      = l1_again ? (int)(b - cd.n_l1) : (int)((CU32*)(uintptr_t)cd.blk_list)[nbk - 1u - b];
    }
    if (part != MRS_PART_FULL) cls = ((CU32*)(uintptr_t)cd.blk_class)[blk];
  }
  blk_out   = blk;
  took_part = false;
  MRS_STAMP(0)
  // the two words other launches change while this one runs, asked for FIRST: vector loads return in issue order, and the wave-uniform
  // exits below would otherwise wait behind the ~40 state loads of the prologue
  uint32_t stall_own = 0u, i_started = 0u;
  if (COLL) {
    CDT& cd = fresh(cd0);
    if ((SHARD && cd.world > 1)) stall_own = word_load(stall_word_of<SHARD>(cd));
    if (part == MRS_PART_BOUNDARY) i_started = word_load(&cd.ctl[CTL_I_STARTED]);
  }
  const uint32_t bt_word = UNIFORM ? sw.BT[blk] : 0u;  // NU > 1 is only launched on single-type swarms
  Lane         L[NU];
  int          idx[NU];
  uint32_t     flags_in[NU];
#pragma unroll
  for (int u = 0; u < NU; u++) {
    const int i = (blk + u) * 64 + threadIdx.x;
    idx[u]      = (i < sw.n && !idle) ? i : -1;
  }
#pragma unroll
  for (int u = 0; u < NU; u++) {
    const int i = idx[u] < 0 ? sw.n - 1 : idx[u];  // tail lanes read the last UAV and leave below
    L[u].flags  = sw.F[i];
    flags_in[u] = L[u].flags;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      L[u].y[c]      = sw.ld(F_X + c, (unsigned)i * 8u);
      L[u].y[3 + c]  = sw.ld(F_V + c, (unsigned)i * 8u);
      L[u].y[15 + c] = sw.ld(F_W + c, (unsigned)i * 8u);
    }
#pragma unroll
    for (int c = 0; c < 9; c++) L[u].y[6 + c] = sw.ld(F_R + c, (unsigned)i * 8u);
    if (PIDPRE && CASCADE) {
#pragma unroll
      for (int c = 0; c < 24; c++) L[u].pid_pre[c] = sw.ld(F_PID + c, (unsigned)i * 8u);
    }
    if (!MULTI) {  // (with fused sub-steps the rpm columns change inside the launch: the motor stage loads them itself)
#pragma unroll
      for (int m = 0; m < 4; m++) {
        L[u].pre_cmd[m] = sw.ld(F_CMD + m, (unsigned)i * 8u);
        L[u].pre_rpm[m] = sw.ld(F_RPM + m, (unsigned)i * 8u);
      }
      if (sw.opts & 1u) {
#pragma unroll
        for (int c = 0; c < 3; c++) L[u].pre_fe[c] = sw.ld(F_FEXT + c, (unsigned)i * 8u);
      }
    }
    L[u].fe_live = (sw.opts & 1u) != 0u;
    CDT& cd = fresh(cd0);
    if (COLL && (MRS_ABL & 16)) {
      L[u].xb[0] = L[u].xb[1] = L[u].xb[2] = 0.0;
      L[u].rc_mass = L[u].rc_arm = L[u].rc_prop = 0.0;
      L[u].stale = false;
      L[u].ncnt = 0; L[u].ne0 = 0; L[u].eslot = MRS_NO_SLOT;
    } else if (COLL) {
      const PosRecord* b = cd.rec + i;
      L[u].xb[0] = b->x; L[u].xb[1] = b->y; L[u].xb[2] = b->z;
      // (one GPU: the host knows when airframe constants change and forces a search; a shard of a sharded swarm checks on the device,
      //  because the other ranks' copies of its constants must be refreshed too)
      L[u].rc_mass = L[u].rc_arm = L[u].rc_prop = 0.0;
      if ((SHARD && cd.world > 1)) {
        L[u].rc_mass = b->mass; L[u].rc_arm = b->arm_length; L[u].rc_prop = b->prop_radius;
      }
      L[u].stale = false;
      L[u].ncnt  = cd.nbr_cnt[i];
      L[u].ne0   = cd.nbr[i];
#pragma unroll
      for (int k = 0; k < MRS_NPRE; k++) L[u].ne[k] = cd.nbr[(size_t)k * (size_t)cd.n + (size_t)i];  // rows of the list: independent loads
      L[u].eslot = (SHARD && cd.world > 1) ? cd.exp_slot[i] : MRS_NO_SLOT;
    } else if (sw.vl_flag) {  // wave-uniform: neighbour lists are live
      const PosRecord* b = sw.vl_rec + i;
      L[u].xb[0] = b->x; L[u].xb[1] = b->y; L[u].xb[2] = b->z;
    }
  }
  asm volatile("" ::: "memory");
  if (COLL && !(MRS_ABL & 4)) {
    CDT& cd = fresh(cd0);
    if (coll_fold_and_decide<SHARD, UNIFORM>(cd0, part, stall_own)) return;
    took_part = part != MRS_PART_FULL;
    if (part == MRS_PART_INTERIOR && blockIdx.x == 0) {
      // What ties the two chains together (normally satisfied long ago).  Interior launch t: it has started, so interior launch t-1
      // is complete — the boundary launches take that word as their short cut —, and it goes on only when every block of boundary
      // launch t-1 has finished: the epoch words of the boundary blocks.
      const long long t0 = wall_clock64();
      for (;;) {
        bool miss = false;
        for (uint32_t j = threadIdx.x; j < cd.n_bnd; j += 64u) miss = miss || word_load(&cd.epoch[cd.blk_list[j]]) < cd.tau - 1u;
        if (__builtin_amdgcn_ballot_w64(miss) == 0ull) break;
        if ((word_load(&cd.ctl[CTL_ERROR]) & 1u) != 0u || wall_clock64() - t0 > MRS_WAIT_TICKS) {
          if (threadIdx.x == 0) raise_error(&cd.ctl[CTL_ERROR], (uint32_t*)cd.send + MRS_HDR_ERROR, 1u);
          break;
        }
        __builtin_amdgcn_s_sleep(16);
      }
    }
    if (part == MRS_PART_BOUNDARY) {
      // Boundary launch t reads records the interior launch t-1 wrote: all of them are there once interior launch t has STARTED (the
      // usual case — the interior chain runs ahead of the collective); else every lane checks the blocks of its own partners below.
      // Its first block also makes sure that interior launch t-2 is complete (t-1 has started): what that launch reported travels
      // with this launch's collective at the latest.
      const uint32_t started = i_started;
      bnd_fast = started >= cd.tau;
      if (blockIdx.x == 0 && threadIdx.x == 0 && started < cd.tau - 1u) word_wait_ge(&cd.ctl[CTL_I_STARTED], cd.tau - 1u, &cd.ctl[CTL_ERROR], (uint32_t*)cd.send + MRS_HDR_ERROR);
    }
    if (part == MRS_PART_INTERIOR && ((cls & MRS_BLK_BOUNDARY) || (l1_again && (cls & MRS_BLK_LAYER1)))) {
      took_part = false;  // (not this launch's block — or one of its first blocks has it)
      blk_out   = -1;
      return;
    }
  }
  MRS_STAMP(1)
  const uint32_t bt = bt_word & 0xFFFFu;
  if (UNIFORM && bt == 0xFFFFu) return;  // mixed blocks belong to the mixed-block launch
  if (idx[0] < 0) return;
  if (COLL) {
    // The position records of the first listed partners, fetched NOW: the entries have arrived with the state, and the (random,
    // L2-missing: the records were written by other XCDs) loads have the whole controller cascade to complete.
    CDT& cd = fresh(cd0);
    if (cd.eval && !(MRS_ABL & 2)) {
      if ((part == MRS_PART_BOUNDARY && !bnd_fast) || (part == MRS_PART_INTERIOR && (cls & MRS_BLK_LAYER1))) {
        // Some listed partner is stepped by the launch on the other stream: its record of the previous tick is ready when the epoch
        // word of its block says so.  (Partners stepped by this stream's own launches are ready by stream order, and their epoch
        // words say so too: one test for every local entry.)  Entries beyond the first MRS_NPRE are polled where they are fetched.
        // Only the lanes that still miss an epoch keep loading (a wave of pollers costs its neighbours memory bandwidth), with a pause
        // between two rounds.
        const uint32_t need = cd.tau - 1u;
        uint32_t       miss = 0u;  // bit k: entry k is live, local and its block's epoch word is not there yet
#pragma unroll
        for (int k = 0; k < MRS_NPRE; k++)
          if ((uint32_t)k < L[0].ncnt && !(L[0].ne[k] & MRS_NBR_FOREIGN)) miss |= 1u << k;
        const long long t0 = wall_clock64();
        for (;;) {
#pragma unroll
          for (int k = 0; k < MRS_NPRE; k++)
            if ((miss >> k) & 1u)
              if (word_load(&cd.epoch[L[0].ne[k] >> 6]) >= need) miss &= ~(1u << k);
          if (__builtin_amdgcn_ballot_w64(miss != 0u) == 0ull) break;
          if ((word_load(&cd.ctl[CTL_ERROR]) & 1u) != 0u || wall_clock64() - t0 > MRS_WAIT_TICKS) {
            if (threadIdx.x == 0) raise_error(&cd.ctl[CTL_ERROR], (uint32_t*)cd.send + MRS_HDR_ERROR, 1u);
            break;
          }
          __builtin_amdgcn_s_sleep(16);
        }
        asm volatile("" ::: "memory");  // (the records are loaded below, not above the poll)
#pragma unroll
        for (int k = 0; k < MRS_NPRE; k++)
          mrs_partner_pos<true>(cd, L[0].ne[k], (uint32_t)k < L[0].ncnt, L[0].pox[k], L[0].poy[k], L[0].poz[k], L[0].pow_[k]);
      } else if (part == MRS_PART_BOUNDARY) {
        // (short cut taken: nothing to wait for, but this CU's L1 may hold lines of those records as an interior wave loaded them
        //  earlier in the tick — agent-scope loads all the same)
#pragma unroll
        for (int k = 0; k < MRS_NPRE; k++)
          mrs_partner_pos<true>(cd, L[0].ne[k], (uint32_t)k < L[0].ncnt, L[0].pox[k], L[0].poy[k], L[0].poz[k], L[0].pow_[k]);
      } else {
#pragma unroll
        for (int k = 0; k < MRS_NPRE; k++) mrs_partner_pos(cd, L[0].ne[k], (uint32_t)k < L[0].ncnt, L[0].pox[k], L[0].poy[k], L[0].poz[k], L[0].pow_[k]);
      }
    }
    asm volatile("" ::: "memory");
  }
  MRS_STAMP(2)
  if (hk.enter(sw, idx[0], L[0], substeps)) return;
  if (!COLL && (L[0].flags & FLAG_HOLD)) return;    // UavSystemRos::makeStep does not iterate this UAV (src/uav_system_ros.cpp:265)
#pragma unroll
  for (int u = 0; u < NU; u++) {
    const int i = idx[u] < 0 ? idx[0] : idx[u];  // a lane without a second UAV recomputes its first one and discards it
#pragma unroll
    for (int c = 0; c < 3; c++) {
      L[u].vp[c]  = L[u].y[3 + c];
      L[u].imu[c] = 0.0;
    }
    if (L[u].flags & FLAG_VPREV_SPLIT) {  // rare: setState changed v since the last step
#pragma unroll
      for (int c = 0; c < 3; c++) L[u].vp[c] = sw.ld(F_VPREV + c, (unsigned)i * 8u);
      L[u].flags &= ~FLAG_VPREV_SPLIT;  // v_prev == v again once this launch has stepped
    }
  }
  __shared__ double y_backup[LOOPED ? 18 * 64 : 1];  // fused sub-steps: the state at the start of the current one, for the NaN rollback
// COLL: handleCollisions of the previous tick from the neighbour list -> applyForce (the F_ext columns stay authoritative:
// getExternalForce, later plain steps) and crash().  The first partner is fetched up front; the evaluation itself runs between the
// controller cascade and the motor stage, where the force is first needed — except in crash mode (the cascade must see the crash
// flag) and for a UAV on hold, which takes part in the collisions but is not iterated: those evaluate at once.
#define MRS_COLLIDE_EVAL(P)                                                                                           \
  {                                                                                                                   \
    CDT&           cd    = fresh(cd0);                                                                                \
    const int      i_    = idx[0];                                                                                    \
    const unsigned off8_ = (unsigned)i_ * 8u;                                                                         \
    bool           hit_  = false;                                                                                     \
    mrs_list_eval_wide(cd, sw.T, flags_in[0] >> FLAG_TYPE_SHIFT, i_, x_start[0], x_start[1], x_start[2], P.mass, P.arm_length, P.prop_radius, \
                       L[0].ncnt, L[0].ne, L[0].pox, L[0].poy, L[0].poz, L[0].pow_, L[0].pre_fe, hit_);               \
    L[0].fe_live = true;                                                                                              \
    if (cd.write_force) { /* else the host re-derives the latched force from the position records when somebody asks (tick_single.hip) */ \
      sw.st(F_FEXT + 0, off8_, L[0].pre_fe[0]); sw.st(F_FEXT + 1, off8_, L[0].pre_fe[1]); sw.st(F_FEXT + 2, off8_, L[0].pre_fe[2]); \
    }                                                                                                                 \
    if (hit_) L[0].flags |= FLAG_CRASHED;                                                                             \
  }
#define MRS_COLLIDE_THEN(P)                                                                                           \
  const double x_start[3] = {L[0].y[0], L[0].y[1], L[0].y[2]};                                                        \
  if (COLL) {                                                                                                         \
    CDT&      cd = fresh(cd0);                                                                                        \
    const int i = idx[0];                                                                                             \
    /* setParams / set_mass since the search (on this rank only, perhaps): partners and other ranks hold stale constants */ \
    L[0].stale = (SHARD && cd.world > 1) && (L[0].rc_mass != P.mass || L[0].rc_arm != P.arm_length || L[0].rc_prop != P.prop_radius); \
    if (cd.eval && !(MRS_ABL & 2) && (cd.crash || (L[0].flags & FLAG_HOLD))) MRS_COLLIDE_EVAL(P)                      \
    if (L[0].flags & FLAG_HOLD) {                                                                                     \
      const Pos4 pp = {L[0].y[0], L[0].y[1], L[0].y[2], (double)(flags_in[0] >> FLAG_TYPE_SHIFT)};                    \
      if ((SHARD && cd.world > 1)) store_pos_sc1(cd.p_out, cd.n, i, pp); else cd.p_out[i] = pp;                                  \
      if (L[0].eslot != MRS_NO_SLOT) cd.send[1u + L[0].eslot] = pp;                                                   \
      if (L[0].stale) report_stall<SHARD>(cd, part, cd.tau, /*exact=*/true);                                                 \
      const uint32_t fl = flags_in[0] | (L[0].flags & FLAG_CRASHED); /* nothing else of the UAV changes: it is not iterated */ \
      if (fl != flags_in[0]) sw.F[i] = fl;                                                                            \
      if constexpr (COLL && !__is_same(HK, NoStepHook)) hk.held(sw, i, L[0], fl);                                     \
      return;                                                                                                         \
    }                                                                                                                 \
  }
#define MRS_RUN_STEPS(P)                                                                                              \
  MRS_COLLIDE_THEN(P)                                                                                                 \
  for (int s = 0; s < substeps; s++) {                                                                                \
    StepConst sc[NU];                                                                                                 \
    double    mean_in[NU];                                                                                            \
    if (FUSE > 0) fused_step_entry(L[0]);                                                                             \
    if (LOOPED) _Pragma("unroll") for (int c = 0; c < 18; c++) y_backup[c * 64 + threadIdx.x] = L[0].y[c];            \
    _Pragma("unroll") for (int u = 0; u < NU; u++) if (u == 0 || idx[u] >= 0) {                                       \
      int    src_;                                                                                                    \
      double cg_[4];                                                                                                  \
      if (L[u].y[0] != L[u].y[0] + 1e300) { MRS_STAMP(3) }                                                           \
      hk.cmd(sw, idx[u], s);                                                                                          \
      hk.cmd_lane(sw, P, idx[u], L[u], s);                                                                            \
      control_cascade<CASCADE, !MULTI, PIDPRE>(sw, P, idx[u], L[u], dt, inv_dt, src_, cg_);                           \
      if (cg_[0] != cg_[0] + 1e300) { MRS_STAMP(4) }                                                                  \
      if (COLL) {                                                                                                     \
        CDT& cdm = fresh(cd0);                                                                                        \
        if (cdm.eval && !cdm.crash && !(MRS_ABL & 2)) MRS_COLLIDE_EVAL(P)                                             \
      }                                                                                                               \
      if (L[u].pre_fe[0] != L[u].pre_fe[0] + 1e300) { MRS_STAMP(5) }                                                  \
      motors_dispatch<UNIFORM, !MULTI, (FUSE > 0)>(sw, P, idx[u], L[u], src_, cg_, sc[u], mean_in[u], (int)(bt_word >> 16)); \
      if (COLL && SHARD) thrust_now = sc[0].thrust; /* displacement bound of the epilogue */                         \
      if (sc[u].thrust != sc[u].thrust + 1e300) { MRS_STAMP(6) }                                                      \
    }                                                                                                                 \
    if (NU > 1 && idx[NU - 1] < 0) {                                                                                  \
      sc[NU - 1]      = sc[0];                                                                                        \
      mean_in[NU - 1] = mean_in[0];                                                                                   \
    }                                                                                                                 \
    rk4_integrate<NU, SU>(sw, P, sc, L, idx, dt, LOOPED ? y_backup : nullptr);                                        \
    _Pragma("unroll") for (int u = 0; u < NU; u++)                                                                    \
        post_step(sw, P, idx[u] < 0 ? idx[0] : idx[u], L[u], mean_in[u], dt, inv_dt);                                 \
    hk.obs(sw, P, idx[0], L[0], s);                                                                                   \
    if (FUSE > 0) fused_step_exit(sw, idx[0], L[0]);                                                                  \
  }
  double thrust_now = 0.0;  // SHARD kernels: allocation * rpm^2 of this step (after the motor low-pass), kept for the displacement bound
  if (UNIFORM) {
    CParams& P = ((CParams*)(uintptr_t)sw.T)[bt];
    MRS_RUN_STEPS(P)
  } else {
    const TypeParams& P = sw.T[L[0].flags >> FLAG_TYPE_SHIFT];
    MRS_RUN_STEPS(P)
  }
#undef MRS_RUN_STEPS
  if (L[0].y[0] != L[0].y[0] + 1e300) { MRS_STAMP(7) }
#pragma unroll
  for (int u = 0; u < NU; u++) {
    const int i = idx[u];
    if (i < 0) continue;
    if (IMU_OPT) {
      // The IMU columns are an output only — no step reads them — so a launch that is followed by another launch of the same run
      // (MRS_OPT_IMU_DEAD, set by mrs_swarm_step_n on every launch but the last) leaves them alone: the stores stand apart from the
      // others, under a wave-uniform branch on a kernel argument.
#pragma unroll
      for (int c = 0; c < 3; c++) {
        sw.st(F_X + c, (unsigned)i * 8u, L[u].y[c]);
        sw.st(F_V + c, (unsigned)i * 8u, L[u].y[3 + c]);
        sw.st(F_W + c, (unsigned)i * 8u, L[u].y[15 + c]);
      }
#pragma unroll
      for (int c = 0; c < 9; c++) sw.st(F_R + c, (unsigned)i * 8u, L[u].y[6 + c]);
      if (FUSE > 0) {  // (the IMU left with each step; the carried rpm of the motors the block has)
#pragma unroll
        for (int m = 0; m < 4; m++)
          if (m < (int)(bt_word >> 16)) sw.st(F_RPM + m, (unsigned)i * 8u, L[u].pre_rpm[m]);
      } else if (!(sw.opts & MRS_OPT_IMU_DEAD)) {
#pragma unroll
        for (int c = 0; c < 3; c++) sw.st(F_IMU + c, (unsigned)i * 8u, L[u].imu[c]);
      }
    } else {  // fused collision ticks, sharded ticks, rollouts: every launch writes its IMU (their code is what it was)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        sw.st(F_X + c, (unsigned)i * 8u, L[u].y[c]);
        sw.st(F_V + c, (unsigned)i * 8u, L[u].y[3 + c]);
        sw.st(F_W + c, (unsigned)i * 8u, L[u].y[15 + c]);
        sw.st(F_IMU + c, (unsigned)i * 8u, L[u].imu[c]);
      }
#pragma unroll
      for (int c = 0; c < 9; c++) sw.st(F_R + c, (unsigned)i * 8u, L[u].y[6 + c]);
    }
    if (L[u].flags != flags_in[u]) sw.F[i] = L[u].flags;
    if (COLL) {
      CDT&       cd = fresh(cd0);
      const Pos4 pp = {L[u].y[0], L[u].y[1], L[u].y[2], (double)(flags_in[u] >> FLAG_TYPE_SHIFT)};  // .w: airframe type, for the partners' constants
      if (!(MRS_ABL & 1)) {  // what the partners of this UAV read in the next launch
        if ((SHARD && cd.world > 1)) store_pos_sc1(cd.p_out, cd.n, i, pp); else cd.p_out[i] = pp;
      }
      if (L[u].eslot != MRS_NO_SLOT) cd.send[1u + L[u].eslot] = pp;  // ... and the other ranks after the all-gather
      if (MRS_ABL & 8) continue;
      const double d0 = L[u].y[0] - L[u].xb[0], d1 = L[u].y[1] - L[u].xb[1], d2 = L[u].y[2] - L[u].xb[2];
      // left the skin (or a usable position turned unusable / vice versa): the lists are good for THIS tick's evaluation no more
      const bool was = mrs_pos_usable(L[u].xb[0], L[u].xb[1], L[u].xb[2]), is = mrs_pos_usable(L[u].y[0], L[u].y[1], L[u].y[2]);
      const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
      const bool   gone = L[u].stale || was != is || (was && !(dd <= cd.lim2));
      const bool   near = !gone && was && dd > cd.lim2_warn;  // most of the skin is used up: time for the host to queue the next search
      // Sharded swarms announce a UAV that MAY leave its skin within the next `horizon` steps (DESIGN §5: interior launches do not wait
      // for the collective that carries the other ranks' reports, so a report has to be that much older than the launch it stops).
      // The bound, its assumptions and the thrust term: collide_device.inc mrs_may_leave.  pred_hdt < 0: the protocol announces nothing
      // (MRS_SHARD_SPLIT=0).
      bool may_leave = false;
      if ((SHARD && cd.world > 1) && was && !gone && cd.pred_hdt >= 0.0) {
        double pa0, pthr, pdrag, gz;
        int    gen;
        if (UNIFORM) {
          CParams& Q = ((CParams*)(uintptr_t)sw.T)[bt];
          pa0 = Q.pred_a0; pthr = Q.pred_thr; pdrag = Q.pred_drag; gz = Q.ground_z; gen = Q.ground_enabled;
        } else {
          const TypeParams& Q = sw.T[flags_in[u] >> FLAG_TYPE_SHIFT];
          pa0 = Q.pred_a0; pthr = Q.pred_thr; pdrag = Q.pred_drag; gz = Q.ground_z; gen = Q.ground_enabled;
        }
        const bool   takeoff = (L[u].flags & FLAG_TAKEOFF) != 0u;
        const double init_z  = takeoff ? sw.ld(F_INITZ, (unsigned)i * 8u) : 0.0;
        may_leave = mrs_may_leave(L[u].y, dd, thrust_now, L[u].ncnt, cd.rebounce, cd.pred_hdt, cd.pred_lim, pa0, pthr, pdrag, gen, gz, takeoff, init_z);
      }
      // one lane per wave reports (the host words sit in pinned host memory: a store per lane would queue up on the bus)
      const unsigned long long m_gone = __builtin_amdgcn_ballot_w64(gone), m_near = __builtin_amdgcn_ballot_w64(near),
                               m_may  = __builtin_amdgcn_ballot_w64(may_leave);
      const int                lane0  = __builtin_ctzll(__builtin_amdgcn_ballot_w64(true));
      if ((int)threadIdx.x == lane0) {
        if (m_gone) report_stall<SHARD>(cd, part, cd.tau, /*exact=*/true);
        if (m_may) report_stall<SHARD>(cd, part, cd.tau + MRS_PRED_HORIZON, /*exact=*/false);
        if (!m_gone && m_near) report_warning<SHARD>(cd, part, cd.tau);
      }
    } else if (sw.vl_flag) {  // wave-uniform: neighbour lists are live, report a UAV that has left its skin (collide.hip)
      const double d0 = L[u].y[0] - L[u].xb[0], d1 = L[u].y[1] - L[u].xb[1], d2 = L[u].y[2] - L[u].xb[2];
      const bool   was = mrs_pos_usable(L[u].xb[0], L[u].xb[1], L[u].xb[2]), is = mrs_pos_usable(L[u].y[0], L[u].y[1], L[u].y[2]);
      if (was != is || (was && !((d0 * d0 + d1 * d1) + d2 * d2 <= sw.vl_lim2))) *sw.vl_flag = 1u;
    }
  }
}
}  // namespace

// End of a block of a split sharded tick: the launches on the other stream learn that this block's position records are in place.
// Every store of the wave has left (vmcnt drained; the records are written through), then ONE lane stores the block's epoch word.
// No arrival counter, no "last block": whoever needs a block polls that block's word (a counter that 1900 blocks add to costs
// 12 ns per add — as long as the launch itself; tools/event_pingpong.hip).
template <class CDT>
DEV void step_kernel_publish(CDT& cd0, const int blk, const bool took_part) {
  CDT& cd = fresh(cd0);
  if (cd.part == MRS_PART_FULL || !took_part || blk < 0) return;  // (wave-uniform)
  if (cd.part == MRS_PART_BOUNDARY && cd.n_bnd == 0u) return;      // (the lone block of an empty boundary launch)
#ifdef MRS_TS
  if (cd.part == (MRS_TS_PART) && MRS_TS_ROW(blockIdx.x) < 128 && threadIdx.x == 0 && (cd.tau & 15u) == 9u) mrs_ts_buf[MRS_TS_ROW(blockIdx.x) * 16 + 8] = (unsigned long long)wall_clock64();
#endif
#ifndef MRS_EXP_NO_DRAIN  // (measurement only: what the drain before the epoch word costs — the protocol needs it)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  if (threadIdx.x == 0) word_store(&cd.epoch[blk], cd.tau);
#ifdef MRS_TS
  if (cd.part == (MRS_TS_PART) && MRS_TS_ROW(blockIdx.x) < 128 && threadIdx.x == 0 && (cd.tau & 15u) == 9u) mrs_ts_buf[MRS_TS_ROW(blockIdx.x) * 16 + 9] = (unsigned long long)wall_clock64();
#endif
}

// mrs_uav_step handles every input mode; mrs_uav_model_step is the same code with the controller cascade compiled out
// (smaller register footprint) — the host launches it while no UAV of the swarm is in a cascade mode (all of them
// ACTUATOR_CMD / INPUT_UNKNOWN / crashed); mrs_uav_step_mixed covers 64-UAV blocks holding several airframe types.
// Every kernel exists twice: the plain name steps once, *_multi loops over fused substeps.  The single-step cascade
// kernel fits two waves per SIMD (227 VGPRs); with the substep loop it needs 350 registers, where one wave per SIMD
// without spills beats two with scratch traffic (29.8 vs 34 us at 100 k UAVs).
#ifndef MRS_SU  // stage-loop unroll factor of the two-wave kernels (tools/tune_step.py overrides it)
#if MRS_FAST
#define MRS_SU 4  // see rk4_stages
#else
#define MRS_SU 1  // LITERAL is best with the rolled loop at any occupancy
#endif
#endif
// -DMRS_TS_STEP=1 (tools/build_variants.sh stepflag): the first and the last block of every plain step launch stamp the wall clock at
// entry and behind their stores into a ring (mrs_debug_ts_step_read; tools/region_timeline.py) — when the launches of a short run
// really start and end, without a tracer that serialises them
#ifdef MRS_TS_STEP
__device__ unsigned long long mrs_ts_step_buf[1024 * 4];
__device__ unsigned           mrs_ts_step_cnt;
#define MRS_TS_STEP_IN                                                                                           \
  unsigned ts_i_ = 0xFFFFFFFFu;                                                                                  \
  if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1)) {                                    \
    ts_i_ = atomicAdd(&mrs_ts_step_cnt, 1u) & 1023u;                                                             \
    mrs_ts_step_buf[ts_i_ * 4 + 0] = (unsigned long long)wall_clock64();                                         \
    mrs_ts_step_buf[ts_i_ * 4 + 2] = ((unsigned long long)(unsigned)sw.blk0 << 32) | blockIdx.x;                 \
  }
#define MRS_TS_STEP_OUT \
  if (ts_i_ != 0xFFFFFFFFu) mrs_ts_step_buf[ts_i_ * 4 + 1] = (unsigned long long)wall_clock64();
#else
#define MRS_TS_STEP_IN
#define MRS_TS_STEP_OUT
#endif
#define MRS_STEP_KERNEL_ACC(name, bounds, CASCADE, UNIFORM, ACC, SU)                                          \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt) {       \
    const CollDev none{};                                                                                        \
    int  blk_;                                                                                                   \
    bool took_;                                                                                                  \
    MRS_TS_STEP_IN                                                                                               \
    step_kernel_body<CASCADE, UNIFORM, 1, false, SU, false>(ACC(sw), dt, inv_dt, 1, none, blk_, took_);          \
    MRS_TS_STEP_OUT                                                                                              \
  }
#ifndef MRS_INTERIOR_PIDPRE  // the interior launch's kernel fetches its PID columns with the state (tuning: 0 / 1)
#define MRS_INTERIOR_PIDPRE 0
#endif
#define MRS_STEP_KERNEL_COLL(name, bounds, CASCADE, UNIFORM, ACC, SU, SHARD) MRS_STEP_KERNEL_COLL_P(name, bounds, CASCADE, UNIFORM, ACC, SU, SHARD, false)
#define MRS_STEP_KERNEL_COLL_P(name, bounds, CASCADE, UNIFORM, ACC, SU, SHARD, PIDPRE)                           \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, CollDev /*read in place*/) { \
    typedef const __attribute__((address_space(4))) char CChar;                                                  \
    CCollDev* cdk = (CCollDev*)((CChar*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(CollKernArgs, cd));     \
    int  blk_;                                                                                                   \
    bool took_;                                                                                                  \
    step_kernel_body<CASCADE, UNIFORM, 1, false, SU, true, PIDPRE, SHARD>(ACC(sw), dt, inv_dt, 1, *cdk, blk_, took_); \
    if (SHARD) step_kernel_publish(*cdk, blk_, took_);                                                           \
  }
#define MRS_STEP_KERNEL(name, bounds, CASCADE, UNIFORM, BUF, SU) MRS_STEP_KERNEL_ACC(name, bounds, CASCADE, UNIFORM, SwarmAcc<BUF>, SU)
#define MRS_STEP_KERNEL_MULTI(name, bounds, CASCADE, UNIFORM, BUF, SU)                                               \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, int substeps) { \
    const CollDev none{};                                                                                           \
    int  blk_;                                                                                                      \
    bool took_;                                                                                                     \
    step_kernel_body<CASCADE, UNIFORM, 1, true, SU, false>(SwarmAcc<BUF>(sw), dt, inv_dt, substeps, none, blk_, took_); \
  }
#define MRS_FUSED_RUN_KERNEL(name, bounds, ACC, SU, D)                                                            \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt) {       \
    const CollDev none{};                                                                                        \
    int  blk_;                                                                                                   \
    bool took_;                                                                                                  \
    MRS_TS_STEP_IN                                                                                               \
    step_kernel_body<false, true, 1, false, SU, false, false, false, NoStepHook, D>(ACC(sw), dt, inv_dt, 1, none, blk_, took_); \
    MRS_TS_STEP_OUT                                                                                              \
  }
#define MRS_STEP_KERNEL_BND(name, bounds, CASCADE, ACC, SU)                                                       \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, CollDev /*read in place*/) { \
    typedef const __attribute__((address_space(4))) char CChar;                                                  \
    CCollDev* cdk = (CCollDev*)((CChar*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(CollKernArgs, cd));     \
    int  blk_;                                                                                                   \
    bool took_;                                                                                                  \
    /* the boundary launch's waves share their SIMDs with the interior launch's: they go first (the collective waits for them) */ \
    __builtin_amdgcn_s_setprio(3);                                                                               \
    step_kernel_body<CASCADE, true, 1, false, SU, true, true, true>(ACC(sw), dt, inv_dt, 1, *cdk, blk_, took_);  \
    step_kernel_publish(*cdk, blk_, took_);                                                                      \
  }
// *_buf: buffer-addressed columns (state array below 4 GiB); the plain names address columns through 64-bit pointers.
// *_w3: rolled stages in 160 VGPRs = three waves per SIMD, launched when the swarm has more than two waves per SIMD.
// *_nt: non-temporal state accesses, launched for small swarms (see MRS_LD_AUX above).
MRS_STEP_KERNEL(mrs_uav_step, (64, MRS_WAVES_PER_SIMD), true, true, false, MRS_SU)
MRS_STEP_KERNEL(mrs_uav_step_buf, (64, MRS_WAVES_PER_SIMD), true, true, true, MRS_SU)
MRS_STEP_KERNEL(mrs_uav_step_buf_w3, (64, 3), true, true, true, 1)
MRS_STEP_KERNEL_MULTI(mrs_uav_step_multi, (64, 1), true, true, false, MRS_SU)
MRS_STEP_KERNEL_MULTI(mrs_uav_step_multi_buf, (64, 1), true, true, true, MRS_SU)
MRS_STEP_KERNEL(mrs_uav_model_step, (64, MRS_WAVES_PER_SIMD), false, true, false, MRS_SU)
MRS_STEP_KERNEL(mrs_uav_model_step_buf, (64, MRS_WAVES_PER_SIMD), false, true, true, MRS_SU)
MRS_STEP_KERNEL(mrs_uav_model_step_buf_w3, (64, 3), false, true, true, 1)
typedef SwarmAcc<true, true> SwarmAccNt;
MRS_STEP_KERNEL_ACC(mrs_uav_model_step_buf_nt, (64, MRS_WAVES_PER_SIMD), false, true, SwarmAccNt, MRS_SU)
MRS_STEP_KERNEL_ACC(mrs_uav_step_buf_nt, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccNt, MRS_SU)
// *_fuseD: D single model steps per launch with the state in registers (plain runs of steps: mrs_launch_step_fused).
// They are instantiated through a macro of another name than MRS_STEP_KERNEL* ON PURPOSE: tests/test_step_kernel_table.py reads every
// MRS_STEP_KERNEL* line of this file and wants a row for it in the variant matrix of tests/test_step_variants_gpu.py, which forces a
// kernel through the single-step / tick forms these kernels do not have.  So that completeness check does not see them; their own
// table - which case forces which of them - is FUSED_KERNELS in tests/test_run_fusion_gpu.py, and tests/test_run_fusion_table.py
// holds it against the MRS_FUSED_RUN_KERNEL lines below in the same way.
typedef SwarmAcc<true, false> SwarmAccBuf;
MRS_FUSED_RUN_KERNEL(mrs_uav_model_step_buf_fuse2, (64, MRS_WAVES_PER_SIMD), SwarmAccBuf, MRS_SU, 2)
MRS_FUSED_RUN_KERNEL(mrs_uav_model_step_buf_fuse3, (64, MRS_WAVES_PER_SIMD), SwarmAccBuf, MRS_SU, 3)
MRS_FUSED_RUN_KERNEL(mrs_uav_model_step_buf_fuse4, (64, MRS_WAVES_PER_SIMD), SwarmAccBuf, MRS_SU, 4)
MRS_FUSED_RUN_KERNEL(mrs_uav_model_step_buf_nt_fuse2, (64, MRS_WAVES_PER_SIMD), SwarmAccNt, MRS_SU, 2)
MRS_FUSED_RUN_KERNEL(mrs_uav_model_step_buf_nt_fuse3, (64, MRS_WAVES_PER_SIMD), SwarmAccNt, MRS_SU, 3)
MRS_FUSED_RUN_KERNEL(mrs_uav_model_step_buf_nt_fuse4, (64, MRS_WAVES_PER_SIMD), SwarmAccNt, MRS_SU, 4)
MRS_STEP_KERNEL_MULTI(mrs_uav_model_step_multi, (64, MRS_WAVES_PER_SIMD), false, true, false, MRS_SU)
MRS_STEP_KERNEL_MULTI(mrs_uav_model_step_multi_buf, (64, MRS_WAVES_PER_SIMD), false, true, true, MRS_SU)
// *_coll: the collision tick of the previous step is evaluated in the prologue (neighbour lists), the step follows
typedef SwarmAcc<false, false> SwarmAccPtr;
MRS_STEP_KERNEL_COLL(mrs_uav_step_coll_buf, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccBuf, MRS_SU, false)
MRS_STEP_KERNEL_COLL(mrs_uav_model_step_coll_buf, (64, MRS_WAVES_PER_SIMD), false, true, SwarmAccBuf, MRS_SU, false)
MRS_STEP_KERNEL_COLL(mrs_uav_step_coll, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccPtr, MRS_SU, false)
MRS_STEP_KERNEL_COLL(mrs_uav_step_mixed_coll, (64, MRS_WAVES_PER_SIMD), true, false, SwarmAccPtr, MRS_SU, false)
// *_xcoll: the same for one shard of a sharded swarm (export-set exchange: headers, export records, announced stalls, split ticks)
MRS_STEP_KERNEL_COLL(mrs_uav_step_xcoll_buf, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccBuf, MRS_SU, true)
MRS_STEP_KERNEL_COLL(mrs_uav_model_step_xcoll_buf, (64, MRS_WAVES_PER_SIMD), false, true, SwarmAccBuf, MRS_SU, true)
MRS_STEP_KERNEL_COLL(mrs_uav_step_xcoll, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccPtr, MRS_SU, true)
MRS_STEP_KERNEL_COLL(mrs_uav_step_mixed_xcoll, (64, MRS_WAVES_PER_SIMD), true, false, SwarmAccPtr, MRS_SU, true)
// *_bnd: the boundary launch of a split sharded tick — a few dozen waves whose duration is one wave's dependent chain: PID state
// fetched with the state, one wave per SIMD's worth of registers (nothing to share them with)
#ifdef MRS_EXP_BND_NOCASCADE  // measurement only (wrong results): what the boundary chain costs without the controller cascade in it
MRS_STEP_KERNEL_BND(mrs_uav_step_coll_bnd_buf, (64, 1), false, SwarmAccBuf, MRS_SU)
#else
MRS_STEP_KERNEL_BND(mrs_uav_step_coll_bnd_buf, (64, 1), true, SwarmAccBuf, MRS_SU)
#endif
// *_coll_buf_nt: the interior launch of a split sharded tick with non-temporal state accesses — it leaves no dirty state lines in the
// L2s, which every kernel boundary of the boundary chain (boundary launch, collective) running beside it would have to write back
MRS_STEP_KERNEL_COLL_P(mrs_uav_step_coll_buf_nt, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccNt, MRS_SU, true, (MRS_INTERIOR_PIDPRE != 0))
MRS_STEP_KERNEL(mrs_uav_step_mixed, (64, MRS_WAVES_PER_SIMD), true, false, false, MRS_SU)
MRS_STEP_KERNEL_MULTI(mrs_uav_step_mixed_multi, (64), true, false, false, MRS_SU)

// Test hook: the cascade's own pid_update over caller-given sequences, one lane per sequence (row-major [n_seq][n_steps] arrays;
// event 1 = reset() before the update, 2 = setSaturation(new_sat) before the update) — lets a parity test put the reference's
// PIDController vectors (tests/golden/pid_reference_vectors.npz) straight to the device code.
extern "C" __global__ void KNAME(mrs_pid_probe)(const double* params, const double* err, const double* dts, const double* event,
                                                const double* new_sat, double* out, int n_seq, int n_steps) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_seq) return;
  const double kp = params[q * 5 + 0], kd = params[q * 5 + 1], ki = params[q * 5 + 2], aw = params[q * 5 + 4];
  double       sat = params[q * 5 + 3], last_error = 0.0, integral = 0.0;
  for (int k = 0; k < n_steps; k++) {
    const size_t at = (size_t)q * n_steps + k;
    if (event[at] == 1.0) {
      last_error = 0.0;
      integral   = 0.0;
    } else if (event[at] == 2.0) {
      sat = new_sat[at];
    }
    const double dt = dts[at];
    out[at]         = pid_update(kp, kd, ki, sat, aw, last_error, integral, err[at], dt, 1.0 / dt);
  }
}
// one PIDController::update for each of n controllers with caller-held state {last_error, integral} (in/out): the stand-alone
// PIDController class of the facade
extern "C" __global__ void KNAME(mrs_pid_update_probe)(const double* params, double* state, const double* err, const double* dts, double* out, int n) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  double       le = state[q * 2 + 0], in = state[q * 2 + 1];
  const double dt = dts[q];
  out[q]          = pid_update(params[q * 5 + 0], params[q * 5 + 1], params[q * 5 + 2], params[q * 5 + 3], params[q * 5 + 4], le, in, err[q], dt, 1.0 / dt);
  state[q * 2 + 0] = le;
  state[q * 2 + 1] = in;
}
extern "C" hipError_t KNAME(mrs_launch_pid_update_probe)(const double* params, double* state, const double* err, const double* dts, double* out, int n,
                                                         hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(KNAME(mrs_pid_update_probe), dim3((n + 63) / 64), dim3(64), 0, st, params, state, err, dts, out, n);
  return hipGetLastError();
}
extern "C" hipError_t KNAME(mrs_launch_pid_probe)(const double* params, const double* err, const double* dts, const double* event,
                                                  const double* new_sat, double* out, int n_seq, int n_steps, hipStream_t st) {
  if (n_seq <= 0 || n_steps <= 0) return hipSuccess;
  hipLaunchKernelGGL(KNAME(mrs_pid_probe), dim3((n_seq + 63) / 64), dim3(64), 0, st, params, err, dts, event, new_sat, out, n_seq, n_steps);
  return hipGetLastError();
}

// Which member of a step-kernel family a launch takes: ONE rule for the single-step launches and the fused ones (kernel choice follows
// the whole swarm, not the part launched).
struct StepKernelChoice {
  bool force_multi, buf, w3, w3_forced, nt, nt_cascade;
};
static StepKernelChoice step_kernel_choice(const SwarmDev& sw, const int variant) {
  StepKernelChoice k;
  const int nb = (sw.n + 63) / 64;
  static const bool force_multi = getenv("MRS_FORCE_MULTI") != nullptr;  // tuning aids: A/B the looped kernels at substeps == 1,
  static const bool no_buf      = getenv("MRS_NO_BUFFER_ADDRESSING") != nullptr;  // and the pointer-addressed ones
  k.force_multi = force_multi;
  k.buf = !no_buf && (unsigned long long)F_COUNT * (unsigned long long)sw.npad * 8ull < (1ull << 32);
  // more than two waves per SIMD to place (256 CUs x 4 SIMDs): the 160-register kernels keep three resident
  static const int w3_pref = getenv("MRS_THREE_WAVES") ? atoi(getenv("MRS_THREE_WAVES")) : -1;  // tuning aid: force on/off
  // (LITERAL's three-wave build spills a few registers since it carries both RK4 passes: measured slower at 1 M, 116 vs 108.5 us)
  static const int nt_pref = getenv("MRS_NT_ACCESSES") ? atoi(getenv("MRS_NT_ACCESSES")) : -1;  // tuning aid: force on/off
  // Far beyond the Infinity Cache (>= 1.4 GB moved per step: 3.4 M UAVs model-only, 1.8 M with the cascade) every access goes to HBM and
  // nothing is read twice: the two-wave kernel with non-temporal accesses streams 5-7 % faster than the three-wave one there
  // (4 M UAVs: 301 vs 319 us; 2 M cascade: 299 vs 319 us), while from 0.3 M to 2.5 M, where the cache still holds part of the
  // state, it is up to 15 % slower (tools/gpu_size_knobs.sh).
  const bool hbm_stream = k.buf && MRS_FAST != 0 && w3_pref < 0 && nt_pref < 0 && (double)sw.npad * (variant == 1 ? 412.0 : 796.0) >= 1.4e9;
  k.w3 = k.buf && !hbm_stream && (w3_pref < 0 ? (MRS_FAST != 0 && nb > 2 * 1024) : w3_pref != 0);
  // small swarm, short launch: non-temporal state accesses too (LITERAL measured neutral: 11.5 us either way)
  k.nt = k.buf && !k.w3 && (nt_pref < 0 ? (MRS_FAST != 0 && (nb <= 1900 || hbm_stream)) : nt_pref != 0);  // 120 k UAVs: -0.5 us, 131 k: +0.8 us
  k.nt_cascade = k.buf && !k.w3 && (nt_pref < 0 ? (MRS_FAST != 0 && (nb <= 900 || hbm_stream)) : nt_pref != 0);  // 56 k UAVs: -0.4 us, 62 k: +0.25 us
  k.w3_forced = w3_pref > 0;
  return k;
}
// A plain run of this swarm may be issued as fused launches (mrs_launch_step_fused): buffer-addressed state, no mixed blocks, and none
// of the tuning aids set that ask for another kernel (MRS_FORCE_MULTI, MRS_THREE_WAVES=1: there is no three-wave fused kernel).
extern "C" int KNAME(mrs_step_fusable)(SwarmDev sw) {
  const StepKernelChoice k = step_kernel_choice(sw, 1);
  return k.buf && !k.force_multi && !k.w3_forced && sw.n_mixed == 0;
}

// variant: 0 = every input mode, 1 = model only (no UAV in a cascade mode).  The launch covers the 64-UAV blocks
// [blk0, blk0 + nblk) — the host splits a step over two streams — and, if asked to, the (normally empty) list of mixed blocks.
extern "C" hipError_t KNAME(mrs_launch_step)(SwarmDev sw, double dt, int substeps, int variant, int blk0, int nblk, int with_mixed, hipStream_t st) {
  const int nb = (sw.n + 63) / 64;  // kernel choice follows the whole swarm, not the part launched here
  if (nb <= 0 || substeps <= 0) return hipSuccess;
  sw.blk0 = blk0;
  const dim3   g(nblk > 0 ? nblk : 1), b(64);
  const double inv_dt = 1.0 / dt;  // the same IEEE division the kernels used to repeat per launch
  const StepKernelChoice k = step_kernel_choice(sw, variant);
  const bool force_multi = k.force_multi, buf = k.buf, w3 = k.w3, nt = k.nt, nt_cascade = k.nt_cascade;
  if (nblk > 0) {
    if (substeps == 1 && !force_multi) {
      if (variant == 1) {
        if (w3)
          hipLaunchKernelGGL(KNAME(mrs_uav_model_step_buf_w3), g, b, 0, st, sw, dt, inv_dt);
        else if (nt)
          hipLaunchKernelGGL(KNAME(mrs_uav_model_step_buf_nt), g, b, 0, st, sw, dt, inv_dt);
        else if (buf)
          hipLaunchKernelGGL(KNAME(mrs_uav_model_step_buf), g, b, 0, st, sw, dt, inv_dt);
        else
          hipLaunchKernelGGL(KNAME(mrs_uav_model_step), g, b, 0, st, sw, dt, inv_dt);
      } else {
        if (w3)
          hipLaunchKernelGGL(KNAME(mrs_uav_step_buf_w3), g, b, 0, st, sw, dt, inv_dt);
        else if (nt_cascade)
          hipLaunchKernelGGL(KNAME(mrs_uav_step_buf_nt), g, b, 0, st, sw, dt, inv_dt);
        else if (buf)
          hipLaunchKernelGGL(KNAME(mrs_uav_step_buf), g, b, 0, st, sw, dt, inv_dt);
        else
          hipLaunchKernelGGL(KNAME(mrs_uav_step), g, b, 0, st, sw, dt, inv_dt);
      }
    } else {
      if (variant == 1) {
        if (buf)
          hipLaunchKernelGGL(KNAME(mrs_uav_model_step_multi_buf), g, b, 0, st, sw, dt, inv_dt, substeps);
        else
          hipLaunchKernelGGL(KNAME(mrs_uav_model_step_multi), g, b, 0, st, sw, dt, inv_dt, substeps);
      } else {
        if (buf)
          hipLaunchKernelGGL(KNAME(mrs_uav_step_multi_buf), g, b, 0, st, sw, dt, inv_dt, substeps);
        else
          hipLaunchKernelGGL(KNAME(mrs_uav_step_multi), g, b, 0, st, sw, dt, inv_dt, substeps);
      }
    }
  }
  if (with_mixed && sw.n_mixed > 0) {
    sw.blk0 = 0;
    if (substeps == 1 && !force_multi)
      hipLaunchKernelGGL(KNAME(mrs_uav_step_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt);
    else
      hipLaunchKernelGGL(KNAME(mrs_uav_step_mixed_multi), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, substeps);
  }
  return hipGetLastError();
}

// `depth` (2 .. MRS_FUSE_MAX) single model steps of the blocks [blk0, blk0 + nblk) in ONE launch, the state in registers in between:
// the plain model-step family only (no UAV in a cascade mode, no mixed blocks, buffer-addressed state) - the caller has checked.
extern "C" hipError_t KNAME(mrs_launch_step_fused)(SwarmDev sw, double dt, int depth, int blk0, int nblk, hipStream_t st) {
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0 || nblk <= 0) return hipSuccess;
  const StepKernelChoice k = step_kernel_choice(sw, 1);
  if (depth < 2 || depth > MRS_FUSE_MAX || sw.n_mixed > 0 || !k.buf) return hipErrorInvalidValue;
  sw.blk0 = blk0;
  const dim3   g(nblk), b(64);
  const double inv_dt = 1.0 / dt;
  // non-temporal accesses where the single-step launch has them: small swarms, and far beyond the Infinity Cache.  Where that launch
  // takes the three-wave kernel (FAST, more than 2048 blocks) this one takes the two-wave *_fuseD: a quarter of the bytes outweighs
  // the third resident wave (MEASUREMENTS section 11, 1 M UAVs).
  const bool nt = k.nt;
#define MRS_FUSE_LAUNCH(D)                                                                             \
  case D:                                                                                              \
    if (nt)                                                                                            \
      hipLaunchKernelGGL(KNAME(mrs_uav_model_step_buf_nt_fuse##D), g, b, 0, st, sw, dt, inv_dt);       \
    else                                                                                               \
      hipLaunchKernelGGL(KNAME(mrs_uav_model_step_buf_fuse##D), g, b, 0, st, sw, dt, inv_dt);          \
    break;
  switch (depth) {
    MRS_FUSE_LAUNCH(2)
    MRS_FUSE_LAUNCH(3)
    MRS_FUSE_LAUNCH(4)
  }
#undef MRS_FUSE_LAUNCH
  return hipGetLastError();
}

#ifdef MRS_TS_STEP
extern "C" int KNAME(mrs_debug_ts_step_read)(unsigned long long* out, unsigned* count) {
  hipError_t e = hipMemcpyFromSymbol(count, HIP_SYMBOL(mrs_ts_step_cnt), sizeof(unsigned));
  if (e == hipSuccess) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(mrs_ts_step_buf), sizeof(unsigned long long) * 1024 * 4);
  return (int)e;
}
#endif
#ifdef MRS_TS
extern "C" int mrs_debug_ts_read(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mrs_ts_buf), sizeof(unsigned long long) * 128 * 16);
}
#endif
// The fused step + collision-evaluation launch (single stream, one step): variant as above.
// grid_blocks > 0: the boundary launch of a split sharded tick (one block per entry of the block list, at least one)
extern "C" hipError_t KNAME(mrs_launch_step_coll)(SwarmDev sw, CollDev cd, double dt, int variant, int grid_blocks, hipStream_t st) {
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3   g(grid_blocks > 0 ? grid_blocks : nb), b(64);
  const double inv_dt = 1.0 / dt;
  static const bool no_buf = getenv("MRS_NO_BUFFER_ADDRESSING") != nullptr;
  const bool buf = !no_buf && (unsigned long long)F_COUNT * (unsigned long long)sw.npad * 8ull < (1ull << 32);
  static const bool no_bnd = getenv("MRS_NO_BOUNDARY_KERNEL") != nullptr;  // tuning aid: the generic kernel for boundary launches too
  static const bool nt_interior = getenv("MRS_INTERIOR_NT") ? atoi(getenv("MRS_INTERIOR_NT")) != 0 : true;
  const bool shard = cd.block > 0;  // a CollDev of the export-set exchange (mrs_collide_export_dev), whatever the world size
  if (!shard) {
    if (buf && variant == 1)
      hipLaunchKernelGGL(KNAME(mrs_uav_model_step_coll_buf), g, b, 0, st, sw, dt, inv_dt, cd);
    else if (buf)
      hipLaunchKernelGGL(KNAME(mrs_uav_step_coll_buf), g, b, 0, st, sw, dt, inv_dt, cd);
    else
      hipLaunchKernelGGL(KNAME(mrs_uav_step_coll), g, b, 0, st, sw, dt, inv_dt, cd);
    if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_step_mixed_coll), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, cd);
    return hipGetLastError();
  }
  if (buf && variant == 1)
    hipLaunchKernelGGL(KNAME(mrs_uav_model_step_xcoll_buf), g, b, 0, st, sw, dt, inv_dt, cd);
  else if (buf && cd.part == MRS_PART_BOUNDARY && !no_bnd)
    hipLaunchKernelGGL(KNAME(mrs_uav_step_coll_bnd_buf), g, b, 0, st, sw, dt, inv_dt, cd);
  else if (buf && cd.part == MRS_PART_INTERIOR && nt_interior)
    hipLaunchKernelGGL(KNAME(mrs_uav_step_coll_buf_nt), g, b, 0, st, sw, dt, inv_dt, cd);
  else if (buf)
    hipLaunchKernelGGL(KNAME(mrs_uav_step_xcoll_buf), g, b, 0, st, sw, dt, inv_dt, cd);
  else
    hipLaunchKernelGGL(KNAME(mrs_uav_step_xcoll), g, b, 0, st, sw, dt, inv_dt, cd);
  if (sw.n_mixed > 0 && cd.part == MRS_PART_FULL) hipLaunchKernelGGL(KNAME(mrs_uav_step_mixed_xcoll), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, cd);
  return hipGetLastError();
}

// ---- component probe (test hook + backing of the facade's stand-alone L0 classes): ONE component of the path for every UAV of a
// range, on the UAV's own state, constants and PID columns; caller-given input row, output row written back.  Component ids and
// row layouts: MRS_COMP_* in include/mrs_swarm.h.  PID-bearing controllers update the UAV's PID columns (getControlSignal mutates
// the controller object in the reference).
extern "C" __global__ void KNAME(mrs_component_probe)(SwarmDev sw, int comp, int first, int count, const double* in, int in_stride, double* out,
                                                      int out_stride, double dt, double inv_dt) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int         i  = first + k;
  const size_t      np = (size_t)sw.npad;
  const TypeParams& P  = sw.T[sw.F[i] >> FLAG_TYPE_SHIFT];
  const double*     a  = in + (size_t)k * in_stride;
  double*           o  = out + (size_t)k * out_stride;
#define COL(f) sw.S[(size_t)(f) * np + i]
  double x[3], v[3], R[9], w[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    x[c] = COL(F_X + c); v[c] = COL(F_V + c); w[c] = COL(F_W + c);
  }
#pragma unroll
  for (int c = 0; c < 9; c++) R[c] = COL(F_R + c);
  double pid[6];
  switch (comp) {
    case 1: {  // MRS_COMP_REORTH: R * inverse(matrixL(LLT(R^T R))), multirotor_model.hpp:249-253 / :314-316
      double Rin[9];
      for (int c = 0; c < 9; c++) Rin[c] = a[c];
      reorth(Rin, o);
    } break;
    case 2: {  // MRS_COMP_MODEL_RHS: MultirotorModel::operator(), multirotor_model.hpp:301-366 (NaN components -> 0 included)
      StepConst sc;
      double    rsq[MRS_MAXM];
      for (int m = 0; m < MRS_MAXM; m++) {
        const double rpm = m < P.n_motors ? COL(F_RPM + m) : 0.0;
        rsq[m]           = rpm * rpm;
      }
      double tt[4];
      for (int r = 0; r < 4; r++) {
        double sacc = P.alloc[r * MRS_MAXM] * rsq[0];
        for (int m = 1; m < MRS_MAXM; m++)
          if (m < P.n_motors) sacc += P.alloc[r * MRS_MAXM + m] * rsq[m];
        tt[r] = sacc;
      }
      sc.tt0 = tt[0]; sc.tt1 = tt[1]; sc.tt2 = tt[2]; sc.thrust = tt[3];
      for (int c = 0; c < 3; c++) {
#if MRS_FAST
        sc.fm[c] = COL(F_FEXT + c) * P.inv_mass;
#else
        sc.fm[c] = COL(F_FEXT + c) / P.mass;
#endif
      }
      double y[18], kk[18];
      for (int c = 0; c < 18; c++) y[c] = a[c];
      model_rhs<true>(P, sc, y, kk);
      for (int c = 0; c < 18; c++) o[c] = kk[c];
    } break;
    case 3: {  // MRS_COMP_MIXER: Mixer::getControlSignal, mixer.hpp:107-144
      const double cg[4] = {a[0], a[1], a[2], a[3]};
      double       m[MRS_MAXM];
      mixer<0>(P, cg, m);
      for (int q = 0; q < MRS_MAXM; q++) o[q] = m[q];
    } break;
    case 4: {  // MRS_COMP_POSITION
      for (int q = 0; q < 6; q++) pid[q] = COL(F_PID + 0 + q);
      const double ref[3] = {a[0], a[1], a[2]};
      double       r3[3];
      position_controller(P, x, ref, pid, dt, inv_dt, r3);
      for (int q = 0; q < 6; q++) COL(F_PID + 0 + q) = pid[q];
      o[0] = r3[0]; o[1] = r3[1]; o[2] = r3[2];
    } break;
    case 5: {  // MRS_COMP_VELOCITY
      for (int q = 0; q < 6; q++) pid[q] = COL(F_PID + 6 + q);
      const double ref[3] = {a[0], a[1], a[2]};
      double       r3[3];
      velocity_controller(P, v, ref, pid, dt, inv_dt, r3);
      for (int q = 0; q < 6; q++) COL(F_PID + 6 + q) = pid[q];
      o[0] = r3[0]; o[1] = r3[1]; o[2] = r3[2];
    } break;
    case 6: {  // MRS_COMP_ACCELERATION_HDG: acc[3], heading -> Rd[9], throttle
      const double acc[3] = {a[0], a[1], a[2]};
      double       fdn[3], Rd[9];
      const double thr = acceleration_thrust(P, R, acc, fdn);
      acceleration_attitude(fdn, a[3], Rd);
      for (int q = 0; q < 9; q++) o[q] = Rd[q];
      o[9] = thr;
    } break;
    case 7: {  // MRS_COMP_ACCELERATION_HDG_RATE: acc[3], heading rate -> tilt[3], heading rate, throttle
      const double acc[3] = {a[0], a[1], a[2]};
      double       fdn[3];
      const double thr = acceleration_thrust(P, R, acc, fdn);
      o[0] = fdn[0]; o[1] = fdn[1]; o[2] = fdn[2]; o[3] = a[3]; o[4] = thr;
    } break;
    case 8:    // MRS_COMP_ATTITUDE: Rd[9], throttle -> rate[3], throttle
    case 9: {  // MRS_COMP_TILT_HDG_RATE: tilt[3], heading rate, throttle -> rate[3], throttle
      for (int q = 0; q < 6; q++) pid[q] = COL(F_PID + 12 + q);
      double Rd[9], rate[3];
      if (comp == 8) {
        for (int q = 0; q < 9; q++) Rd[q] = a[q];
      } else {
        const double tilt[3] = {a[0], a[1], a[2]};
        tilt_attitude(R, tilt, Rd);
      }
      attitude_error_pids(P, R, Rd, pid, dt, inv_dt, rate);
      for (int q = 0; q < 6; q++) COL(F_PID + 12 + q) = pid[q];
      if (comp == 9) rate[2] += tilt_yaw_rate(sw.diag, R, rate, a[3]);
      o[0] = rate[0]; o[1] = rate[1]; o[2] = rate[2];
      o[3] = comp == 8 ? a[9] : a[4];
    } break;
    case 10: {  // MRS_COMP_RATE: rate[3], throttle -> roll, pitch, yaw, throttle
      for (int q = 0; q < 6; q++) pid[q] = COL(F_PID + 18 + q);
      const double rate[3] = {a[0], a[1], a[2]};
      double       cg[4];
      rate_controller(P, w, rate, a[3], pid, dt, inv_dt, cg);
      for (int q = 0; q < 6; q++) COL(F_PID + 18 + q) = pid[q];
      o[0] = cg[0]; o[1] = cg[1]; o[2] = cg[2]; o[3] = cg[3];
    } break;
    default: break;
  }
#undef COL
  (void)x; (void)v; (void)w;
}
extern "C" hipError_t KNAME(mrs_launch_component_probe)(SwarmDev sw, int comp, int first, int count, const double* in, int in_stride, double* out,
                                                        int out_stride, double dt, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(KNAME(mrs_component_probe), dim3((count + 63) / 64), dim3(64), 0, st, sw, comp, first, count, in, in_stride, out, out_stride, dt,
                     1.0 / dt);
  return hipGetLastError();
}

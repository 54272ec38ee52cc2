/*
 * abrk_types.h - constants and the arm description of the libabrk C ABI (see abrk.h, which includes this file).
 * Kept apart so that the runtime-table kernels (abr_control_amd/csrc/abrk_rt.h), which only need the arm
 * description, do not depend on the list of entry points.
 */
#ifndef ABRK_TYPES_H
#define ABRK_TYPES_H

#include <stdint.h>

#define ABRK_VERSION 100
#define ABRK_MAX_JOINTS 7
#define ABRK_MAX_NULL 4

enum { ABRK_F64 = 0, ABRK_F32 = 1 };

enum {
  ABRK_OK = 0,
  ABRK_EINVAL = -1,   /* bad argument (shape, id, dtype, unsupported combination)      */
  ABRK_ENODEV = -2,   /* no HIP device / HIP runtime error                              */
  ABRK_ENOMEM = -3,   /* device allocation failed                                       */
  ABRK_ENOARM = -4,   /* unknown arm id / name                                          */
  ABRK_EFRAME = -5,   /* invalid frame id ("Invalid transformation name", ur5/config.py:337) */
  ABRK_EPATH = -7,    /* the path planner's plan pass (abrk_path_plan_batch) met a row without a path: start == target, no
                         max_v candidate whose ramps fit the curve (the reference raises ValueError,
                         path_planners/path_planner.py:245), fewer than 2 steps.  n_timesteps is 0 for those rows; reported
                         like ABRK_ESINGULAR (the call itself for host arrays, else the stream's next sync).        */
  ABRK_ESINGULAR = -6 /* a row's joint-space inertia matrix M is not positive definite: where the reference's
                         numpy.linalg.inv(M) raises LinAlgError (controllers/osc.py:136).  Host-array calls return
                         it themselves (the outputs of the offending rows are unspecified, every other row is
                         valid); device-pointer calls are asynchronous - the flag is kept per (device, stream) and is
                         returned (once) by whatever drains THAT stream next: abrk_stream_sync, abrk_memcpy_d2h on
                         it, or abrk_device_sync (any stream of the device).  Another stream's sync never reports it.
                         Raised by abrk_osc_generate_batch / _full_batch / _sharded, abrk_osc_law_batch and the fused
                         rollout; NOT by the helper abrk_osc_mx_batch (a singular M gives non-finite Mx / M_inv there)
                         nor by the measurement variant abrk_osc_generate_coop_batch.
                         Difference to the reference: the test is "a Cholesky pivot of M is a real number <= 0", the
                         reference's is LAPACK's "exactly singular" (getrf hits a zero pivot).  In fp64 the two agree
                         on every M a rigid-body model produces; in fp32 (dtype ABRK_F32) a valid but ill-conditioned
                         M (cond ~1e7 and beyond) can round a pivot to <= 0 and raise here where the reference - which
                         inverts a float32 M too, osc.py:136 - returns finite values of no accuracy.               */
};

/* History columns of abrk_loop_trace_batch (abrk.h), in the order they take in a history row: q, dq, u [n],
 * target [6], xyz [3], err [1]. */
enum {
  ABRK_TR_Q = 1u << 0,
  ABRK_TR_DQ = 1u << 1,
  ABRK_TR_U = 1u << 2,
  ABRK_TR_TARGET = 1u << 3,
  ABRK_TR_XYZ = 1u << 4,
  ABRK_TR_ERR = 1u << 5
};

/* ---------------------------------------------------------------------------------
 * Arm description = the constant table a reference `Config.__init__` + `_calc_T`
 * encode symbolically (abr_control/arms/ur5/config.py:35-339, jaco2/config.py:35-356,
 * twojoint/config.py:30-181, threejoint/config.py:32-223, onejoint/config.py:30-133).
 *
 *   T(link0)     = A0
 *   T(joint_i)   = T(link_i) * AJ[i]
 *   T(link_i+1)  = T(joint_i) * Rz(q_i) * B[i]          (all joints revolute about local z)
 *   T(EE)        = T(link_n) * E   if has_ee else T(link_n)
 *
 * Each static transform is a 3x4 row-major affine [R | t] (bottom row 0 0 0 1 implied);
 * R need not be exactly orthogonal (Jaco2's 8-digit constants are not) - the kernels
 * differentiate the affine chain exactly.
 * mdiag[l] = diagonal of the reference's 6x6 `_M_LINKS[l]` (m,m,m,Ixx,Iyy,Izz), applied
 * in the WORLD frame exactly as base_config.py:628 does.  Only links l < n_links_dyn
 * (= the reference's N_LINKS) enter M, g and C (base_config.py:449,626).
 * --------------------------------------------------------------------------------- */
typedef struct abrk_arm_desc {
  int32_t n_joints;
  int32_t n_links_dyn;
  int32_t has_ee;
  int32_t reserved;
  double A0[12];
  double AJ[ABRK_MAX_JOINTS][12];
  double B[ABRK_MAX_JOINTS][12];
  double E[12];
  double mdiag[ABRK_MAX_JOINTS + 1][6];
  char name[32];
} abrk_arm_desc;

/* ---------------------------------------------------------------------------------
 * Full inertias of a general-inertia arm (compiled arms only, abrk_arm_create_compiled_inertia): the reference's
 * 6x6 `_M_LINKS[l]` (base_config.py:449-451, 626-628) and `_M_JOINTS[j]` - motor / rotor inertias, applied through the
 * Jacobian of the joint frame (:452-455, 629-632) - row-major, in the WORLD frame like mdiag.  Matrices are symmetric.
 * mlink[l] for l < n_links_dyn counts; its diagonal is mdiag[l] (the kernels add the off-diagonal remainder).  Joint
 * frame j moves with joints 0..j-1 only, so mjoint[0] contributes nothing, as in the reference.
 * A plain arm's inertia is diag(mdiag[l]) per link and zero per joint.
 * --------------------------------------------------------------------------------- */
typedef struct abrk_arm_inertia {
  double mlink[ABRK_MAX_JOINTS + 1][36];
  double mjoint[ABRK_MAX_JOINTS][36];
} abrk_arm_inertia;

#endif /* ABRK_TYPES_H */

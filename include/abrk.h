/*
 * abrk.h - C ABI of libabrk.so, the MI355X-native batched operational-space-control engine.
 *
 * This is the drop-in boundary for ONE hot path of abr/abr_control: the per-timestep
 * evaluation of an arm's kinematics/dynamics and the control laws built on it.  Every
 * entry point below names the reference interface (file:line under /root/reference)
 * it replaces.  The reference evaluates one joint state per call through SymPy-generated
 * Cython functions; this library evaluates a batch of B independent joint states per
 * call with hand-written HIP kernels for gfx950.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, caller-owned buffers, no allocation inside
 *     the compute calls.  Arrays are row-major [B, ...] exactly like the reference's
 *     per-call outputs stacked along a leading batch axis.
 *   - dtype selects the arithmetic AND the element type of every array argument:
 *     ABRK_F64 (double) or ABRK_F32 (float).
 *   - Every array pointer may be a device pointer (zero-copy) or a host pointer (the
 *     library stages it through device scratch on the given stream and copies results
 *     back before returning).  Detection is by hipPointerGetAttributes.
 *   - `device` is a HIP device ordinal; `stream` is a hipStream_t (NULL = default
 *     stream of that device).  Calls with device pointers are asynchronous on `stream`;
 *     calls that had to stage host memory synchronise the stream before returning.
 *   - Return value: 0 on success, negative ABRK_E* code on failure; abrk_last_error()
 *     returns a thread-local message.  There is NO CPU fallback: without a usable HIP
 *     device every compute call fails with ABRK_ENODEV.
 *   - Re-entrant per (device, stream): concurrent calls must use distinct streams.
 *
 * Frames are addressed by integer id: link_i -> 2*i, joint_i -> 2*i+1, "EE" ->
 * 2*n_joints+1 (the reference addresses them by the strings "link{i}", "joint{i}",
 * "EE": e.g. abr_control/arms/ur5/config.py:301-339).
 */
#ifndef ABRK_H
#define ABRK_H

#include <stddef.h>
#include <stdint.h>

#include "abrk_types.h" /* ABRK_VERSION, limits, dtype / error codes, abrk_arm_desc */

#ifdef __cplusplus
extern "C" {
#endif

/* Built-in arms ("ur5", "jaco2", "twojoint", "threejoint", "onejoint"): compile-time
 * specialised kernels.  Returns an arm id >= 0 or ABRK_ENOARM.                        */
int abrk_arm_builtin(const char* name);
/* Register a user arm (runtime table; generic kernels).  Returns arm id >= 0.
 * Replaces writing a BaseConfig subclass + first-use SymPy/Cython code generation
 * (base_config.py:125-146).                                                            */
int abrk_arm_create(const abrk_arm_desc* desc);
/* Register a user arm together with kernels compiled for its own table - the counterpart of the reference's cached
 * generated functions (base_config.py:173-191: `_load_from_file` imports the Cython module generated for this arm;
 * _generate_and_save_function :125-146 writes it).  `plugin_path` is a shared object built by
 * `make -C abr_control_amd/csrc plugin` from the same description (abr_control_amd/specialize.py generates the source,
 * runs the build and caches the result); it is checked against `desc` value by value and against abrk_plugin_abi(), and
 * refused with ABRK_EINVAL on any mismatch.  The arm then runs the same compile-time specialised kernels as a built-in
 * arm (about 2.2x the rate of the runtime-table kernels abrk_arm_create gives).  Returns arm id >= 0.                */
int abrk_arm_create_compiled(const abrk_arm_desc* desc, const char* plugin_path);
/* The same for an arm with full link inertias and joint inertias (abrk_types.h abrk_arm_inertia): `inertia` is checked
 * value by value against the one the plugin was compiled for, like `desc`.  NULL stands for the plain form of `desc`
 * (diagonal link inertias, no joint inertias), i.e. abrk_arm_create_compiled.  General inertias run on compiled arms
 * only: abrk_arm_create has no inertia argument.  Returns arm id >= 0.                                                  */
int abrk_arm_create_compiled_inertia(const abrk_arm_desc* desc, const abrk_arm_inertia* inertia,
                                     const char* plugin_path);
/* the inertias an arm runs with: the plain form (diag(mdiag), zero joint inertias) for every arm but a general-inertia
 * compiled one                                                                                                        */
int abrk_arm_get_inertia(int arm_id, abrk_arm_inertia* out);
/* tag of the kernel headers and compile flags this library was built from; a plugin must carry the same one */
const char* abrk_plugin_abi(void);
int abrk_arm_get_desc(int arm_id, abrk_arm_desc* out);
int abrk_arm_destroy(int arm_id);

/* ---------------------------------------------------------------------------------
 * Dynamics: replaces the generated `autofunc_c(q0..,[dq0..],[x,y,z])` calls behind
 * BaseConfig.Tx/J/M/g/C/dJ/R/T/T_inv (base_config.py:210-415).  One launch evaluates
 * every requested quantity for all B states; FK is shared between them.
 *   want-mask bit      output (row-major per state)                reference wrapper
 *   ABRK_WANT_TX       Tx  [B,3]      position of x in `frame`     base_config.py:371
 *   ABRK_WANT_J        J   [B,6,n]    Jacobian of that point       base_config.py:249
 *   ABRK_WANT_M        M   [B,n,n]    joint-space inertia          base_config.py:272
 *   ABRK_WANT_G        g   [B,n]      gravity torque               base_config.py:210
 *   ABRK_WANT_C        C   [B,n,n]    Christoffel Coriolis matrix  base_config.py:320
 *   ABRK_WANT_DJ       dJ  [B,6,n]    time derivative of J         base_config.py:225
 *   ABRK_WANT_R        R   [B,3,3]    rotation of `frame`          base_config.py:287
 *   ABRK_WANT_T        T   [B,4,4]    transform of `frame`         base_config.py:338
 *   ABRK_WANT_TINV     Ti  [B,4,4]    inverse transform            base_config.py:394
 *   ABRK_WANT_QUAT     quat[B,4]      (w,x,y,z) of `frame`         base_config.py:304
 * Outputs keep full `dtype` precision; the reference's float32 rounding of
 * J/M/g/C/dJ/R (base_config.py:223,247,270,285,301,336) is applied by the Python layer.
 * q: [B,n]; dq: [B,n] (needed for C/dJ, else may be NULL); x_off: [3] host values or NULL.
 * --------------------------------------------------------------------------------- */
enum {
  ABRK_WANT_TX = 1u << 0,
  ABRK_WANT_J = 1u << 1,
  ABRK_WANT_M = 1u << 2,
  ABRK_WANT_G = 1u << 3,
  ABRK_WANT_C = 1u << 4,
  ABRK_WANT_DJ = 1u << 5,
  ABRK_WANT_R = 1u << 6,
  ABRK_WANT_T = 1u << 7,
  ABRK_WANT_TINV = 1u << 8,
  ABRK_WANT_QUAT = 1u << 9
};

typedef struct abrk_dyn_out {
  void* Tx;
  void* J;
  void* M;
  void* g;
  void* C;
  void* dJ;
  void* R;
  void* T;
  void* Tinv;
  void* quat;
} abrk_dyn_out;

int abrk_dynamics_batch(int arm_id, int dtype, int64_t B, const void* q, const void* dq,
                        int frame, const double* x_off, uint32_t want,
                        const abrk_dyn_out* out, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * Secondary (null-space / joint-space) controllers: Damping.generate
 * (controllers/damping.py:21-32), RestingConfig.generate (resting_config.py:18-42) and
 * Joint.generate (joint.py:104-131, angle states only).
 * --------------------------------------------------------------------------------- */
enum { ABRK_NULL_DAMPING = 1, ABRK_NULL_RESTING = 2 };

typedef struct abrk_null_ctrl {
  int32_t kind;
  int32_t rest_mask[ABRK_MAX_JOINTS]; /* RestingConfig.rest_indices                  */
  double kp;                          /* Joint kp (resting)                          */
  double kv;                          /* Damping kv / Joint kv                       */
  double rest_angles[ABRK_MAX_JOINTS];
} abrk_null_ctrl;

/* OSC constructor arguments (controllers/osc.py:53-118), passed through unchanged; the
 * derived constants (task_space_gains, lamb, sat_gain_*, scale_*) are formed inside
 * with the reference's expressions.                                                    */
typedef struct abrk_osc_params {
  double kp, ko, kv, ki;
  int32_t use_vmax;
  int32_t use_g;
  int32_t use_C;
  int32_t orientation_algorithm;
  double vmax[2];
  int32_t ctrlr_dof[6];
  int32_t ref_frame;            /* frame id of generate(ref_frame=...), osc.py:218       */
  int32_t n_null;
  double xyz_offset[3];         /* generate(xyz_offset=...), zeros == None               */
  abrk_null_ctrl null_ctrl[ABRK_MAX_NULL];
} abrk_osc_params;

/* OSC.generate (controllers/osc.py:217-320) for B independent states.
 *   q, dq [B,n]; target [B,6]; target_velocity [B,6] or NULL (== zeros, osc.py:239);
 *   integrated_error [B,6] in/out state, required iff ki != 0 (osc.py:81,262-264);
 *   u_null_ext [B,n] or NULL: extra secondary control signal already evaluated by the
 *     caller (any Python null controller), projected into the null space with the same
 *     filter as osc.py:315-318;
 *   u [B,n] out; training_signal [B,n] out or NULL (osc.py:297).
 * training_signal == NULL changes the LAST BITS of u on one family of laws: the six-row law (any ctrlr_dof beyond x,y,z
 * of the end effector) without optional inputs (no target_velocity / integrated_error / u_null_ext / null_ctrl) then
 * runs kernels that never form the training signal (`osc_kernel<.., NOTS = true>`: the gravity term joins the velocity
 * term before the factorisations instead of being subtracted from the finished sum).  Same law, same accuracy against
 * the reference (both forms are held to the same 1e-6 against its outputs: tests/test_gpu_parity.py
 * test_gpu_six_row_cases_without_training_signal), a different rounding order: u differs by ~1e-16 of its scale times
 * cond(Mx_inv).  For a given choice of NULL / non-NULL a row's bits depend on nothing else (batch size, position in the
 * batch, sharding).  Every other law returns the same bits either way.                                             */
int abrk_osc_generate_batch(int arm_id, int dtype, const abrk_osc_params* params, int64_t B,
                            const void* q, const void* dq, const void* target,
                            const void* target_velocity, void* integrated_error,
                            const void* u_null_ext, void* u, void* training_signal,
                            int device, void* stream);

/* OSC.generate AND the robot_config outputs it consumed, in one launch (one forward kinematics): besides u, any of
 *   Tx [B,3] = robot_config.Tx(ref_frame, q, x=xyz_offset)   (base_config.py:371-392)
 *   J  [B,6,n] = robot_config.J(ref_frame, q, x=xyz_offset)  (:249-270)
 *   M  [B,n,n] = robot_config.M(q)                            (:272-285)
 *   g  [B,n]   = robot_config.g(q)                            (:210-223)
 *   C  [B,n,n] = robot_config.C(q, dq)                        (:320-336)   } the velocity-dependent functions:
 *   dJ [B,6,n] = robot_config.dJ(ref_frame, q, dq, x=xyz_offset) (:225-247) } +288 B per UR5 row each
 * selected by `want` (ABRK_WANT_TX | ABRK_WANT_J | ABRK_WANT_M | ABRK_WANT_G | ABRK_WANT_C | ABRK_WANT_DJ; the other
 * fields of `out` are ignored), in the kernel's arithmetic type.  For callers that read those next to ctrlr.generate - adaptive terms on
 * training_signal, logging, a second controller on the same state (the consumers of osc.py:242-301) - and would
 * otherwise evaluate the kinematics twice.  840 B of algorithmic traffic per UR5 row in fp64: the HBM-bound form of
 * the path (SURVEY.md 8d "Mode F").  Everything else as abrk_osc_generate_batch.                              */
int abrk_osc_generate_full_batch(int arm_id, int dtype, const abrk_osc_params* params, int64_t B,
                                 const void* q, const void* dq, const void* target,
                                 const void* target_velocity, void* integrated_error,
                                 const void* u_null_ext, void* u, void* training_signal, uint32_t want,
                                 const abrk_dyn_out* out, int device, void* stream);

/* The WAVE-COOPERATIVE mapping of the same law (K = lanes_per_arm in {4, 8, 16} lanes per arm instance, frames /
 * Jacobian columns / M staged in LDS, abr_control_amd/csrc/abrk_coop.h): a measurement variant kept beside the
 * lane-per-arm kernels for the config-sized batch (profiles/round2/coop_ab.md).  Built-in ur5, fp64, the plain law of
 * BASELINE config 2 (x,y,z of the EE; no xyz_offset, null controllers, Coriolis term or integral term).      */
int abrk_osc_generate_coop_batch(int arm_id, int dtype, const abrk_osc_params* params, int64_t B, const void* q,
                                 const void* dq, const void* target, void* u, void* training_signal,
                                 int lanes_per_arm, int device, void* stream);

/* The same call over SEVERAL devices (BASELINE config 4: 2^20 rows over the 8 GPUs of a node): host arrays in, host
 * arrays out; the batch is cut into n_shards contiguous row ranges (sizes differing by at most one row), shard g is
 * evaluated on devices[g] (a device may appear more than once), each on a stream of its own, all kernels in flight before the first result is collected.  Rows are
 * independent: no exchange step, no collective.  Per-row state (integrated_error) stays with its shard.            */
int abrk_osc_generate_sharded(int arm_id, int dtype, const abrk_osc_params* params, int64_t B, const void* q,
                              const void* dq, const void* target, const void* target_velocity,
                              void* integrated_error, const void* u_null_ext, void* u, void* training_signal,
                              int n_shards, const int* devices);

/* The same control law (osc.py:244-318) on CALLER-SUPPLIED dynamics: keeps `OSC(robot_config=<any duck
 * type>)` working for configs whose arithmetic lives elsewhere (the reference's MujocoConfig,
 * abr_control/arms/mujoco_config.py:201-451: J/M/g/Tx/R read from mjData).  Per row, row-major:
 *   J [B,6,n] = robot_config.J(ref_frame,q,x); M [B,n,n] = robot_config.M(q);
 *   g [B,n] (iff use_g); Cdq [B,n] = C(q,dq)@dq (iff use_C); xyz [B,3] = robot_config.Tx(...) (iff any
 *   of ctrlr_dof[0:3]); R [B,3,3] = robot_config.R(...) (iff any of ctrlr_dof[3:6]);
 *   q [B,n] only for a fused RestingConfig; the remaining arguments as abrk_osc_generate_batch.
 * params->ref_frame / xyz_offset are ignored (already applied by whoever produced J, xyz, R).    */
int abrk_osc_law_batch(int n_joints, int dtype, const abrk_osc_params* params, int64_t B, const void* J,
                       const void* M, const void* g, const void* Cdq, const void* xyz, const void* R,
                       const void* q, const void* dq, const void* target, const void* target_velocity,
                       void* integrated_error, const void* u_null_ext, void* u, void* training_signal,
                       int device, void* stream);

/* The helper methods of OSC that callers (and the reference's own tests, controllers/tests/test_osc.py:12-140)
 * use directly.  The fused kernels above carry the same steps inline; these are their general forms.
 *
 * OSC._Mx (controllers/osc.py:120-147): task-space inertia Mx = (J M^-1 J^T)^-1, inverse while
 * |det| >= threshold, else pinv(rcond = 0.1 threshold).
 *   M [B,n,n] symmetric positive definite; J [B,k,n] = the k task rows OSC keeps (J[ctrlr_dof]), 1 <= k <= 6;
 *   Mx [B,k,k] out; M_inv [B,n,n] out or NULL.                                                    */
int abrk_osc_mx_batch(int n_joints, int k, int dtype, int64_t B, const void* M, const void* J, double threshold,
                      void* Mx, void* M_inv, int device, void* stream);
/* OSC._velocity_limiting (osc.py:198-215): u_task [B,6] -> out [B,6] with kp, ko, kv, vmax of params
 * (params->use_vmax must be set).                                                                 */
int abrk_osc_velocity_limiting_batch(int dtype, const abrk_osc_params* params, int64_t B, const void* u_task,
                                     void* out, int device, void* stream);
/* OSC._calc_orientation_forces (osc.py:149-196) from R [B,3,3] = robot_config.R(ref_frame, q) (ABRK_WANT_R of
 * abrk_dynamics_batch) and target_abg [B,3] (Euler angles, 'rxyz'); algorithm 0 or 1; out [B,3]. */
int abrk_osc_orientation_forces_batch(int algorithm, int dtype, int64_t B, const void* R, const void* target_abg,
                                      void* u_task_orientation, int device, void* stream);

/* The functions of abr_control/utils/transformations.py that the control path uses, B rows per call:
 *   ABRK_TF_QUAT_FROM_EULER_RXYZ / _SXYZ  a [B,3] angles          -> out [B,4] (w,x,y,z)   transformations.py:1096
 *   ABRK_TF_QUAT_FROM_MATRIX              a [B,3,3] rotations     -> out [B,4], w >= 0     :1192
 *   ABRK_TF_QUAT_MULTIPLY                 a = q1, b = q0 [B,4]    -> out [B,4]             :1274
 *   ABRK_TF_QUAT_CONJUGATE                a [B,4]                 -> out [B,4]             :1293
 *   ABRK_TF_UNIT_VECTOR4 / _VECTOR3       a [B,4] / [B,3]         -> out same shape        :1632
 *   ABRK_TF_EULER_MATRIX_RXYZ             a [B,3] angles          -> out [B,3,3]           :973
 * b is NULL except for the product.                                                               */
enum {
  ABRK_TF_QUAT_FROM_EULER_RXYZ = 0, ABRK_TF_QUAT_FROM_EULER_SXYZ = 1, ABRK_TF_QUAT_FROM_MATRIX = 2,
  ABRK_TF_QUAT_MULTIPLY = 3, ABRK_TF_QUAT_CONJUGATE = 4, ABRK_TF_UNIT_VECTOR4 = 5, ABRK_TF_UNIT_VECTOR3 = 6,
  ABRK_TF_EULER_MATRIX_RXYZ = 7
};
int abrk_transformations_batch(int op, int dtype, int64_t B, const void* a, const void* b, void* out, int device,
                               void* stream);

/* Launch plans for control loops that call the same law on the same device buffers every tick (the
 * shape of every example loop, examples/PyGame/force_osc_xy.py:57-78): all arguments of
 * abrk_osc_generate_batch are validated and converted ONCE; abrk_plan_launch then only enqueues the
 * kernel on the plan's stream (no pointer classification, no locks, no staging).  Every array must be a
 * device pointer.  Returns a plan id >= 0.                                                       */
int abrk_osc_plan_create(int arm_id, int dtype, const abrk_osc_params* params, int64_t B, const void* q,
                         const void* dq, const void* target, const void* target_velocity,
                         void* integrated_error, const void* u_null_ext, void* u, void* training_signal,
                         int device, void* stream);
/* General form: RECORD one control tick.  Between abrk_plan_begin and abrk_plan_end every abrk_*_batch call made by
 * this thread (dynamics, OSC, OSC law, Sliding, Joint / Damping / RestingConfig, AvoidJointLimits, Floating,
 * AvoidObstacles, inverse kinematics, the two-link plant step and rollout) is validated and converted as usual but
 * its kernel launch is kept in the plan instead of being enqueued - e.g. AvoidJointLimits and AvoidObstacles
 * accumulating into the buffer that the OSC call then takes as u_null_ext (osc.py:310-318) become ONE plan of
 * three kernels.  Each recorded call must pass device pointers only and the device and stream given to
 * abrk_plan_begin.  abrk_plan_end returns the plan id (>= 0); abrk_plan_abort drops the recording.  Ids of
 * destroyed plans are never valid again (generation-tagged), their slots and memory are recycled: a loop that
 * re-plans whenever gains, targets or buffers change can do so indefinitely; up to 4096 plans live at a time. */
int abrk_plan_begin(int device, void* stream);
int abrk_plan_end(void);
int abrk_plan_abort(void);
int abrk_plan_count(void); /* live plans */
int abrk_plan_launch(int plan);
/* `repeat` consecutive plain launches of the plan enqueued by ONE call (no per-launch crossing of the language
 * boundary): for a few tens of ticks this beats the fixed cost of a graph launch.                              */
int abrk_plan_launch_repeat(int plan, int repeat);
/* `repeat` consecutive launches of the plan as ONE hipGraph launch (captured on first use and cached per
 * repeat count): removes the per-launch host work and tightens the dependent-launch gaps of short kernels. */
int abrk_plan_launch_graph(int plan, int repeat);
int abrk_plan_destroy(int plan);

/* Sliding.generate (controllers/sliding.py:34-99), cartesian=True or False.
 *   target [B,3] (cartesian) or [B,n]; target_velocity / target_acc same shape or NULL
 *   (== 0); u [B,n] out; s [B,n] out or NULL (Sliding.s, sliding.py:89).              */
typedef struct abrk_sliding_params {
  double kd, lamb;
  int32_t cartesian;
  int32_t ref_frame;
  double offset[3];
} abrk_sliding_params;

int abrk_sliding_generate_batch(int arm_id, int dtype, const abrk_sliding_params* params,
                                int64_t B, const void* q, const void* dq, const void* target,
                                const void* target_velocity, const void* target_acc, void* u,
                                void* s, int device, void* stream);
/* Launch plan for Sliding.generate on fixed device buffers (see abrk_osc_plan_create; launched, replayed as a
 * hipGraph and destroyed by abrk_plan_launch / abrk_plan_launch_graph / abrk_plan_destroy).      */
int abrk_sliding_plan_create(int arm_id, int dtype, const abrk_sliding_params* params, int64_t B, const void* q,
                             const void* dq, const void* target, const void* target_velocity, const void* target_acc,
                             void* u, void* s, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * Closed loop on the device: the reference's examples alternate OSC.generate and
 * the two-link plant step ArmSim._step (abr_control/arms/twojoint/arm_sim.py:101-137) once per
 * millisecond of simulated time (examples/PyGame/force_osc_xy.py:57-78).  K1..K4 are the constants
 * ArmSim.__init__ derives (arm_sim.py:26-41); dt the Euler step.
 * --------------------------------------------------------------------------------- */
typedef struct abrk_twolink_plant {
  double K1, K2, K3, K4;
  double dt;
} abrk_twolink_plant;

/* ArmSim._step for B arms: (q, dq) [B,2] advanced in place by the torques u [B,2].            */
int abrk_twolink_step_batch(int dtype, const abrk_twolink_plant* plant, int64_t B, void* q, void* dq,
                            const void* u, int device, void* stream);

/* n_steps x { u = OSC.generate(q, dq, target); ArmSim._step(u) } in ONE launch, state in registers.
 *   arm_id: a two-joint arm; q, dq [B,2] in/out; target [B,6]; integrated_error [B,6] in/out (ki != 0);
 *   checkpoints (optional, every `every` steps, n_chk = n_steps / every):
 *   q_traj, dq_traj, u_traj [B, n_chk, 2] or NULL.                                              */
int abrk_osc_rollout_twolink_batch(int arm_id, int dtype, const abrk_osc_params* params,
                                   const abrk_twolink_plant* plant, int64_t B, int32_t n_steps, int32_t every,
                                   void* q, void* dq, const void* target, void* integrated_error,
                                   void* q_traj, void* dq_traj, void* u_traj, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * Rigid-body plant of ANY arm: forward dynamics and Euler steps on the device, so that a recorded plan
 * { control law; plant step } closes the loop without the host (abrk_plan_begin .. abrk_plan_end).
 *   ddq = M(q)^-1 (u - C(q,dq) dq - g(q))      with M, C, g as robot_config.M / .C / .g return them
 *   `substeps` times, h = dt / substeps, u held:  dq += ddq h;  q += dq h     (the update order of
 *   abr_control/arms/twojoint/arm_sim.py:131-132; arms/threejoint/arm_sim.py:93-94 takes dt/1e-5 such substeps)
 * gravity = 0 leaves g out.  These two entry points are the nominal plant; joint friction, joint limits, torque
 * saturation and external loads are the *_fx entry points below, a payload the *_payload ones, and contact of the end
 * effector with planes is abrk_contact_step_batch, whose torque arrives as tau_ext.
 * A row whose M has a non-positive Cholesky pivot is reported as ABRK_ESINGULAR exactly as by
 * abrk_osc_generate_batch: host arrays - the call returns the code; device pointers - the stream's next sync does.
 * --------------------------------------------------------------------------------- */
typedef struct abrk_plant_params {
  double dt;
  int32_t substeps; /* >= 1 */
  int32_t gravity;
} abrk_plant_params;

/* ddq [B,n] for B states (q, dq, u [B,n]); q, dq are not written.                                */
int abrk_forward_dynamics_batch(int arm_id, int dtype, int64_t B, const void* q, const void* dq,
                                const void* u, void* ddq, int device, void* stream);
/* (q, dq) [B,n] advanced in place by params->dt under the torques u [B,n] (host arrays: staged in and out). */
int abrk_plant_step_batch(int arm_id, int dtype, const abrk_plant_params* params, int64_t B,
                          void* q, void* dq, const void* u, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * The same plant with non-ideal effects, each of them optional.  Per substep of h = dt / substeps, with q and dq as
 * they are at the start of the substep (n = the arm's joint count):
 *   1. actuator saturation   tau_i  = clamp(u_i, -tau_max_i, +tau_max_i)
 *   2. loads and friction    tau_i += tau_ext[b, i]                             per-row joint-space disturbance [B,n]
 *                            tau_i += (J("EE", q)^T w[b])_i                     per-row wrench w = [fx fy fz mx my mz]
 *                                     [B,6] in the world frame, applied at the origin of the end-effector frame (the
 *                                     point Tx("EE", q) returns); J is the 6 x n Jacobian of robot_config.J("EE", q)
 *                            tau_i -= damping_i dq_i                            viscous friction
 *                            tau_i -= coulomb_i dq_i / sqrt(dq_i^2 + coulomb_vs^2)   Coulomb friction, smoothed
 *   3. dynamics              ddq = M^-1 (tau - C dq - g)                        gravity = 0 leaves g out
 *   4. integration           dq += ddq h;  q += dq h
 *   5. joint limits          q_i > q_max_i: q_i = q_max_i, and dq_i > 0 becomes -restitution dq_i; the mirror image at
 *                            q_min_i.  restitution = 0 leaves dq_i = 0.
 * abrk_forward_dynamics_fx_batch does steps 1-3 once and returns ddq.  An effect whose flag is off needs no infinity
 * in its fields (a zeroed struct will do: they only have to be finite); with fx, tau_ext and wrench all NULL, or with
 * every flag off, the results have the bits of the plain entry points.  One set of per-joint constants serves every
 * row.  ABRK_EINVAL (with a message): a negative damping or coulomb, coulomb_vs <= 0 with Coulomb friction on,
 * tau_max <= 0 with saturation on, q_min >= q_max with limits on, restitution outside [0, 1], a non-finite value
 * anywhere.  ABRK_ESINGULAR as above.  Recordable into a plan like every entry point: the kernel reads tau_ext and
 * wrench where a substep consumes them, so their contents may change between replays.
 * --------------------------------------------------------------------------------- */
enum {
  ABRK_FX_SATURATION = 1 << 0, /* tau_max                      */
  ABRK_FX_VISCOUS = 1 << 1,    /* damping                      */
  ABRK_FX_COULOMB = 1 << 2,    /* coulomb, coulomb_vs          */
  ABRK_FX_LIMITS = 1 << 3      /* q_min, q_max, restitution    */
};
typedef struct abrk_plant_effects {
  uint32_t flags; /* ABRK_FX_* */
  double damping[ABRK_MAX_JOINTS]; /* >= 0 */
  double coulomb[ABRK_MAX_JOINTS]; /* >= 0 */
  double coulomb_vs;               /* > 0: the speed below which Coulomb friction fades to zero */
  double tau_max[ABRK_MAX_JOINTS]; /* > 0 */
  double q_min[ABRK_MAX_JOINTS];
  double q_max[ABRK_MAX_JOINTS];   /* > q_min */
  double restitution;              /* in [0, 1] */
} abrk_plant_effects;

/* fx, tau_ext [B,n] and wrench [B,6] may each be NULL */
int abrk_forward_dynamics_fx_batch(int arm_id, int dtype, const abrk_plant_effects* fx, int64_t B, const void* q,
                                   const void* dq, const void* u, const void* tau_ext, const void* wrench, void* ddq,
                                   int device, void* stream);
int abrk_plant_step_fx_batch(int arm_id, int dtype, const abrk_plant_params* params, const abrk_plant_effects* fx,
                             int64_t B, void* q, void* dq, const void* u, const void* tau_ext, const void* wrench,
                             int device, void* stream);

/* ---------------------------------------------------------------------------------
 * The same plant carrying a payload that differs from row to row: a point mass m[b] >= 0 fixed to the end-effector
 * link at offset r[b] from the origin of the EE frame, in that frame's coordinates (the x of
 * robot_config.Tx("EE", q, x=r)).  Row b is the arm with one more link of _M_LINKS = diag(m, m, m, 0, 0, 0) whose centre
 * of mass is that point.  `payload` is [B,4] of `dtype`: m, rx, ry, rz.  With Jp = J("EE", q, x=r)[:3] and
 * dJp = dJ("EE", q, dq, x=r)[:3], step 3 of the sequence above becomes
 *   ddq = (M + m Jp^T Jp)^-1 (tau - C dq - m Jp^T (dJp dq) - g - Jp^T m (0, 0, -9.81)^T)
 * (gravity = 0 leaves both gravity terms out); steps 1, 2, 4 and 5 are unchanged, q and dq are those of the substep's
 * start, and ABRK_ESINGULAR looks at the pivots of the augmented matrix.  The payload has no rotational inertia.
 * fx, tau_ext and wrench stay optional.  payload == NULL forwards to the *_fx entry point: the same bits.
 * A HOST payload array is validated before it is staged: a negative or non-finite m, or a non-finite r, is
 * ABRK_EINVAL with the row in the message.  A DEVICE array is NOT validated: the kernel reads it with ordinary
 * per-lane loads at every launch, so a recorded plan picks up a mass rewritten between replays, and what a bad value
 * does there is the caller's business (a negative m can make the augmented matrix indefinite: ABRK_ESINGULAR or NaN).
 * --------------------------------------------------------------------------------- */
int abrk_forward_dynamics_payload_batch(int arm_id, int dtype, const abrk_plant_effects* fx, int64_t B, const void* q,
                                        const void* dq, const void* u, const void* tau_ext, const void* wrench,
                                        const void* payload, void* ddq, int device, void* stream);
int abrk_plant_step_payload_batch(int arm_id, int dtype, const abrk_plant_params* params, const abrk_plant_effects* fx,
                                  int64_t B, void* q, void* dq, const void* u, const void* tau_ext, const void* wrench,
                                  const void* payload, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * End-effector contact with per-row planes, and a force report.  One kernel per tick that WRITES the plant's
 * joint-space disturbance: record { law; abrk_contact_step_batch -> tau; abrk_plant_step_fx_batch(tau_ext = tau) } and
 * the arm can press on a table, slide along it and lift off inside a replayed plan.  The plant kernels are untouched.
 *
 * Row b has the contact point p = Tx(frame, q, x = off) - `frame` any frame of robot_config.Tx, `off` a tool offset in
 * that frame, shared by the batch - with a sphere tip of radius rho around it, and S half-spaces of its own,
 * `surface` [B,S,8] of `dtype` = nx, ny, nz, d, k, c, mu, rho; the free side is n.x > d.  With Jp = J(frame, q, x = off)[:3]
 * and v = Jp dq each surface contributes
 *   delta = d + rho - n.p                   penetration; delta <= 0: nothing
 *   vn    = n.v                             > 0 leaving
 *   fn    = max(0, k delta - c vn)          Kelvin-Voigt, no adhesion
 *   vt    = v - vn n
 *   f     = fn n - mu fn vt / sqrt(|vt|^2 + vs^2)       Coulomb friction smoothed like coulomb_vs of abrk_plant_effects
 * and with F the sum of f over the row's surfaces
 *   tau_c = Jp^T F                          written to tau [B,n], or added to it (accumulate != 0)
 * n is used as given (the kernel does not normalise it).  Columns of Jp of joints past `frame` are zero, as in
 * robot_config.J, so those entries of tau_c are exact zeros; a row clear of every surface gets tau_c = 0 exactly.
 * `report` [B,8] (optional) is what a wrist force sensor and a logger want: F in the world frame [3]; R(frame, q)^T F,
 * the same force in the frame's own coordinates [3]; the deepest delta of the row (negative: clear of every surface);
 * the number of surfaces with delta > 0.
 *
 * LIMITATION: the force is evaluated ONCE per tick from the state at the start of the tick, and the plant holds it over
 * its substeps like u - the price of leaving the plant kernels alone.  The contact spring is therefore sampled with the
 * TICK h = dt, whatever `substeps` is.  With m_eff = 1 / (n^T Jp M^-1 Jp^T n) the arm's effective mass along the normal,
 * A = k h^2 / m_eff and D = c h / m_eff, the linearised contact is stable
 *   substeps = 1 (the plant's dq += ddq h; q += dq h):   A + 2 D < 4
 *   many substeps (a force held over an exact step):     A / 2 < D < 2, i.e. k h / 2 < c < 2 m_eff / h
 * so more substeps do NOT stiffen the contact, and with them an undamped plane (c = 0) gains energy at every bounce.
 * Keep A below about 1 and c above k h / 2 (k = 1e4 N/m, h = 1 ms: m_eff > 0.01 kg, c > 5 N s/m).
 * More than one contact point: one call per point, the later ones with accumulate.
 *
 * Recordable into a plan like every entry point: `surface` is read with ordinary loads at every launch, so a plane
 * moved or softened between two replays takes effect.  A HOST surface array is validated before it is staged -
 * | |n| - 1 | > 1e-6, a negative k, c, mu or rho, anything non-finite: ABRK_EINVAL with the row and the surface in the
 * message.  A DEVICE array is NOT validated, as with the payload.  ABRK_EINVAL also for params: a frame outside the arm,
 * a non-finite off, n_surfaces outside 1..ABRK_CONTACT_MAX_SURFACES, vs <= 0.
 * --------------------------------------------------------------------------------- */
#define ABRK_CONTACT_MAX_SURFACES 4
typedef struct abrk_contact_params {
  int32_t frame;        /* link_i -> 2i, joint_i -> 2i+1, EE -> 2N+1: the loop recorder's encoding */
  double off[3];
  int32_t n_surfaces;   /* 1..ABRK_CONTACT_MAX_SURFACES */
  double vs;            /* > 0 */
  int32_t accumulate;
} abrk_contact_params;

int abrk_contact_step_batch(int arm_id, int dtype, const abrk_contact_params* params, int64_t B, const void* q,
                            const void* dq, const void* surface, void* tau, void* report /* or NULL */, int device,
                            void* stream);

/* ---------------------------------------------------------------------------------
 * Force-controlled contact: Khatib's unified motion/force law for the point of abrk_contact_step_batch.  One kernel per
 * tick that writes u: record { abrk_force_control_batch(force = the contact report of the previous tick) -> u;
 * abrk_contact_step_batch -> tau, report; abrk_plant_step_fx_batch(u, tau_ext = tau) } and an arm approaches a surface,
 * presses on it with a commanded force and moves along it inside a replayed plan.
 *
 * Row b has the point p = Tx(frame, q, x = off), Jp = J(frame, q, x = off)[:3], v = Jp dq, and M, g as robot_config
 * returns them.  Its inputs: `target` [B,6] as abrk_osc_generate_batch takes it, of which only x_d = columns 0..2 are
 * read; `target_velocity` [B,6] or NULL, v_d = columns 0..2 (NULL: 0); `cmd` [B,4] = nx, ny, nz, f_des - n the surface
 * normal, a unit vector in the world frame that points INTO FREE SPACE, f_des >= 0 the force the tip shall press with
 * (N); `force` [B, force_ld], columns 0..2 the sensed force F ON the tip in the world frame (force_ld = 8: a contact
 * `report` array as it is); `integ` [B], the force integral, read and written.
 *   A    = Jp M^-1 Jp^T
 *   Mx   = inv(A) where det(A) > 1e-3, else pinv(A, rcond = 1e-4)          the rule of the task-space Floating law
 *   a    = kp (x_d - p) + kv (v_d - v);   a_n = n.a;   v_n = n.v;   f_m = n.F
 *   in contact (f_m > f_touch):
 *          e   = f_des - f_m                                                > 0: pressing too lightly
 *          I'  = clamp(I + ki e dt, -i_max, +i_max)
 *          F_c = Mx (a - a_n n - kvf v_n n) - (f_des + kf e + I') n         pushes along -n, into the surface
 *   free (otherwise):
 *          I'  = 0
 *          F_c = Mx (a - a_n n + kv (-v_app - v_n) n)                       approaches along -n at v_app
 *   u    = Jp^T F_c - [use_g] g(q) - kv_null (M dq - Jp^T Mx v)
 *   integ <- I';  u written to u [B,n], or added to it (accumulate != 0)
 * The last term of u is the Damping law, -kv_null M dq, passed through OSC's null-space filter I - Jp^T Mx Jp M^-1.
 * use_g has OSC's sign (u -= g).  n is used as given (the kernel does not normalise it).  The two modes are a per-lane
 * select: a row's mode may differ from its neighbour's and change from tick to tick.
 * NOT MODELLED: orientation (no rotational rows: the wrist is left to the null-space damping); more than one
 * constrained direction; Coriolis compensation; a moment about the point.
 *
 * Recordable into a plan like every entry point, host or device pointers, re-entrant per stream.  `cmd` is read with
 * ordinary loads at every launch, so a normal or a desired force rewritten between two replays takes effect.  A HOST cmd
 * array is validated before it is staged - | |n| - 1 | > 1e-6, f_des < 0, anything non-finite: ABRK_EINVAL with the row
 * in the message.  A DEVICE array is NOT validated, as with the payload and the contact surfaces.  ABRK_EINVAL also for
 * params: a frame outside the arm, a non-finite off, a negative or non-finite gain, f_touch, v_app, i_max or kv_null,
 * dt <= 0, force_ld < 3.  ABRK_ESINGULAR for a non-positive Cholesky pivot of M, as in the other laws.
 * --------------------------------------------------------------------------------- */
typedef struct abrk_force_params {
  int32_t frame;        /* as abrk_contact_params */
  double off[3];
  double kp, kv;        /* motion gains (>= 0) */
  double kf, ki, i_max; /* force PI, anti-windup clamp (>= 0) */
  double kvf;           /* damping along n while in contact (>= 0) */
  double f_touch;       /* >= 0: in contact where n.F exceeds it */
  double v_app;         /* >= 0: approach speed along -n while free */
  double kv_null;       /* >= 0; 0 switches the null-space damping off */
  double dt;            /* > 0 */
  int32_t use_g, accumulate, force_ld; /* force_ld >= 3 */
} abrk_force_params;

int abrk_force_control_batch(int arm_id, int dtype, const abrk_force_params* params, int64_t B, const void* q,
                             const void* dq, const void* target, const void* target_velocity /* or NULL */,
                             const void* cmd, const void* force, void* integ, void* u, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * Whole-arm contact: the arm's link segments as capsules against per-row sphere obstacles.  One kernel per tick, in the
 * shape of abrk_contact_step_batch, that WRITES the plant's joint-space disturbance: record { law;
 * abrk_link_contact_step_batch -> tau; abrk_plant_step_fx_batch(tau_ext = tau) } and an elbow that passes through a
 * sphere is pushed out of it inside a replayed plan.  The spheres are those of AvoidObstacles
 * (abrk_avoid_obstacles_generate_batch), so a loop can show whether avoidance kept the arm clear.
 *
 * Segments.  Segment i (0 <= i < N) runs from a_i, the origin of joint_i, to b_i, the origin of joint_{i+1}; for the
 * last segment b_i is the origin of EE.  These are the segments of avoid_obstacles.py:61-68.  Segment i is a body of
 * link i+1: joints 0..i move it.  It has a radius r_i = link_radius[i], the same for every row; r_i < 0 switches the
 * segment off.  A segment with |b-a|^2 == 0 is skipped.
 * Obstacles.  Row b has K spheres of its own (1 <= K <= ABRK_LINK_CONTACT_MAX_OBSTACLES), `obstacle` [B,K,7] of `dtype`
 * = cx, cy, cz, R, k, c, mu; the spheres are at rest; the first four columns are the AvoidObstacles obstacle.
 * Per pair, for every (obstacle, segment), obstacle-major and segment-minor:
 *   t     = clamp((c - a).(b - a) / |b - a|^2, 0, 1)        x = a + t (b - a)   (x = b exactly at t = 1)
 *   e     = x - c;  d = |e|;  delta = R + r_i - d            penetration; delta <= 0: nothing
 *   n     = e / d                                            from the obstacle to the link; d == 0: n = 0 (counted, no force)
 *   v     = Jx dq,  Jx = J("link{i+1}", q, x = the material point at x)[:3]     (columns j > i are zero)
 *   vn    = n.v;  fn = max(0, k delta - c vn)                Kelvin-Voigt, no adhesion - the law of the contact section
 *   vt    = v - vn n;  f = fn n - mu fn vt / sqrt(|vt|^2 + vs^2)
 *   tau_c += Jx^T f                                          written to tau [B,n], or added to it (accumulate != 0)
 * The force acts at the axis point x, as the tip force of abrk_contact_step_batch acts at the sphere's centre; the moment
 * r_i n x f of the friction about the axis is NOT MODELLED, nor are planes against capsules, link against link, or a
 * velocity of the obstacles.  tau entries of joints past the segment get exact zeros from that pair.  A row with no
 * pushing pair gets tau_c = 0 exactly; with accumulate its tau is left untouched to the bit.  The force is that of the
 * start of the tick: the stability note of the contact section, on k h^2 / m_eff, applies unchanged.
 * `report` [B,8] (optional): F = the sum of f in the world frame [3]; the deepest delta over the active pairs (negative:
 * clear of everything; the lowest finite value where no pair is active); the number of pairs with delta > 0; the segment index, the
 * obstacle index and the t of the deepest pair (the first in loop order on a tie).
 *
 * Recordable into a plan like every entry point, host or device pointers.  `obstacle` is read with ordinary loads at
 * every launch, so an obstacle moved between two replays takes effect.  A HOST obstacle array is validated before it is
 * staged - anything non-finite, R <= 0, a negative k, c or mu: ABRK_EINVAL with the row and the obstacle in the message.
 * A DEVICE array is NOT validated, as with the surfaces.  ABRK_EINVAL also for params: n_obstacles outside
 * 1..ABRK_LINK_CONTACT_MAX_OBSTACLES, vs <= 0, a non-finite radius among the first N, every segment off.
 * --------------------------------------------------------------------------------- */
#define ABRK_LINK_CONTACT_MAX_OBSTACLES 8
typedef struct abrk_link_contact_params {
  int32_t n_obstacles;    /* 1..ABRK_LINK_CONTACT_MAX_OBSTACLES */
  double link_radius[7];  /* the first N are used; < 0: that segment is off */
  double vs;              /* > 0 */
  int32_t accumulate;
} abrk_link_contact_params;

int abrk_link_contact_step_batch(int arm_id, int dtype, const abrk_link_contact_params* params, int64_t B, const void* q,
                                 const void* dq, const void* obstacle, void* tau, void* report /* or NULL */, int device,
                                 void* stream);

/* ---------------------------------------------------------------------------------
 * Iterative inverse kinematics: InverseKinematics.generate_path
 * (abr_control/controllers/path_planners/inverse_kinematics.py:28-135) for B independent paths, all
 * n_timesteps iterations of a path inside one kernel (each iteration: Tx, J, quaternion of the EE, two
 * pseudo-inverses).  max_dx / max_dr / max_dq are the constructor values (per second); they are scaled by
 * dt exactly as generate_path does.  method 1: resolved motion, 2: damped least squares, 3: position with
 * orientation in its null space (the reference default).  target [B,6] = xyz + Euler angles 'sxyz'.
 * position [B,n] start joint angles; position_path, velocity_path [B, n_timesteps, n] out.
 * --------------------------------------------------------------------------------- */
typedef struct abrk_ik_params {
  double max_dx, max_dr, max_dq, dt;
  int32_t n_timesteps;
  int32_t method;
} abrk_ik_params;

int abrk_ik_generate_path_batch(int arm_id, int dtype, const abrk_ik_params* params, int64_t B,
                                const void* position, const void* target, void* position_path,
                                void* velocity_path, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * PathPlanner.generate_path (abr_control/controllers/path_planners/path_planner.py:99-452) for B independent
 * movements, fp64 only: position profile warped onto start -> target, velocity-limited stepping along it, SLERP
 * orientation (orientation.py:157-198, utils/transformations.py:1096-1147, 1333-1369, 1033-1093), np.gradient
 * velocities.  What depends on the caller's profile OBJECTS is evaluated once per call by the caller (in this
 * package: the Python classes' own step() / generate()) and handed over as ONE packed table of doubles plus an
 * offsets array; what depends on a row runs on the device.
 *   table   [table_len] doubles, host or device
 *   offsets [2 + 4 n_candidates] int64, HOST-readable (validated against table_len on every call):
 *     offsets[0]              S x 3 samples pos_profile.step(linspace(0, 1, S))            (path_planner.py:197-205)
 *     offsets[1]              n_candidates x 3: max_v_k, starting_dist_k, ending_dist_k, for max_v_k = max_velocity
 *                             - 0.1 k formed by repeated subtraction (:242-302; np.sum(profile * dt), :255, :269)
 *     offsets[2 + 4k], [+1]   np.cumsum(starting_vel_profile_k * dt) and its length        (:249-251, :316)
 *     offsets[2 + 4k + 2], [+3]  np.cumsum(ending_vel_profile_k * dt) and its length       (:257-265)
 *   axes: firstaxis | parity << 2 | repetition << 3 | frame << 4 of transformations.py:1565-1590 ('rxyz' = 22,
 *   'sxyz' = 0); width: 6 (position, velocity) or 12 (+ Euler angles, their np.gradient).
 * Two calls, because the output is sized by the first one's result:
 *   abrk_path_plan_batch: start, target [B,3] -> n_timesteps [B] int32 (0: the row has no path), rowplan [B,2] int32
 *     (candidate taken, constant-speed steps), dist_steps [B, n_samples] doubles (cumulative chord lengths, :215).
 *     A row without a path - start == target, a movement exactly towards -(1,1,1)/sqrt(3) (align_vectors, :75-97,
 *     divides by zero there), every candidate rejected (the reference's ValueError, :245), fewer than the 2 steps
 *     np.gradient needs - is reported as ABRK_EPATH the way ABRK_ESINGULAR is.
 *   abrk_path_fill_batch: the same table and rows + the three arrays above -> path [B, t_max, width]; row b holds
 *     its path in [:n_timesteps[b]] and its last point after that (what PathPlanner.next() keeps returning, :454-464).
 *     t_max >= max(n_timesteps) for all of it; a row with n_timesteps 0 or n_timesteps > t_max is not written at all
 *     (no column of it, no truncated path; `path` is an output only, so into a HOST array such a row comes back
 *     unspecified - a device array keeps what it held).  start_/target_orientation [B,3]: width 12.
 * Neither can be recorded into a plan.
 * --------------------------------------------------------------------------------- */
typedef struct abrk_path_params {
  double dt;            /* vel_profile.dt */
  int32_t n_samples;    /* S >= 2 */
  int32_t n_candidates; /* >= 1 */
  int32_t axes;
  int32_t width;
  int64_t table_len;
} abrk_path_params;

int abrk_path_plan_batch(const abrk_path_params* params, const void* table, const int64_t* offsets, int64_t B,
                         const void* start, const void* target, void* n_timesteps, void* rowplan, void* dist_steps,
                         int device, void* stream);
int abrk_path_fill_batch(const abrk_path_params* params, const void* table, const int64_t* offsets, int64_t B,
                         int32_t t_max, const void* start, const void* target, const void* start_orientation,
                         const void* target_orientation, const void* n_timesteps, const void* rowplan,
                         const void* dist_steps, void* path, int device, void* stream);
/* PathPlanner.next() (path_planner.py:454-464) for B rows, as the feed of a recorded loop: with n = counter[b]
 * (clamped into the row's path), target[b] = path[b, n, (0:3, 6:9)], target_velocity[b] = path[b, n, (3:6, 9:12)]
 * - the layout OSC.generate takes (osc.py:217-239) - and counter[b] = min(n + 1, n_timesteps[b] - 1).  A 6-wide path
 * leaves the orientation columns of both outputs as they are.  path is fp64 [B, t_max, width]; `dtype` is the type of
 * target / target_velocity [B,6] (NULL: not written): an fp32 loop is fed from the fp64 path.  counter, n_timesteps
 * [B] int32.  Recordable: { path_next; OSC; plant step } replayed K times tracks K path points without the host. */
int abrk_path_next_batch(int dtype, int64_t B, int32_t t_max, int32_t width, const void* path,
                         const void* n_timesteps, void* counter, void* target, void* target_velocity, int device,
                         void* stream);

/* ---------------------------------------------------------------------------------
 * The adaptive signal of a recorded loop: what the reference's controllers/signals/DynamicsAdaptation
 * (abr_control/controllers/signals/dynamics_adaptation.py) builds out of Nengo - ensembles of LIF neurons over the
 * scaled joint state whose decoders learn by PES from the controller's training_signal - for B independent rows, one
 * tick per call.  N = n_neurons_total neurons (all ensembles side by side), D = n_input, O = n_output.
 * Shared by the rows, of `dtype`: enc [N,D] (unit rows), gain [N], bias [N], shift [D], scale [D].
 * Per row, of `dtype`, read and written by every call (abrk_adapt_state): x_f [B,D], e_f [B,O], v [B,N], ref [B,N],
 * a_f [B,N], W [B,O,N] (neuron index contiguous), out_f [B,O].  Zero filling all seven restarts the rows.
 * With a(tau) = 1 - exp(-dt / tau), a(0) = 1, one tick of row b is
 *   1  x = (concat(in0[b], in1[b]) - shift) * scale;  x_f += a(tau_input) (x - x_f)     in0 [B,w0], in1 [B,w1] or NULL
 *   2  e_f += a(tau_training) (training[b] - e_f)                                          training [B,O]
 *   3  J_i = gain_i (enc_i . x_f) + bias_i, then per neuron
 *        ABRK_ADAPT_LIF       ref -= dt;  d = clip(dt - ref, 0, dt);  v -= (J - v) expm1(-d / tau_rc);  on v > 1:
 *                             t_s = dt + tau_rc log1p(-(v - 1) / (J - 1)), v = 0, ref = tau_ref + t_s, s = 1 / dt;
 *                             otherwise v = max(v, 0), s = 0
 *        ABRK_ADAPT_LIF_RATE  s = 1 / (tau_ref + tau_rc log1p(1 / (J - 1))) for J > 1, else 0   (v, ref are not touched
 *                             and may be NULL)
 *   4  y_o = sum_i W[o,i] s_i                          (the weights from before this tick's update)
 *   5  out_f += a(tau_output) (y - out_f);  out[b] = out_f;  u_add[b] += out_f              out, u_add [B,O]; u_add or NULL
 *   6  a_f,i += a(ABRK_ADAPT_TAU_PRE) (s_i - a_f,i)
 *   7  W[o,i] += (pes_learning_rate dt / n_per_ensemble) e_f[o] a_f,i
 * (the reference feeds -training_signal as the error and PES subtracts: the two signs cancel).  These are Nengo's published
 * Lowpass, LIF / LIFRate and PES operators; their order within a tick is this library's, and agreement with Nengo's
 * simulator to the tick is not claimed.
 * Goes through the staging of every *_batch call (host arrays work for one-off calls) and is recorded between
 * abrk_plan_begin and abrk_plan_end: in { law(training_signal = ts); adapt(q, dq, ts, u_add = u); plant step } the state
 * lives in device memory and advances at every replay.
 * ABRK_EINVAL: dtype, neuron_type, B < 0, n_input outside 1..ABRK_ADAPT_MAX_INPUT, n_output outside
 * 1..ABRK_ADAPT_MAX_OUTPUT, n_neurons_total < 1, n_per_ensemble < 1, w0 + w1 != n_input (w1 != 0 with in1 NULL), a dt, tau_rc
 * that is not positive and finite, another time constant or pes_learning_rate that is negative or not finite, a NULL
 * required array.
 * --------------------------------------------------------------------------------- */
#define ABRK_ADAPT_LIF 0
#define ABRK_ADAPT_LIF_RATE 1
#define ABRK_ADAPT_MAX_INPUT 64
#define ABRK_ADAPT_MAX_OUTPUT 16
#define ABRK_ADAPT_TAU_PRE 0.005
typedef struct abrk_adapt_params {
  int32_t n_input;         /* D */
  int32_t n_output;        /* O */
  int32_t n_neurons_total; /* N = n_ensembles * n_per_ensemble */
  int32_t n_per_ensemble;
  int32_t neuron_type;     /* ABRK_ADAPT_LIF | ABRK_ADAPT_LIF_RATE */
  double dt;
  double tau_input, tau_training, tau_output; /* 0: no filter */
  double tau_rc, tau_ref;                     /* Nengo's LIF defaults: 0.02, 0.002 */
  double pes_learning_rate;
} abrk_adapt_params;
typedef struct abrk_adapt_state {
  void *x_f, *e_f, *v, *ref, *a_f, *W, *out_f;
} abrk_adapt_state;
int abrk_adapt_step_batch(int dtype, const abrk_adapt_params* params, int64_t B, const void* enc, const void* gain,
                          const void* bias, const void* shift, const void* scale, const void* in0, int32_t w0,
                          const void* in1, int32_t w1, const void* training, const abrk_adapt_state* state, void* out,
                          void* u_add, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * The measurement and actuation channel of a recorded loop: a [B, W] signal passed through bias, noise, quantisation,
 * latency and an optional filtered difference, one tick per call.  The same call serves the sensing side (q, dq -> what
 * the law reads) and the actuation side (u -> what the plant receives).  All arrays are of `dtype` but counter (int32).
 * With t = max(counter[b], 0), d = delay, x = concat(in0[b], in1[b])[c] (in0 [B,w0], in1 [B,w1] or NULL, w0 + w1 = width),
 * one tick of row b, column c is
 *   1  v = fma(sigma[c], n, x + bias[c])               n: the standard normal below.  sigma[c] == 0: no number is drawn
 *                                                      and v = x + bias[c]
 *   2  resolution[c] > 0: v = rint(v * inv_res[c]) * resolution[c]        inv_res = 1 / resolution formed in double and
 *                                                      rounded to `dtype`; rint rounds half to even
 *   3  d > 0: ring[t % (d + 1), b, c] = v, then out = ring[max(t - d, 0) % (d + 1), b, c]      ring [d + 1, B, width],
 *      time-major: a tick's rows are contiguous.  For t < d that is the sample of tick 0: the channel holds its first
 *      sample.  d == 0: out = v; the ring is neither read nor written and may be NULL
 *   4  out -> out0[b, c] or out1[b, c - w0], mirroring the inputs
 *   5  only when dy [B,width] is given: at t == 0 g = 0 and d_f = 0, otherwise g = (out - prev[b,c]) / dt (a product with
 *      1 / dt) and d_f = fma(a, g - d_f, d_f) with a = 1 - exp(-dt / tau_diff), a = 1 for tau_diff = 0 (formed in double);
 *      dy[b,c] = d_f, prev[b,c] = out                   prev, d_f [B,width]
 *   6  counter[b] = t + 1
 * Zero filling counter - of all rows or of some - restarts them; nothing else needs clearing, since tick 0 reads nothing
 * it has not written.  With sigma = bias = resolution = 0, delay = 0 and no dy the call returns x bit for bit.
 * n is computed in fp64 whatever `dtype` is and rounded to `dtype` at the fma (fp32 sees the same realisation):
 * Philox4x32-10 - multipliers 0xD2511F53 on word 0 and 0xCD9E8D57 on word 2, one round [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2),
 * hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)], key increments 0x9E3779B9 and 0xBB67AE85 - with the key (seed low 32, seed high 32)
 * and the counter (r low 32, r high 32, t, c), r = b + row_offset as a 64-bit value.  From the output words w0..w3:
 * k1 = (w0 >> 5) 2^26 + (w1 >> 6), k2 likewise from w2, w3; u1 = (k1 + 1) 2^-53 in (0, 1], u2 = k2 2^-53;
 * n = sqrt(-2 ln u1) cos(2 pi u2).  n depends on (seed, global row, tick, column) alone: a row's bits do not depend on
 * the batch it arrives in, and a shard continues the numbering through row_offset.
 * Goes through the staging of every *_batch call (host arrays work for one-off calls) and is recorded between
 * abrk_plan_begin and abrk_plan_end: in { channel(q, dq -> q_meas, dq_meas); law on q_meas, dq_meas; channel(u -> u_act);
 * plant step on u_act } the state lives in device memory and advances at every replay.
 * ABRK_EINVAL: dtype; B < 0; width outside 1..ABRK_CHANNEL_MAX_WIDTH; delay outside 0..ABRK_CHANNEL_MAX_DELAY; w0 + w1 !=
 * width; w1 != 0 with in1 or out1 NULL; a sigma or resolution that is negative or not finite, a bias that is not finite;
 * dt <= 0; with dy, a tau_diff that is negative or not finite; NULL params, in0, out0, state or counter; NULL ring with
 * delay > 0; NULL prev or d_f with dy.  B == 0 returns before the device is touched.
 * --------------------------------------------------------------------------------- */
#define ABRK_CHANNEL_MAX_WIDTH 16
#define ABRK_CHANNEL_MAX_DELAY 4096
typedef struct abrk_channel_params {
  int32_t width;      /* W, 1..ABRK_CHANNEL_MAX_WIDTH */
  int32_t delay;      /* whole ticks, 0..ABRK_CHANNEL_MAX_DELAY */
  uint64_t seed;
  int64_t row_offset; /* global number of row 0 */
  double dt;
  double tau_diff;    /* low-pass of the difference; 0: none */
  double bias[ABRK_CHANNEL_MAX_WIDTH];
  double sigma[ABRK_CHANNEL_MAX_WIDTH];      /* noise standard deviation; 0: none */
  double resolution[ABRK_CHANNEL_MAX_WIDTH]; /* quantisation step; 0: none */
} abrk_channel_params;
typedef struct abrk_channel_state {
  void* counter;           /* int32 [B] */
  void *ring, *prev, *d_f; /* [delay + 1, B, width], [B,width], [B,width] */
} abrk_channel_state;
int abrk_channel_step_batch(int dtype, const abrk_channel_params* params, int64_t B, const void* in0, int32_t w0,
                            const void* in1, int32_t w1, void* out0, void* out1, void* dy,
                            const abrk_channel_state* state, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * The output side of a recorded loop: what every closed-loop example of the reference keeps in ee_track / target_track /
 * q_track lists and reduces with np.linalg.norm(ee - target), kept on the device.  One call = one tick of every row.  With
 * t = counter[b]:
 *   xyz = Tx(frame, x_off) of q[b] (as abrk_dynamics_batch);  err = |target[b, 0:3] - xyz| in `dtype`
 *   history (may be NULL): if t % every == 0 and slot = t / every < capacity, the selected columns go to history[slot, b, :].
 *     Columns (ABRK_TR_*, abrk_types.h) keep the order q, dq, u [n], target [6], xyz [3], err [1]; W = the sum of the selected
 *     widths.  [capacity, B, W] of `dtype`, time-major: a tick's rows are contiguous.  Slots past `capacity` are dropped (no
 *     ring buffer); slots never written keep what the caller filled them with.
 *   stats (may be NULL) [B,4] ALWAYS fp64: err_last, err_max, err_min, err_sumsq - assigned at t == 0, combined after it
 *     (max, min, += err^2).  settle [B] int32 (required with stats): err <= tol ? (settle ? settle : t + 1) : 0, i.e. 0 =
 *     outside the tolerance now, k > 0 = inside since tick k - 1.
 *   counter[b] = t + 1.  The tick is per row and lives in device memory (a graph replay repeats identical arguments): zero
 *     filling counter, settle and stats - of all rows or of some - restarts them.
 * q is read for xyz, err, stats and its own column; dq / u only for their columns; target for err, stats and its column: a
 * source nothing selected needs may be NULL.  Goes through the staging of every *_batch call (host arrays work for one-off
 * calls) and is recorded between abrk_plan_begin and abrk_plan_end: { path_next; law; plant step; loop_trace } replayed K
 * times returns K ticks of trajectory and statistics with no host round trip.
 * ABRK_EINVAL: dtype, B < 0, every < 1, a history with capacity < 1 or with an empty / unknown column mask, a NULL array
 * that is needed, neither history nor stats, a frame id outside 0..2n+1, a non-finite tol or x_off.
 * --------------------------------------------------------------------------------- */
typedef struct abrk_trace_params {
  int32_t frame;    /* link_i -> 2i, joint_i -> 2i+1, EE -> 2n+1 */
  double x_off[3];
  int32_t every;    /* >= 1: history keeps every `every`-th tick (statistics see every tick) */
  int32_t capacity; /* history slots */
  uint32_t columns; /* ABRK_TR_* */
  double tol;
} abrk_trace_params;
int abrk_loop_trace_batch(int arm_id, int dtype, const abrk_trace_params* params, int64_t B, const void* q,
                          const void* dq, const void* u, const void* target, void* counter, void* history, void* stats,
                          void* settle, int device, void* stream);

/* Joint.generate (controllers/joint.py:104-131) / Damping / RestingConfig standalone.
 *   ctrl.kind == ABRK_NULL_DAMPING: u = M (-kv dq)            (damping.py:31-32)
 *   ctrl.kind == ABRK_NULL_RESTING: RestingConfig.generate     (resting_config.py:33-42)
 *   ctrl.kind == 0: Joint.generate with target [B,n], target_velocity [B,n] or NULL,
 *                   account_for_gravity as given.                                       */
int abrk_joint_generate_batch(int arm_id, int dtype, const abrk_null_ctrl* ctrl,
                              int account_for_gravity, int64_t B, const void* q,
                              const void* dq, const void* target, const void* target_velocity,
                              void* u, int device, void* stream);

/* The same for Sliding.generate (sliding.py:34-99; BASELINE config 5), Joint / Damping / RestingConfig.generate
 * (joint.py:104-131, damping.py:21-32, resting_config.py:18-42) and the robot_config functions (base_config.py:210-415):
 * arguments as the *_batch entry point of the same name, host arrays only, n_shards contiguous row ranges on
 * devices[0..n_shards-1], no collective.  The shards of one device are staged in, launched and collected by one host
 * thread per device (the caller's own for the first device named), under that device's lock only: staging copies of
 * different devices overlap, and calls on disjoint device sets do not wait for each other.  Shards that should STAY
 * on the devices: the *_resident entry points below.                                                              */
int abrk_sliding_generate_sharded(int arm_id, int dtype, const abrk_sliding_params* params, int64_t B, const void* q,
                                  const void* dq, const void* target, const void* target_velocity,
                                  const void* target_acc, void* u, void* s_out, int n_shards, const int* devices);
int abrk_joint_generate_sharded(int arm_id, int dtype, const abrk_null_ctrl* ctrl, int account_for_gravity, int64_t B,
                                const void* q, const void* dq, const void* target, const void* target_velocity, void* u,
                                int n_shards, const int* devices);
int abrk_dynamics_sharded(int arm_id, int dtype, int64_t B, const void* q, const void* dq, int frame,
                          const double* x_off, uint32_t want, const abrk_dyn_out* out, int n_shards,
                          const int* devices);

/* ---- RESIDENT SHARDS ("results remain in per-device buffers unless the caller asks for host arrays";
 * north_star: "the batch shards trivially across the 8 GPUs of one node").  A batch whose shards LIVE on the devices, driven
 * by ONE host thread: every array argument is a table of n_shards DEVICE pointers - shard g holds rows[g] rows of every
 * array on devices[g] (a device may appear more than once; a NULL table = the array is absent).  A call only ENQUEUES:
 * shard g's kernels go to streams[g] (streams == NULL: the library's own stream of (device, k) for the k-th shard on
 * that device, abrk_shard_stream), nothing is staged, nothing is waited for; per-row state (integrated_error) stays
 * with its shard.  Semantics per shard are those of the *_batch entry point of the same name on (devices[g],
 * streams[g]) - the call IS that entry point, once per shard - so results are bit-identical to the unsharded call on
 * the same rows.  abrk_shards_sync drains every shard's stream and reports (once) ABRK_ESINGULAR of any of them.
 * Control loops record one plan per shard (abrk_plan_begin(devices[g], streams[g]) ... abrk_plan_end) and replay all of
 * them with one abrk_plans_launch per tick / per K ticks.  No collective, no exchange step: rows are independent.
 * Replaces: the reference evaluates one state per Python call (controllers/osc.py:217-320); its usage model - one
 * process owning the whole control loop, examples/PyGame/force_osc_xy.py:57-78 - scaled to N GPUs.               */
typedef struct abrk_shard_cut {
  int32_t n_shards;
  const int32_t* devices; /* [n_shards] */
  const int64_t* rows;    /* [n_shards]; 0 = the shard is skipped */
  void* const* streams;   /* [n_shards] or NULL */
} abrk_shard_cut;
void* abrk_shard_stream(int device, int slot); /* the stream a NULL `streams` stands for; NULL on failure */
int abrk_osc_generate_resident(int arm_id, int dtype, const abrk_osc_params* params, const abrk_shard_cut* cut,
                               const void* const* q, const void* const* dq, const void* const* target,
                               const void* const* target_velocity, void* const* integrated_error,
                               const void* const* u_null_ext, void* const* u, void* const* training_signal);
int abrk_sliding_generate_resident(int arm_id, int dtype, const abrk_sliding_params* params, const abrk_shard_cut* cut,
                                   const void* const* q, const void* const* dq, const void* const* target,
                                   const void* const* target_velocity, const void* const* target_acc, void* const* u,
                                   void* const* s_out);
int abrk_joint_generate_resident(int arm_id, int dtype, const abrk_null_ctrl* ctrl, int account_for_gravity,
                                 const abrk_shard_cut* cut, const void* const* q, const void* const* dq,
                                 const void* const* target, const void* const* target_velocity, void* const* u);
/* out: [n_shards] abrk_dyn_out, one per shard (only the fields selected by `want` are read) */
int abrk_dynamics_resident(int arm_id, int dtype, const abrk_shard_cut* cut, const void* const* q,
                           const void* const* dq, int frame, const double* x_off, uint32_t want,
                           const abrk_dyn_out* out);
int abrk_shards_sync(const abrk_shard_cut* cut);
/* `repeat` ticks of SEVERAL plans (one per shard) from one call: mode 0 = plain launches, 1 = one hipGraph of `repeat`
 * ticks per plan (abrk_plan_launch_graph).  Returns when every plan's work is enqueued.                          */
int abrk_plans_launch(const int* plans, int n_plans, int repeat, int mode);

/* ---------------------------------------------------------------------------------
 * The remaining secondary controllers.  Each writes u [B,n]; with accumulate != 0 it
 * adds to u instead (several secondary controllers summed on device before OSC's null-space filter,
 * abr_control/controllers/osc.py:310-318 - pass the sum as u_null_ext to abrk_osc_generate_batch).
 * --------------------------------------------------------------------------------- */

/* AvoidJointLimits (controllers/avoid_joint_limits.py:35-142).  The limit arrays are the ones the
 * reference's constructor stores (avoid_joint_limits.py:45-75): shifted by -pi, min/max swapped where
 * cross_zero, "no limit" (NaN there) flagged in no_limits_min / no_limits_max.                       */
typedef struct abrk_limits_params {
  double min_joint_angles[ABRK_MAX_JOINTS];
  double max_joint_angles[ABRK_MAX_JOINTS];
  double max_torque[ABRK_MAX_JOINTS];
  int32_t cross_zero[ABRK_MAX_JOINTS];
  int32_t gradient[ABRK_MAX_JOINTS];
  int32_t no_limits_min[ABRK_MAX_JOINTS];
  int32_t no_limits_max[ABRK_MAX_JOINTS];
} abrk_limits_params;

/* AvoidJointLimits.generate (avoid_joint_limits.py:83-142); depends on q only. */
int abrk_avoid_joint_limits_generate_batch(int n_joints, int dtype, const abrk_limits_params* params, int64_t B,
                                           const void* q, void* u, int accumulate, int device, void* stream);

/* Floating.generate (controllers/floating.py:27-71): gravity compensation in joint space or through
 * the task-space inertia of the EE (floating.py:42-62), minus M dq when dynamic (floating.py:66-69).
 * dq [B,n] is read only when dynamic != 0.                                                          */
int abrk_floating_generate_batch(int arm_id, int dtype, int dynamic, int task_space, int64_t B, const void* q,
                                 const void* dq, void* u, int accumulate, int device, void* stream);

/* AvoidObstacles.generate (controllers/avoid_obstacles.py:38-120): Khatib potential field between each
 * arm segment (joint_i .. joint_i+1 / EE) and each obstacle [x, y, z, radius], mapped through the
 * inertia of the closest point.  Obstacles are shared by all rows (set_obstacles, avoid_obstacles.py:122). */
#define ABRK_MAX_OBSTACLES 16
typedef struct abrk_obstacles_params {
  int32_t n_obstacles;
  int32_t reserved;
  double threshold, gain, maximum;
  double obstacles[ABRK_MAX_OBSTACLES][4];
} abrk_obstacles_params;

int abrk_avoid_obstacles_generate_batch(int arm_id, int dtype, const abrk_obstacles_params* params, int64_t B,
                                        const void* q, void* u, int accumulate, int device, void* stream);

/* ---------------------------------------------------------------------------------
 * Device plumbing (the host side is Python + ctypes; no PyTorch involved).
 * --------------------------------------------------------------------------------- */
int abrk_device_count(void);
int abrk_device_name(int device, char* buf, size_t len);
void* abrk_malloc(int device, size_t bytes);               /* NULL on failure */
int abrk_free(int device, void* p);
int abrk_memcpy_h2d(int device, void* dst, const void* src, size_t bytes, void* stream);
int abrk_memcpy_d2h(int device, void* dst, const void* src, size_t bytes, void* stream);
int abrk_memset(int device, void* dst, int value, size_t bytes, void* stream);
void* abrk_stream_create(int device);
int abrk_stream_destroy(int device, void* stream);
int abrk_stream_sync(int device, void* stream);
int abrk_device_sync(int device);
void* abrk_event_create(int device);
int abrk_event_destroy(int device, void* ev);
int abrk_event_record(int device, void* ev, void* stream);
int abrk_event_elapsed_ms(int device, void* start, void* stop, float* ms); /* syncs stop */

/* Diagnostics of the library's own device scratch (what the tests and a long-running host watch): the six-row OSC law
 * (any ctrlr_dof beyond x,y,z; osc.py:134-147 - its truncating pinv) parks the rows that need the eigen-decomposition in
 * a per-(device, stream) worklist; abrk_stream_destroy hands a stream's slot back.  Counters are process-wide and
 * monotonic. */
typedef struct abrk_scratch_info {
  int64_t worklist_slots;      /* (device, stream) pairs that currently hold six-row scratch, all devices */
  int64_t worklist_bytes;      /* device memory they hold */
  int64_t inline_fallbacks;    /* six-row calls that ran one-pass because no scratch could be had */
  int64_t evictions;           /* slots of idle / vanished streams that were recycled */
  int64_t device_free_bytes;   /* hipMemGetInfo of `device` */
  int64_t device_total_bytes;
  int64_t status_words_out;    /* ABRK_ESINGULAR words in use: one per live thread that made a host-array OSC call, one
                                  per (device, stream) that took a device-pointer OSC call and was not destroyed      */
  int64_t status_blocks;       /* pinned 4 KiB blocks (64 words each) the pool holds; never shrinks                  */
} abrk_scratch_info;
int abrk_scratch_stats(int device, abrk_scratch_info* out);

const char* abrk_last_error(void);
int abrk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ABRK_H */

// abrk_host_ctrl.cpp - the controllers beside OSC: dynamics, Sliding, Joint / Damping / RestingConfig,
// AvoidJointLimits, Floating, AvoidObstacles, inverse kinematics.
#include "abrk_host.h"
#include "abrk_params.h"

// ------------------------------------------------------------------------------- dynamics
void host::add_dyn_outputs(ArrayTable& t, int n, uint32_t want, int count) {
  static const char* const names[10] = {"Tx", "J", "M", "g", "C", "dJ", "R", "T", "Tinv", "quat"};
  const size_t N = (size_t)n;
  const size_t per[10] = {3, 6 * N, N * N, N, N * N, 6 * N, 9, 16, 16, 4};
  for (int i = 0; i < count; i++) t.add(names[i], per[i], kWritten, (want >> i & 1) != 0);
}
ArrayTable host::dynamics_arrays(int n, uint32_t want) {
  ArrayTable t;
  t.add("q", n, kRead);
  t.add("dq", n, kRead, (want & (ABRK_WANT_C | ABRK_WANT_DJ)) != 0);
  add_dyn_outputs(t, n, want, 10);
  return t;
}
int host::dynamics_call(int arm_id, int dtype, int64_t B, void* const* arr, int frame, const double* x_off,
                        uint32_t want, int device, void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  const int n = a->desc.n_joints;
  if (frame < 0 || frame > 2 * n + 1) return fail(ABRK_EFRAME, "Invalid transformation name: frame id %d", frame);
  if (!want) return fail(ABRK_EINVAL, "nothing requested");
  if (want >> 10) return fail(ABRK_EINVAL, "unknown want bits 0x%x", want);
  if (!arr[0]) return fail(ABRK_EINVAL, "q is NULL");
  if ((want & (ABRK_WANT_C | ABRK_WANT_DJ)) && !arr[1]) return fail(ABRK_EINVAL, "C / dJ need dq");
  for (int i = 0; i < 10; i++)
    if ((want >> i & 1) && !arr[2 + i]) return fail(ABRK_EINVAL, "output %d requested but its pointer is NULL", i);
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  Stager st{device, (hipStream_t)stream};
  DynArgs da{};
  void** fields[12] = {(void**)&da.q, (void**)&da.dq};
  for (int i = 0; i < 10; i++) fields[2 + i] = &da.out[i];
  st.bind_table(dynamics_arrays(n, want), arr, fields, B, esz(dtype));
  if (int rc = st.reserve()) return rc;
  da.frame = frame;
  da.m = frame_m(frame, n);
  for (int r = 0; r < 3; r++) da.off[r] = x_off ? x_off[r] : 0.0;
  da.want = want;
  return launch_arm(st, a, dtype, B, &ArmOps::dyn, da);
}
extern "C" int abrk_dynamics_batch(int arm_id, int dtype, int64_t B, const void* q, const void* dq, int frame,
                                   const double* x_off, uint32_t want, const abrk_dyn_out* out, int device,
                                   void* stream) {
  static_assert(sizeof(abrk_dyn_out) == 10 * sizeof(void*), "abrk_dyn_out is its ten pointers");
  void* arr[12] = {const_cast<void*>(q), const_cast<void*>(dq)};
  if (out) memcpy(arr + 2, out, sizeof *out);
  return dynamics_call(arm_id, dtype, B, arr, frame, x_off, want, device, stream);
}

// ------------------------------------------------------------------------------- Sliding
ArrayTable host::sliding_arrays(int n, bool cartesian) {
  const size_t nt = cartesian ? 3 : n;
  ArrayTable t;
  t.add("q", n, kRead);
  t.add("dq", n, kRead);
  t.add("target", nt, kRead);
  t.add("target_velocity", nt, kRead);
  t.add("target_acc", nt, kRead);
  t.add("u", n, kWritten);
  t.add("s", n, kWritten);
  return t;
}
int host::sliding_call(int arm_id, int dtype, const abrk_sliding_params* P, int64_t B, void* const* arr, int device,
                       void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  const int n = a->desc.n_joints;
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  if (P->ref_frame < 0 || P->ref_frame > 2 * n + 1)
    return fail(ABRK_EFRAME, "Invalid transformation name: frame id %d", P->ref_frame);
  if (!arr[0] || !arr[1] || !arr[2] || !arr[5]) return fail(ABRK_EINVAL, "q, dq, target and u are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  Stager st{device, (hipStream_t)stream};
  SlidingArgs sa;
  void** const fields[] = {(void**)&sa.q, (void**)&sa.dq, (void**)&sa.target, (void**)&sa.tv, (void**)&sa.ta, &sa.u, &sa.s};
  st.bind_table(sliding_arrays(n, P->cartesian != 0), arr, fields, B, esz(dtype));
  if (int rc = st.reserve()) return rc;
  const auto pb = blocks([&](auto t) { return make_slidingp<decltype(t)>(*P, n); });
  return launch_arm(st, a, dtype, B, &ArmOps::sliding, sa, pb);
}
extern "C" int abrk_sliding_generate_batch(int arm_id, int dtype, const abrk_sliding_params* P, int64_t B,
                                           const void* q, const void* dq, const void* target,
                                           const void* target_velocity, const void* target_acc, void* u, void* s_out,
                                           int device, void* stream) {
  void* const arr[] = {(void*)q, (void*)dq, (void*)target, (void*)target_velocity, (void*)target_acc, u, s_out};
  return sliding_call(arm_id, dtype, P, B, arr, device, stream);
}

// ------------------------------------------------------------------------------- Joint / Damping / RestingConfig
ArrayTable host::joint_arrays(int n) {
  ArrayTable t;
  t.add("q", n, kRead);
  t.add("dq", n, kRead);
  t.add("target", n, kRead);
  t.add("target_velocity", n, kRead);
  t.add("u", n, kWritten);
  return t;
}
int host::joint_call(int arm_id, int dtype, const abrk_null_ctrl* ctrl, int account_for_gravity, int64_t B,
                     void* const* arr, int device, void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  if (!ctrl) return fail(ABRK_EINVAL, "ctrl is NULL");
  if (ctrl->kind < 0 || ctrl->kind > 2) return fail(ABRK_EINVAL, "unknown controller kind %d", ctrl->kind);
  if (!arr[0] || !arr[1] || !arr[4]) return fail(ABRK_EINVAL, "q, dq and u are required");
  if (ctrl->kind == 0 && !arr[2]) return fail(ABRK_EINVAL, "Joint.generate needs target");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  Stager st{device, (hipStream_t)stream};
  JointArgs ja;
  void** const fields[] = {(void**)&ja.q, (void**)&ja.dq, (void**)&ja.target, (void**)&ja.tv, &ja.u};
  st.bind_table(joint_arrays(a->desc.n_joints), arr, fields, B, esz(dtype));
  if (int rc = st.reserve()) return rc;
  const auto pb = blocks([&](auto t) { return make_jointp<decltype(t)>(*ctrl, account_for_gravity); });
  return launch_arm(st, a, dtype, B, &ArmOps::joint, ja, pb);
}
extern "C" int abrk_joint_generate_batch(int arm_id, int dtype, const abrk_null_ctrl* ctrl, int account_for_gravity,
                                         int64_t B, const void* q, const void* dq, const void* target,
                                         const void* target_velocity, void* u, int device, void* stream) {
  void* const arr[] = {(void*)q, (void*)dq, (void*)target, (void*)target_velocity, u};
  return joint_call(arm_id, dtype, ctrl, account_for_gravity, B, arr, device, stream);
}

// ------------------------------------------------------------------------------- AvoidJointLimits / Floating / AvoidObstacles
extern "C" int abrk_avoid_joint_limits_generate_batch(int n_joints, int dtype, const abrk_limits_params* params,
                                                      int64_t B, const void* q, void* u, int accumulate, int device,
                                                      void* stream) {
  if (int rc = check_joints(n_joints)) return rc;
  if (int rc = check_batch(dtype, B)) return rc;
  if (!params) return fail(ABRK_EINVAL, "params is NULL");
  if (!q || !u) return fail(ABRK_EINVAL, "q and u are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const int n = n_joints;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  const void* qd;
  void* ud;
  st.in(&qd, q, B * n * s);
  st.bind(&ud, u, B * n * s, accumulate != 0, true);
  if (int rc = st.reserve()) return rc;
  const auto pb = blocks([&](auto t) { return make_limitsp<decltype(t)>(*params); });
  const hipStream_t hs = (hipStream_t)stream;
  return dispatch(st, nullptr, dtype, [=](const void*) {
    return launch_limits(n, dtype, LaunchArgs{nullptr, (long)B, hs}, pb.of(dtype), qd, ud, accumulate != 0);
  });
}

extern "C" int abrk_floating_generate_batch(int arm_id, int dtype, int dynamic, int task_space, int64_t B,
                                            const void* q, const void* dq, void* u, int accumulate, int device,
                                            void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  const int n = a->desc.n_joints;
  if (!q || !u) return fail(ABRK_EINVAL, "q and u are required");
  if (dynamic && !dq) return fail(ABRK_EINVAL, "Floating(dynamic=True) needs dq");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  FloatingArgs fa;
  fa.dynamic = dynamic != 0;
  fa.task_space = task_space != 0;
  fa.acc = accumulate != 0;
  st.in(&fa.q, q, B * n * s);
  st.in(&fa.dq, dynamic ? dq : nullptr, B * n * s);
  st.bind(&fa.u, u, B * n * s, accumulate != 0, true);
  if (int rc = st.reserve()) return rc;
  return launch_arm(st, a, dtype, B, &ArmOps::floating, fa);
}

extern "C" int abrk_avoid_obstacles_generate_batch(int arm_id, int dtype, const abrk_obstacles_params* params,
                                                   int64_t B, const void* q, void* u, int accumulate, int device,
                                                   void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  const int n = a->desc.n_joints;
  if (!params) return fail(ABRK_EINVAL, "params is NULL");
  if (params->n_obstacles < 0 || params->n_obstacles > ABRK_MAX_OBSTACLES)
    return fail(ABRK_EINVAL, "n_obstacles=%d outside 0..%d", params->n_obstacles, ABRK_MAX_OBSTACLES);
  if (!(params->threshold > 0)) return fail(ABRK_EINVAL, "threshold must be positive");
  if (!q || !u) return fail(ABRK_EINVAL, "q and u are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  ObstaclesArgs oa{};
  oa.acc = accumulate != 0;
  st.in(&oa.q, q, B * n * s);
  st.bind(&oa.u, u, B * n * s, accumulate != 0, true);
  if (int rc = st.reserve()) return rc;
  const auto pb = blocks([&](auto t) { return make_obsp<decltype(t)>(*params); });
  return launch_arm(st, a, dtype, B, &ArmOps::obstacles, oa, pb);
}

// ------------------------------------------------------------------------------- inverse kinematics
extern "C" int abrk_ik_generate_path_batch(int arm_id, int dtype, const abrk_ik_params* P, int64_t B,
                                           const void* position, const void* target, void* position_path,
                                           void* velocity_path, int device, void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  const int n = a->desc.n_joints;
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  if (P->method < 1 || P->method > 3) return fail(ABRK_EINVAL, "method %d outside 1..3", P->method);
  if (P->n_timesteps < 0) return fail(ABRK_EINVAL, "negative n_timesteps");
  if (!position || !target || !position_path || !velocity_path)
    return fail(ABRK_EINVAL, "position, target, position_path and velocity_path are required");
  if (B == 0 || P->n_timesteps == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  const size_t T = (size_t)P->n_timesteps;
  Stager st{device, (hipStream_t)stream};
  IkArgs ia{};
  st.in(&ia.q, position, B * n * s);
  st.in(&ia.target, target, B * 6 * s);
  st.out(&ia.pp, position_path, B * T * n * s);
  st.out(&ia.vp, velocity_path, B * T * n * s);
  if (int rc = st.reserve()) return rc;
  const auto pb = blocks([&](auto t) {
    using R = decltype(t);
    return IkP<R>{R(P->max_dx * P->dt), R(P->max_dr * P->dt), R(P->max_dq * P->dt), P->n_timesteps, P->method};
  });
  return launch_arm(st, a, dtype, B, &ArmOps::ik, ia, pb);
}

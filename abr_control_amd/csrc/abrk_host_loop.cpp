// abrk_host_loop.cpp - what a closed loop adds around the law: two-link step and rollout, the rigid-body plant, the
// loop recorder, end-effector contact, whole-arm contact, the force-control law, the path planner, the adaptive signal
// and the measurement channel.
#include <cmath>

#include "abrk_host.h"
#include "abrk_adapt.h"
#include "abrk_channel.h"
#include "abrk_params.h"
#include "abrk_path.h"

// ------------------------------------------------------------------------------- two-link plant / closed loop
namespace {
template <class T>
TwoLinkP<T> make_plant(const abrk_twolink_plant& s) {
  TwoLinkP<T> k;
  k.K1 = T(s.K1);
  k.K2 = T(s.K2);
  k.K3 = T(s.K3);
  k.K4 = T(s.K4);
  k.dt = T(s.dt);
  return k;
}
}  // namespace

extern "C" int abrk_twolink_step_batch(int dtype, const abrk_twolink_plant* plant, int64_t B, void* q, void* dq,
                                       const void* u, int device, void* stream) {
  if (int rc = check_batch(dtype, B)) return rc;
  if (!plant || !q || !dq || !u) return fail(ABRK_EINVAL, "plant, q, dq and u are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  void *qd, *dqd;
  const void* ud;
  st.inout(&qd, q, B * 2 * s);
  st.inout(&dqd, dq, B * 2 * s);
  st.in(&ud, u, B * 2 * s);
  if (int rc = st.reserve()) return rc;
  const auto kb = blocks([&](auto t) { return make_plant<decltype(t)>(*plant); });
  const hipStream_t hs = (hipStream_t)stream;
  return dispatch(st, nullptr, dtype, [=](const void*) {
    return launch_twolink_step(dtype, LaunchArgs{nullptr, (long)B, hs}, kb.of(dtype), qd, dqd, ud);
  });
}

extern "C" int abrk_osc_rollout_twolink_batch(int arm_id, int dtype, const abrk_osc_params* P,
                                              const abrk_twolink_plant* plant, int64_t B, int32_t n_steps,
                                              int32_t every, void* q, void* dq, const void* target,
                                              void* integrated_error, void* q_traj, void* dq_traj, void* u_traj,
                                              int device, void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  const int n = a->desc.n_joints;
  if (n != 2 || !a->ops->rollout)
    return fail(ABRK_EINVAL, "the plant of this entry point is the two-link arm (arms/twojoint/arm_sim.py); arm has %d joints", n);
  if (!P || !plant) return fail(ABRK_EINVAL, "params / plant is NULL");
  if (P->ref_frame < 0 || P->ref_frame > 2 * n + 1)
    return fail(ABRK_EFRAME, "Invalid transformation name: frame id %d", P->ref_frame);
  if (P->n_null < 0 || P->n_null > ABRK_MAX_NULL) return fail(ABRK_EINVAL, "n_null=%d outside 0..%d", P->n_null, ABRK_MAX_NULL);
  int k = 0;
  for (int r = 0; r < 6; r++) k += P->ctrlr_dof[r] ? 1 : 0;
  if (k == 0) return fail(ABRK_EINVAL, "ctrlr_dof selects no task-space dimension");
  if (n_steps < 0 || every < 0) return fail(ABRK_EINVAL, "negative n_steps / every");
  if (!q || !dq || !target) return fail(ABRK_EINVAL, "q, dq and target are required");
  if (P->ki != 0 && !integrated_error) return fail(ABRK_EINVAL, "ki != 0 needs the integrated_error state array");
  if ((q_traj || dq_traj || u_traj) && every <= 0) return fail(ABRK_EINVAL, "trajectory outputs need every > 0");
  if (B == 0 || n_steps == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  const size_t n_chk = every > 0 ? (size_t)(n_steps / every) : 0;
  Stager st{device, (hipStream_t)stream};
  RolloutArgs ra{};
  st.inout(&ra.q, q, B * 2 * s);
  st.inout(&ra.dq, dq, B * 2 * s);
  st.in(&ra.target, target, B * 6 * s);
  st.inout(&ra.ierr, P->ki != 0 ? integrated_error : nullptr, B * 6 * s);
  st.out(&ra.qt, q_traj, B * n_chk * 2 * s);
  st.out(&ra.dqt, dq_traj, B * n_chk * 2 * s);
  st.out(&ra.ut, u_traj, B * n_chk * 2 * s);
  if (int rc = st.reserve()) return rc;
  ra.use_C = P->use_C ? 1 : 0;
  ra.fast = osc_fast_rows(*P, n, false);
  ra.n_steps = n_steps;
  ra.every = every;
  auto pb = blocks([&](auto t) { return make_oscp<decltype(t)>(*P, n); });
  const auto kb = blocks([&](auto t) { return make_plant<decltype(t)>(*plant); });
  const ArmOps* ops = a->ops;
  const hipStream_t hs = (hipStream_t)stream;
  return with_status_word(st, pb, nullptr, [&] {
    return dispatch(st, a, dtype, [=](const void* rt) {
      RolloutArgs o = ra;
      o.P = pb.of(dtype);
      o.K = kb.of(dtype);
      return ops->rollout(dtype, LaunchArgs{rt, (long)B, hs}, o);
    });
  });
}

// ------------------------------------------------------- rigid-body plant of any arm, plain and with non-ideal effects
namespace {
template <class T>
PlantP<T> make_plantp(double h, int substeps, int gravity, int mode) {
  PlantP<T> p;
  p.h = T(h);
  p.substeps = substeps;
  p.gravity = gravity;
  p.mode = mode;
  p.status = nullptr;
  return p;
}
// Every field of the arm's n joints must be finite whether its effect is on or not (a zeroed struct is); the sign and
// order rules of tau_max, coulomb_vs and the limits hold where their flag puts them to use.
int check_effects(const abrk_plant_effects* fx, int n) {
  if (!fx) return 0;
  const uint32_t all = ABRK_FX_SATURATION | ABRK_FX_VISCOUS | ABRK_FX_COULOMB | ABRK_FX_LIMITS;
  if (fx->flags & ~all) return fail(ABRK_EINVAL, "effects: flags=0x%x has bits beyond ABRK_FX_*", fx->flags);
  for (int i = 0; i < n; i++) {
    if (!nonnegative_finite_at(&fx->damping[i]))
      return fail(ABRK_EINVAL, "effects: damping[%d]=%g is not a finite value >= 0", i, fx->damping[i]);
    if (!nonnegative_finite_at(&fx->coulomb[i]))
      return fail(ABRK_EINVAL, "effects: coulomb[%d]=%g is not a finite value >= 0", i, fx->coulomb[i]);
    if (!finite_at(&fx->tau_max[i]) || ((fx->flags & ABRK_FX_SATURATION) && !positive_finite_at(&fx->tau_max[i])))
      return fail(ABRK_EINVAL, "effects: tau_max[%d]=%g is not a finite value > 0", i, fx->tau_max[i]);
    if (!finite_at(&fx->q_min[i]) || !finite_at(&fx->q_max[i]))
      return fail(ABRK_EINVAL, "effects: q_min[%d]=%g, q_max[%d]=%g: a limit is not finite", i, fx->q_min[i], i,
                  fx->q_max[i]);
    if ((fx->flags & ABRK_FX_LIMITS) && !(fx->q_min[i] < fx->q_max[i]))
      return fail(ABRK_EINVAL, "effects: q_min[%d]=%g is not below q_max[%d]=%g", i, fx->q_min[i], i, fx->q_max[i]);
  }
  if (!finite_at(&fx->coulomb_vs) || ((fx->flags & ABRK_FX_COULOMB) && !positive_finite_at(&fx->coulomb_vs)))
    return fail(ABRK_EINVAL, "effects: coulomb_vs=%g is not a finite value > 0", fx->coulomb_vs);
  if (!nonnegative_finite_at(&fx->restitution) || fx->restitution > 1.0)
    return fail(ABRK_EINVAL, "effects: restitution=%g is outside [0, 1]", fx->restitution);
  return 0;
}
// the checks of the two step entries, ahead of plant_impl's own
int check_plant_params(int arm_id, const abrk_plant_params* P) {
  if (!get_arm(arm_id)) return fail(ABRK_ENOARM, "unknown arm id %d", arm_id);
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  if (!positive_finite_at(&P->dt)) return fail(ABRK_EINVAL, "dt=%g is not a positive finite step", P->dt);
  if (P->substeps < 1) return fail(ABRK_EINVAL, "substeps=%d < 1", P->substeps);
  return 0;
}
// A host payload array [B, 4] = m, rx, ry, rz of `dtype`, looked at where it is about to be staged: m finite and >= 0, r
// finite.  (A device array is taken as it is: the kernel reads it at every launch, long after any check here.)
int check_payload_host(int dtype, int64_t B, const void* payload) {
  for (int64_t b = 0; b < B; b++)
    for (int k = 0; k < 4; k++) {
      double v;
      if (dtype == ABRK_F64) {
        memcpy(&v, static_cast<const char*>(payload) + (b * 4 + k) * 8, 8);
      } else {
        float f;
        memcpy(&f, static_cast<const char*>(payload) + (b * 4 + k) * 4, 4);
        v = f;  // (exact; an infinity or a NaN stays one)
      }
      if (k == 0 ? !nonnegative_finite_at(&v) : !finite_at(&v))
        return fail(ABRK_EINVAL, "payload: row %lld: %s=%g is not a finite value%s", (long long)b,
                    k == 0 ? "m" : k == 1 ? "rx" : k == 2 ? "ry" : "rz", v, k == 0 ? " >= 0" : "");
    }
  return 0;
}
// mode 0: ddq out, q / dq read; mode 1: q / dq in place.  fx_entry: the entries with non-ideal effects, which launch the
// effects kernel whatever is switched on; the others launch the plain kernel and pass no fx, tau_ext or wrench.  With a
// payload (fx entries only) the payload kernel is launched instead.
int plant_impl(bool fx_entry, int arm_id, int dtype, int mode, double dt, int substeps, int gravity,
               const abrk_plant_effects* fx, int64_t B, void* q, void* dq, const void* u, const void* tau_ext,
               const void* wrench, void* ddq, int device, void* stream, const void* payload = nullptr) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  if (payload && !a->ops->plant_load)
    return fail(ABRK_EINVAL, "this arm's kernels carry no plant with a payload (rebuild its plugin)");
  if (!fx_entry && !a->ops->plant) return fail(ABRK_EINVAL, "this arm's kernels carry no plant (rebuild its plugin)");
  if (fx_entry && !a->ops->plant_fx)
    return fail(ABRK_EINVAL, "this arm's kernels carry no plant with effects (rebuild its plugin)");
  if (!q || !dq || !u || (mode == 0 && !ddq)) return fail(ABRK_EINVAL, "q, dq, u%s are required", mode == 0 ? ", ddq" : "");
  const int n = a->desc.n_joints;
  if (int rc = check_effects(fx, n)) return rc;
  if (B == 0) return 0;
  if (payload && !device_view(payload))
    if (int rc = check_payload_host(dtype, B, payload)) return rc;
  if (int rc = use_device(device)) return rc;
  const size_t bytes = (size_t)B * n * esz(dtype);
  Stager st{device, (hipStream_t)stream};
  const void* pl = nullptr;
  PlantFxArgs pa{};  // (the plain kernel's PlantArgs: its q, dq, u and ddq)
  if (mode == 0) {
    st.bind(&pa.q, q, bytes, true, false);
    st.bind(&pa.dq, dq, bytes, true, false);
  } else {
    st.inout(&pa.q, q, bytes);
    st.inout(&pa.dq, dq, bytes);
  }
  st.in(&pa.u, u, bytes);
  st.in(&pa.tau_ext, tau_ext, bytes);
  st.in(&pa.wrench, wrench, (size_t)B * 6 * esz(dtype));
  st.in(&pl, payload, (size_t)B * 4 * esz(dtype));
  st.out(&pa.ddq, mode == 0 ? ddq : nullptr, bytes);
  if (int rc = st.reserve()) return rc;
  auto pb = blocks([&](auto t) { return make_plantp<decltype(t)>(dt / substeps, substeps, gravity, mode); });
  const ArmOps* ops = a->ops;
  const hipStream_t hs = (hipStream_t)stream;
  return with_status_word(st, pb, nullptr, [&] {
    if (!fx_entry)
      return dispatch(st, a, dtype, [=](const void* rt) {
        return ops->plant(dtype, LaunchArgs{rt, (long)B, hs}, PlantArgs{pb.of(dtype), pa.q, pa.dq, pa.u, pa.ddq});
      });
    const auto fb = blocks([&](auto t) { return make_plantfx<decltype(t)>(fx, n, tau_ext != nullptr, wrench != nullptr); });
    return dispatch(st, a, dtype, [=](const void* rt) {
      PlantFxArgs o = pa;
      o.P = pb.of(dtype);
      o.F = fb.of(dtype);
      if (payload) return ops->plant_load(dtype, LaunchArgs{rt, (long)B, hs}, PlantLoadArgs{o, pl});
      return ops->plant_fx(dtype, LaunchArgs{rt, (long)B, hs}, o);
    });
  });
}
}  // namespace

extern "C" int abrk_forward_dynamics_batch(int arm_id, int dtype, int64_t B, const void* q, const void* dq,
                                           const void* u, void* ddq, int device, void* stream) {
  return plant_impl(false, arm_id, dtype, 0, 1.0, 1, 1, nullptr, B, const_cast<void*>(q), const_cast<void*>(dq), u,
                    nullptr, nullptr, ddq, device, stream);
}

extern "C" int abrk_plant_step_batch(int arm_id, int dtype, const abrk_plant_params* P, int64_t B, void* q, void* dq,
                                     const void* u, int device, void* stream) {
  if (int rc = check_plant_params(arm_id, P)) return rc;
  return plant_impl(false, arm_id, dtype, 1, P->dt, P->substeps, P->gravity ? 1 : 0, nullptr, B, q, dq, u, nullptr,
                    nullptr, nullptr, device, stream);
}

extern "C" int abrk_forward_dynamics_fx_batch(int arm_id, int dtype, const abrk_plant_effects* fx, int64_t B,
                                              const void* q, const void* dq, const void* u, const void* tau_ext,
                                              const void* wrench, void* ddq, int device, void* stream) {
  return plant_impl(true, arm_id, dtype, 0, 1.0, 1, 1, fx, B, const_cast<void*>(q), const_cast<void*>(dq), u, tau_ext,
                    wrench, ddq, device, stream);
}

extern "C" int abrk_plant_step_fx_batch(int arm_id, int dtype, const abrk_plant_params* P, const abrk_plant_effects* fx,
                                        int64_t B, void* q, void* dq, const void* u, const void* tau_ext,
                                        const void* wrench, int device, void* stream) {
  if (int rc = check_plant_params(arm_id, P)) return rc;
  return plant_impl(true, arm_id, dtype, 1, P->dt, P->substeps, P->gravity ? 1 : 0, fx, B, q, dq, u, tau_ext, wrench,
                    nullptr, device, stream);
}

extern "C" int abrk_forward_dynamics_payload_batch(int arm_id, int dtype, const abrk_plant_effects* fx, int64_t B,
                                                   const void* q, const void* dq, const void* u, const void* tau_ext,
                                                   const void* wrench, const void* payload, void* ddq, int device,
                                                   void* stream) {
  return plant_impl(true, arm_id, dtype, 0, 1.0, 1, 1, fx, B, const_cast<void*>(q), const_cast<void*>(dq), u, tau_ext,
                    wrench, ddq, device, stream, payload);
}

extern "C" int abrk_plant_step_payload_batch(int arm_id, int dtype, const abrk_plant_params* P,
                                             const abrk_plant_effects* fx, int64_t B, void* q, void* dq, const void* u,
                                             const void* tau_ext, const void* wrench, const void* payload, int device,
                                             void* stream) {
  if (int rc = check_plant_params(arm_id, P)) return rc;
  return plant_impl(true, arm_id, dtype, 1, P->dt, P->substeps, P->gravity ? 1 : 0, fx, B, q, dq, u, tau_ext, wrench,
                    nullptr, device, stream, payload);
}

// ------------------------------------------------------------------------------- loop recorder
namespace {
static_assert((unsigned)ABRK_TR_Q == (unsigned)TR_Q && (unsigned)ABRK_TR_DQ == (unsigned)TR_DQ &&
                  (unsigned)ABRK_TR_U == (unsigned)TR_U && (unsigned)ABRK_TR_TARGET == (unsigned)TR_TARGET &&
                  (unsigned)ABRK_TR_XYZ == (unsigned)TR_XYZ && (unsigned)ABRK_TR_ERR == (unsigned)TR_ERR,
              "abrk_types.h and abrk_trace.h name the same columns");
template <class T>
TraceP<T> make_tracep(const abrk_trace_params& P, int n) {
  TraceP<T> p;
  p.frame = P.frame;
  for (int r = 0; r < 3; r++) p.off[r] = T(P.x_off[r]);
  p.every = P.every;
  p.capacity = P.capacity;
  p.columns = P.columns;
  p.W = trace_width(P.columns, n);
  p.lds = 1;
  p.tol = P.tol;
  return p;
}
}  // namespace

extern "C" int abrk_loop_trace_batch(int arm_id, int dtype, const abrk_trace_params* P, int64_t B, const void* q,
                                     const void* dq, const void* u, const void* target, void* counter, void* history,
                                     void* stats, void* settle, int device, void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  if (!a->ops->trace) return fail(ABRK_EINVAL, "this arm's kernels carry no loop recorder (rebuild its plugin)");
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  const int n = a->desc.n_joints;
  if (P->frame < 0 || P->frame > 2 * n + 1) return fail(ABRK_EINVAL, "Invalid transformation name: frame id %d", P->frame);
  for (int r = 0; r < 3; r++)
    if (!finite_at(&P->x_off[r])) return fail(ABRK_EINVAL, "x_off[%d] is not finite", r);
  if (!finite_at(&P->tol)) return fail(ABRK_EINVAL, "tol is not finite");
  if (P->every < 1) return fail(ABRK_EINVAL, "every=%d < 1", P->every);
  if (!history && !stats) return fail(ABRK_EINVAL, "neither a history nor statistics requested");
  const unsigned cols = history ? P->columns : 0u;
  if (history) {
    if (P->capacity < 1) return fail(ABRK_EINVAL, "capacity=%d < 1", P->capacity);
    if (!cols || (cols & ~(unsigned)TR_ALL)) return fail(ABRK_EINVAL, "column mask 0x%x is empty or has unknown bits", cols);
  }
  if (!counter) return fail(ABRK_EINVAL, "counter is NULL");
  const bool need_err = (cols & ABRK_TR_ERR) || stats;
  if (!q && (need_err || (cols & (ABRK_TR_Q | ABRK_TR_XYZ)))) return fail(ABRK_EINVAL, "q is NULL");
  if (!dq && (cols & ABRK_TR_DQ)) return fail(ABRK_EINVAL, "the dq column is selected but dq is NULL");
  if (!u && (cols & ABRK_TR_U)) return fail(ABRK_EINVAL, "the u column is selected but u is NULL");
  if (!target && (need_err || (cols & ABRK_TR_TARGET))) return fail(ABRK_EINVAL, "err, the target column and the statistics need target");
  if (stats && !settle) return fail(ABRK_EINVAL, "statistics need settle");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  const int W = trace_width(cols, n);
  Stager st{device, (hipStream_t)stream};
  TraceArgs ta{};
  st.in(&ta.q, q, (size_t)B * n * s);
  st.in(&ta.dq, (cols & ABRK_TR_DQ) ? dq : nullptr, (size_t)B * n * s);
  st.in(&ta.u, (cols & ABRK_TR_U) ? u : nullptr, (size_t)B * n * s);
  st.in(&ta.target, target, (size_t)B * 6 * s);
  st.inout(&ta.counter, counter, (size_t)B * 4);
  // (in as well as out: slots that are not due keep the caller's values)
  st.inout(&ta.history, history, history ? (size_t)P->capacity * B * W * s : 0);
  st.inout(&ta.stats, stats, (size_t)B * 4 * 8);
  st.inout(&ta.settle, stats ? settle : nullptr, (size_t)B * 4);
  if (int rc = st.reserve()) return rc;
  abrk_trace_params Pc = *P;
  Pc.columns = cols;
  const auto pb = blocks([&](auto t) { return make_tracep<decltype(t)>(Pc, n); });
  return launch_arm(st, a, dtype, B, &ArmOps::trace, ta, pb);
}

// ------------------------------------------------------------------------------- end-effector contact
namespace {
static_assert(ABRK_CONTACT_MAX_SURFACES == kContactMaxSurfaces, "abrk.h and abrk_contact.h agree on the surfaces of a row");
template <class T>
ContactP<T> make_contactp(const abrk_contact_params& P, int n) {
  ContactP<T> p;
  p.frame = P.frame;
  p.m = frame_m(P.frame, n);
  for (int r = 0; r < 3; r++) p.off[r] = T(P.off[r]);
  p.S = P.n_surfaces;
  p.vs2 = T(P.vs * P.vs);
  p.accumulate = P.accumulate ? 1 : 0;
  return p;
}
// A host surface array [B, S, 8] = nx, ny, nz, d, k, c, mu, rho of `dtype`, looked at where it is about to be staged:
// everything finite, | |n| - 1 | <= 1e-6, and k, c, mu, rho >= 0.  (A device array is taken as it is.)
int check_surface_host(int dtype, int64_t B, int S, const void* surface) {
  static const char* const names[8] = {"nx", "ny", "nz", "d", "k", "c", "mu", "rho"};
  for (int64_t b = 0; b < B; b++)
    for (int s = 0; s < S; s++) {
      double v[8];
      for (int k = 0; k < 8; k++) {
        const int64_t at = (b * S + s) * 8 + k;
        if (dtype == ABRK_F64) {
          memcpy(&v[k], static_cast<const char*>(surface) + at * 8, 8);
        } else {
          float f;
          memcpy(&f, static_cast<const char*>(surface) + at * 4, 4);
          v[k] = f;  // (exact; an infinity or a NaN stays one)
        }
        if (!finite_at(&v[k]))
          return fail(ABRK_EINVAL, "surface: row %lld, surface %d: %s is not finite", (long long)b, s, names[k]);
        if (k >= 4 && !nonnegative_finite_at(&v[k]))
          return fail(ABRK_EINVAL, "surface: row %lld, surface %d: %s=%g is negative", (long long)b, s, names[k], v[k]);
      }
      const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      if (!(std::fabs(len - 1.0) <= 1e-6))
        return fail(ABRK_EINVAL, "surface: row %lld, surface %d: |n|=%.9g is not 1 to within 1e-6", (long long)b, s, len);
    }
  return 0;
}
}  // namespace

extern "C" int abrk_contact_step_batch(int arm_id, int dtype, const abrk_contact_params* P, int64_t B, const void* q,
                                       const void* dq, const void* surface, void* tau, void* report, int device,
                                       void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  if (!a->ops->contact) return fail(ABRK_EINVAL, "this arm's kernels carry no contact step (rebuild its plugin)");
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  const int n = a->desc.n_joints;
  if (P->frame < 0 || P->frame > 2 * n + 1) return fail(ABRK_EINVAL, "Invalid transformation name: frame id %d", P->frame);
  for (int r = 0; r < 3; r++)
    if (!finite_at(&P->off[r])) return fail(ABRK_EINVAL, "off[%d] is not finite", r);
  if (P->n_surfaces < 1 || P->n_surfaces > ABRK_CONTACT_MAX_SURFACES)
    return fail(ABRK_EINVAL, "n_surfaces=%d outside 1..%d", P->n_surfaces, ABRK_CONTACT_MAX_SURFACES);
  if (!positive_finite_at(&P->vs)) return fail(ABRK_EINVAL, "vs=%g is not a finite value > 0", P->vs);
  if (!q || !dq || !surface || !tau) return fail(ABRK_EINVAL, "q, dq, surface and tau are required");
  if (B == 0) return 0;
  const int S = P->n_surfaces;
  if (!device_view(surface))
    if (int rc = check_surface_host(dtype, B, S, surface)) return rc;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  ContactArgs ca{};
  st.in(&ca.q, q, (size_t)B * n * s);
  st.in(&ca.dq, dq, (size_t)B * n * s);
  st.in(&ca.surface, surface, (size_t)B * S * 8 * s);
  // (accumulate: tau goes in as well as out)
  st.bind(&ca.tau, tau, (size_t)B * n * s, P->accumulate != 0, true);
  st.out(&ca.report, report, (size_t)B * 8 * s);
  if (int rc = st.reserve()) return rc;
  const auto pb = blocks([&](auto t) { return make_contactp<decltype(t)>(*P, n); });
  return launch_arm(st, a, dtype, B, &ArmOps::contact, ca, pb);
}

// ------------------------------------------------------------------------------- force-controlled contact
namespace {
template <class T>
ForceP<T> make_forcep(const abrk_force_params& P, int n) {
  ForceP<T> p;
  p.frame = P.frame;
  p.m = frame_m(P.frame, n);
  for (int r = 0; r < 3; r++) p.off[r] = T(P.off[r]);
  p.kp = T(P.kp);
  p.kv = T(P.kv);
  p.kf = T(P.kf);
  p.ki = T(P.ki);
  p.i_max = T(P.i_max);
  p.kvf = T(P.kvf);
  p.f_touch = T(P.f_touch);
  p.v_app = T(P.v_app);
  p.kv_null = T(P.kv_null);
  p.dt = T(P.dt);
  p.use_g = P.use_g ? 1 : 0;
  p.accumulate = P.accumulate ? 1 : 0;
  p.force_ld = P.force_ld;
  p.status = nullptr;
  return p;
}
// A host command array [B, 4] = nx, ny, nz, f_des of `dtype`, looked at where it is about to be staged: everything
// finite, | |n| - 1 | <= 1e-6, f_des >= 0.  (A device array is taken as it is.)
int check_cmd_host(int dtype, int64_t B, const void* cmd) {
  static const char* const names[4] = {"nx", "ny", "nz", "f_des"};
  for (int64_t b = 0; b < B; b++) {
    double v[4];
    for (int k = 0; k < 4; k++) {
      const int64_t at = b * 4 + k;
      if (dtype == ABRK_F64) {
        memcpy(&v[k], static_cast<const char*>(cmd) + at * 8, 8);
      } else {
        float f;
        memcpy(&f, static_cast<const char*>(cmd) + at * 4, 4);
        v[k] = f;
      }
      if (!finite_at(&v[k])) return fail(ABRK_EINVAL, "cmd: row %lld: %s is not finite", (long long)b, names[k]);
    }
    if (v[3] < 0) return fail(ABRK_EINVAL, "cmd: row %lld: f_des=%g is negative", (long long)b, v[3]);
    const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(std::fabs(len - 1.0) <= 1e-6))
      return fail(ABRK_EINVAL, "cmd: row %lld: |n|=%.9g is not 1 to within 1e-6", (long long)b, len);
  }
  return 0;
}
}  // namespace

extern "C" int abrk_force_control_batch(int arm_id, int dtype, const abrk_force_params* P, int64_t B, const void* q,
                                        const void* dq, const void* target, const void* target_velocity,
                                        const void* cmd, const void* force, void* integ, void* u, int device,
                                        void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  if (!a->ops->force) return fail(ABRK_EINVAL, "this arm's kernels carry no force-control law (rebuild its plugin)");
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  const int n = a->desc.n_joints;
  if (P->frame < 0 || P->frame > 2 * n + 1) return fail(ABRK_EINVAL, "Invalid transformation name: frame id %d", P->frame);
  for (int r = 0; r < 3; r++)
    if (!finite_at(&P->off[r])) return fail(ABRK_EINVAL, "off[%d] is not finite", r);
  const struct {
    const char* name;
    const double* v;
  } nonneg[] = {{"kp", &P->kp},     {"kv", &P->kv},           {"kf", &P->kf},       {"ki", &P->ki},          {"i_max", &P->i_max},
                {"kvf", &P->kvf},   {"f_touch", &P->f_touch}, {"v_app", &P->v_app}, {"kv_null", &P->kv_null}};
  for (const auto& g : nonneg)
    if (!nonnegative_finite_at(g.v)) return fail(ABRK_EINVAL, "%s=%g is not a finite value >= 0", g.name, *g.v);
  if (!positive_finite_at(&P->dt)) return fail(ABRK_EINVAL, "dt=%g is not a finite value > 0", P->dt);
  if (P->force_ld < 3) return fail(ABRK_EINVAL, "force_ld=%d < 3", P->force_ld);
  if (!q || !dq || !target || !cmd || !force || !integ || !u)
    return fail(ABRK_EINVAL, "q, dq, target, cmd, force, integ and u are required");
  if (B == 0) return 0;
  if (!device_view(cmd))
    if (int rc = check_cmd_host(dtype, B, cmd)) return rc;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  ForceArgs fa{};
  st.in(&fa.q, q, (size_t)B * n * s);
  st.in(&fa.dq, dq, (size_t)B * n * s);
  st.in(&fa.target, target, (size_t)B * 6 * s);
  st.in(&fa.tv, target_velocity, (size_t)B * 6 * s);
  st.in(&fa.cmd, cmd, (size_t)B * 4 * s);
  st.in(&fa.force, force, (size_t)B * P->force_ld * s);
  st.inout(&fa.integ, integ, (size_t)B * s);
  // (accumulate: u goes in as well as out)
  st.bind(&fa.u, u, (size_t)B * n * s, P->accumulate != 0, true);
  if (int rc = st.reserve()) return rc;
  auto pb = blocks([&](auto t) { return make_forcep<decltype(t)>(*P, n); });
  return with_status_word(st, pb, nullptr, [&] { return launch_arm(st, a, dtype, B, &ArmOps::force, fa, pb); });
}

// ------------------------------------------------------------------------------- whole-arm contact
namespace {
static_assert(ABRK_LINK_CONTACT_MAX_OBSTACLES == kLinkContactMaxObstacles, "abrk.h and abrk_link_contact.h agree on the obstacles of a row");
static_assert(sizeof(((abrk_link_contact_params*)0)->link_radius) / sizeof(double) == kLinkContactMaxSegments,
              "abrk.h and abrk_link_contact.h agree on the segments of an arm");
template <class T>
LinkContactP<T> make_linkcontactp(const abrk_link_contact_params& P, int n) {
  LinkContactP<T> p;
  p.K = P.n_obstacles;
  for (int i = 0; i < kLinkContactMaxSegments; i++) p.radius[i] = i < n ? T(P.link_radius[i]) : T(-1);
  p.vs2 = T(P.vs * P.vs);
  p.accumulate = P.accumulate ? 1 : 0;
  return p;
}
// A host obstacle array [B, K, 7] = cx, cy, cz, R, k, c, mu of `dtype`, looked at where it is about to be staged:
// everything finite, R > 0, and k, c, mu >= 0.  (A device array is taken as it is.)
int check_obstacle_host(int dtype, int64_t B, int K, const void* obstacle) {
  static const char* const names[7] = {"cx", "cy", "cz", "R", "k", "c", "mu"};
  for (int64_t b = 0; b < B; b++)
    for (int o = 0; o < K; o++) {
      double v[7];
      for (int k = 0; k < 7; k++) {
        const int64_t at = (b * K + o) * 7 + k;
        if (dtype == ABRK_F64) {
          memcpy(&v[k], static_cast<const char*>(obstacle) + at * 8, 8);
        } else {
          float f;
          memcpy(&f, static_cast<const char*>(obstacle) + at * 4, 4);
          v[k] = f;  // (exact; an infinity or a NaN stays one)
        }
        if (!finite_at(&v[k]))
          return fail(ABRK_EINVAL, "obstacle: row %lld, obstacle %d: %s is not finite", (long long)b, o, names[k]);
        if (k == 3 && !positive_finite_at(&v[k]))
          return fail(ABRK_EINVAL, "obstacle: row %lld, obstacle %d: R=%g is not > 0", (long long)b, o, v[k]);
        if (k >= 4 && !nonnegative_finite_at(&v[k]))
          return fail(ABRK_EINVAL, "obstacle: row %lld, obstacle %d: %s=%g is negative", (long long)b, o, names[k], v[k]);
      }
    }
  return 0;
}
}  // namespace

extern "C" int abrk_link_contact_step_batch(int arm_id, int dtype, const abrk_link_contact_params* P, int64_t B,
                                            const void* q, const void* dq, const void* obstacle, void* tau, void* report,
                                            int device, void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  if (!a->ops->link_contact) return fail(ABRK_EINVAL, "this arm's kernels carry no link contact step (rebuild its plugin)");
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  const int n = a->desc.n_joints;
  if (P->n_obstacles < 1 || P->n_obstacles > ABRK_LINK_CONTACT_MAX_OBSTACLES)
    return fail(ABRK_EINVAL, "n_obstacles=%d outside 1..%d", P->n_obstacles, ABRK_LINK_CONTACT_MAX_OBSTACLES);
  if (!positive_finite_at(&P->vs)) return fail(ABRK_EINVAL, "vs=%g is not a finite value > 0", P->vs);
  bool any_on = false;
  for (int i = 0; i < n; i++) {
    if (!finite_at(&P->link_radius[i])) return fail(ABRK_EINVAL, "link_radius[%d] is not finite", i);
    any_on = any_on || P->link_radius[i] >= 0;
  }
  if (!any_on) return fail(ABRK_EINVAL, "every segment is switched off (link_radius < 0 for all %d)", n);
  if (!q || !dq || !obstacle || !tau) return fail(ABRK_EINVAL, "q, dq, obstacle and tau are required");
  if (B == 0) return 0;
  const int K = P->n_obstacles;
  if (!device_view(obstacle))
    if (int rc = check_obstacle_host(dtype, B, K, obstacle)) return rc;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  LinkContactArgs ca{};
  st.in(&ca.q, q, (size_t)B * n * s);
  st.in(&ca.dq, dq, (size_t)B * n * s);
  st.in(&ca.obstacle, obstacle, (size_t)B * K * 7 * s);
  // (accumulate: tau goes in as well as out)
  st.bind(&ca.tau, tau, (size_t)B * n * s, P->accumulate != 0, true);
  st.out(&ca.report, report, (size_t)B * 8 * s);
  if (int rc = st.reserve()) return rc;
  const auto pb = blocks([&](auto t) { return make_linkcontactp<decltype(t)>(*P, n); });
  return launch_arm(st, a, dtype, B, &ArmOps::link_contact, ca, pb);
}

// ------------------------------------------------------------------------------- path planner
namespace {
// the checks every path entry shares; -> PathArgs with the table fields set (the arrays are bound by the caller)
int check_path(const abrk_path_params* P, const void* table, const int64_t* off, int64_t B, PathArgs* out) {
  if (recording()) return fail(ABRK_EINVAL, "the path planning entry points cannot be recorded into a plan (abrk_path_next_batch can)");
  if (!P || !table || !off) return fail(ABRK_EINVAL, "params, table and offsets are required");
  if (B < 0 || B > 2147483647) return fail(ABRK_EINVAL, "batch %lld outside 0..2^31-1", (long long)B);
  if (P->n_samples < 2) return fail(ABRK_EINVAL, "n_samples=%d < 2", P->n_samples);
  if (P->n_candidates < 1 || P->n_candidates > 1 << 20) return fail(ABRK_EINVAL, "n_candidates=%d outside 1..2^20", P->n_candidates);
  if (!positive_finite_at(&P->dt)) return fail(ABRK_EINVAL, "dt=%g is not a positive finite step", P->dt);
  if (P->width != 6 && P->width != 12) return fail(ABRK_EINVAL, "width=%d is not 6 or 12", P->width);
  if (P->axes < 0 || P->axes > 31 || (P->axes & 3) == 3) return fail(ABRK_EINVAL, "axes code %d is none of the 24 sequences", P->axes);
  if (P->table_len < 0) return fail(ABRK_EINVAL, "negative table_len");
  const int64_t len = P->table_len, S = P->n_samples, K = P->n_candidates;
  auto inside = [&](int64_t o, int64_t n) { return o >= 0 && n >= 0 && o <= len && n <= len - o; };
  if (!inside(off[0], 3 * S)) return fail(ABRK_EINVAL, "offsets[0]: the sample table leaves the packed table");
  if (!inside(off[1], 3 * K)) return fail(ABRK_EINVAL, "offsets[1]: the candidate scalars leave the packed table");
  for (int64_t k = 0; k < K; k++) {
    const int64_t* o = off + 2 + 4 * k;
    if (!inside(o[0], o[1]) || !inside(o[2], o[3]) || o[1] > 1000000000 || o[3] > 1000000000)
      return fail(ABRK_EINVAL, "offsets: a ramp of candidate %lld leaves the packed table", (long long)k);
  }
  out->dt = P->dt;
  out->S = (int)S;
  out->K = (int)K;
  out->axes = P->axes;
  out->W = P->width;
  out->B = (long)B;
  return 0;
}
}  // namespace

extern "C" int abrk_path_plan_batch(const abrk_path_params* P, const void* table, const int64_t* offsets, int64_t B,
                                    const void* start, const void* target, void* n_timesteps, void* rowplan,
                                    void* dist_steps, int device, void* stream) {
  PathArgs pa{};
  if (int rc = check_path(P, table, offsets, B, &pa)) return rc;
  if (!start || !target || !n_timesteps || !rowplan || !dist_steps)
    return fail(ABRK_EINVAL, "start, target, n_timesteps, rowplan and dist_steps are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  Stager st{device, (hipStream_t)stream};
  st.in((const void**)&pa.tab, table, (size_t)P->table_len * 8);
  st.in((const void**)&pa.off, offsets, (size_t)(2 + 4 * (size_t)pa.K) * 8);
  st.in((const void**)&pa.start, start, (size_t)B * 24);
  st.in((const void**)&pa.target, target, (size_t)B * 24);
  st.out((void**)&pa.n_timesteps, n_timesteps, (size_t)B * 4);
  st.out((void**)&pa.rowplan, rowplan, (size_t)B * 8);
  st.out((void**)&pa.dist_steps, dist_steps, (size_t)B * pa.S * 8);
  if (int rc = st.reserve()) return rc;
  // anything staged (as a rule the offsets, which live on the host): the call is synchronous and reports a row without
  // a path itself, on the calling thread's word; device-visible memory throughout: the stream's next sync does
  StatusWord* sw = status_word(st.staged, device, stream);
  pa.status = sw ? sw->path_dev() : nullptr;
  if (sw && st.staged) *sw->path_host() = 0;
  HIPCHK(launch_path_plan(pa, (hipStream_t)stream));
  if (int rc = st.finish()) return rc;
  return st.staged && sw && sw->take_path() ? path_error() : 0;
}

extern "C" int abrk_path_fill_batch(const abrk_path_params* P, const void* table, const int64_t* offsets, int64_t B,
                                    int32_t t_max, const void* start, const void* target,
                                    const void* start_orientation, const void* target_orientation,
                                    const void* n_timesteps, const void* rowplan, const void* dist_steps, void* path,
                                    int device, void* stream) {
  PathArgs pa{};
  if (int rc = check_path(P, table, offsets, B, &pa)) return rc;
  if (t_max < 1) return fail(ABRK_EINVAL, "t_max=%d < 1", t_max);
  if (!start || !target || !n_timesteps || !rowplan || !dist_steps || !path)
    return fail(ABRK_EINVAL, "start, target, n_timesteps, rowplan, dist_steps and path are required");
  if (P->width == 12 && (!start_orientation || !target_orientation))
    return fail(ABRK_EINVAL, "a 12-wide path needs start_orientation and target_orientation");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const bool ori = P->width == 12;
  Stager st{device, (hipStream_t)stream};
  st.in((const void**)&pa.tab, table, (size_t)P->table_len * 8);
  st.in((const void**)&pa.off, offsets, (size_t)(2 + 4 * (size_t)pa.K) * 8);
  st.in((const void**)&pa.start, start, (size_t)B * 24);
  st.in((const void**)&pa.target, target, (size_t)B * 24);
  st.in((const void**)&pa.start_o, ori ? start_orientation : nullptr, (size_t)B * 24);
  st.in((const void**)&pa.target_o, ori ? target_orientation : nullptr, (size_t)B * 24);
  st.in((const void**)&pa.n_timesteps, n_timesteps, (size_t)B * 4);
  st.in((const void**)&pa.rowplan, rowplan, (size_t)B * 8);
  st.in((const void**)&pa.dist_steps, dist_steps, (size_t)B * pa.S * 8);
  st.out((void**)&pa.path, path, (size_t)B * t_max * P->width * 8);
  if (int rc = st.reserve()) return rc;
  pa.Tmax = t_max;
  HIPCHK(launch_path_fill(pa, (hipStream_t)stream));
  HIPCHK(launch_path_gradient(pa, (hipStream_t)stream));
  return st.finish();
}

extern "C" int abrk_path_next_batch(int dtype, int64_t B, int32_t t_max, int32_t width, const void* path,
                                    const void* n_timesteps, void* counter, void* target, void* target_velocity,
                                    int device, void* stream) {
  if (int rc = check_batch(dtype, B)) return rc;
  if (t_max < 1) return fail(ABRK_EINVAL, "t_max=%d < 1", t_max);
  if (width != 6 && width != 12) return fail(ABRK_EINVAL, "width=%d is not 6 or 12", width);
  if (!path || !n_timesteps || !counter || !target) return fail(ABRK_EINVAL, "path, n_timesteps, counter and target are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  PathNextArgs na{};
  st.in((const void**)&na.path, path, (size_t)B * t_max * width * 8);
  st.in((const void**)&na.n_timesteps, n_timesteps, (size_t)B * 4);
  st.inout((void**)&na.counter, counter, (size_t)B * 4);
  // a 6-wide path leaves the orientation columns as they are: the arrays go in as well as out
  st.inout(&na.target, target, (size_t)B * 6 * s);
  st.inout(&na.target_velocity, target_velocity, (size_t)B * 6 * s);
  if (int rc = st.reserve()) return rc;
  na.B = (long)B;
  na.Tmax = t_max;
  na.W = width;
  const hipStream_t hs = (hipStream_t)stream;
  return dispatch(st, nullptr, dtype, [=](const void*) { return launch_path_next(dtype, na, hs); });
}

// ------------------------------------------------------------------------------- adaptive signal
namespace {
template <class T>
AdaptArgs<T> make_adapt_args(const abrk_adapt_params& P, int64_t B, int w0, int w1) {
  return adapt_make_args<T>(P.n_input, P.n_output, P.n_neurons_total, P.n_per_ensemble, w0, w1, (long)B, P.dt, P.tau_input,
                            P.tau_training, P.tau_output, P.tau_rc, P.tau_ref, P.pes_learning_rate);
}
}  // namespace

extern "C" int abrk_adapt_step_batch(int dtype, const abrk_adapt_params* P, int64_t B, const void* enc, const void* gain,
                                     const void* bias, const void* shift, const void* scale, const void* in0, int32_t w0,
                                     const void* in1, int32_t w1, const void* training, const abrk_adapt_state* S,
                                     void* out, void* u_add, int device, void* stream) {
  if (int rc = check_batch(dtype, B)) return rc;
  if (!P || !S) return fail(ABRK_EINVAL, "params and state are required");
  if (B > 2147483647) return fail(ABRK_EINVAL, "batch %lld outside 0..2^31-1", (long long)B);
  if (P->neuron_type != ABRK_ADAPT_LIF && P->neuron_type != ABRK_ADAPT_LIF_RATE)
    return fail(ABRK_EINVAL, "neuron_type %d is not ABRK_ADAPT_LIF/ABRK_ADAPT_LIF_RATE", P->neuron_type);
  if (P->n_input < 1 || P->n_input > ABRK_ADAPT_MAX_INPUT)
    return fail(ABRK_EINVAL, "n_input=%d outside 1..%d", P->n_input, ABRK_ADAPT_MAX_INPUT);
  if (P->n_output < 1 || P->n_output > ABRK_ADAPT_MAX_OUTPUT)
    return fail(ABRK_EINVAL, "n_output=%d outside 1..%d", P->n_output, ABRK_ADAPT_MAX_OUTPUT);
  if (P->n_neurons_total < 1) return fail(ABRK_EINVAL, "n_neurons_total=%d < 1", P->n_neurons_total);
  if (P->n_per_ensemble < 1) return fail(ABRK_EINVAL, "n_per_ensemble=%d < 1", P->n_per_ensemble);
  if ((int64_t)P->n_neurons_total * P->n_output > 2147483647)
    return fail(ABRK_EINVAL, "n_neurons_total * n_output = %lld weights per row exceed 2^31-1",
                (long long)P->n_neurons_total * P->n_output);
  if (w0 < 1 || w1 < 0 || (int64_t)w0 + w1 != P->n_input)
    return fail(ABRK_EINVAL, "input widths %d + %d do not make n_input=%d", w0, w1, P->n_input);
  if (!positive_finite_at(&P->dt)) return fail(ABRK_EINVAL, "dt=%g is not a positive finite step", P->dt);
  if (!positive_finite_at(&P->tau_rc)) return fail(ABRK_EINVAL, "tau_rc=%g is not positive and finite", P->tau_rc);
  if (!nonnegative_finite_at(&P->tau_ref) || !nonnegative_finite_at(&P->tau_input) ||
      !nonnegative_finite_at(&P->tau_training) || !nonnegative_finite_at(&P->tau_output) ||
      !nonnegative_finite_at(&P->pes_learning_rate))
    return fail(ABRK_EINVAL, "a time constant or pes_learning_rate is negative or not finite");
  const bool lif = P->neuron_type == ABRK_ADAPT_LIF;
  if (!enc || !gain || !bias || !shift || !scale) return fail(ABRK_EINVAL, "enc, gain, bias, shift and scale are required");
  if (!in0 || (w1 > 0 && !in1)) return fail(ABRK_EINVAL, "in0 is required, and in1 when w1 > 0");
  if (!training || !out) return fail(ABRK_EINVAL, "training and out are required");
  if (!S->x_f || !S->e_f || !S->a_f || !S->W || !S->out_f || (lif && (!S->v || !S->ref)))
    return fail(ABRK_EINVAL, "a state array is NULL (x_f, e_f, a_f, W, out_f; v and ref for ABRK_ADAPT_LIF)");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype), D = (size_t)P->n_input, O = (size_t)P->n_output, N = (size_t)P->n_neurons_total;
  const int type = lif ? kAdaptLif : kAdaptLifRate;
  const hipStream_t hs = (hipStream_t)stream;
  // the arrays are bound straight into the typed block of the call's arithmetic type
  const auto run = [&](auto t) -> int {
    AdaptArgs<decltype(t)> a = make_adapt_args<decltype(t)>(*P, B, w0, w1);
    Stager st{device, hs};
    st.in((const void**)&a.enc, enc, N * D * s);
    st.in((const void**)&a.gain, gain, N * s);
    st.in((const void**)&a.bias, bias, N * s);
    st.in((const void**)&a.shift, shift, D * s);
    st.in((const void**)&a.scale, scale, D * s);
    st.in((const void**)&a.in0, in0, (size_t)B * w0 * s);
    st.in((const void**)&a.in1, w1 > 0 ? in1 : nullptr, (size_t)B * w1 * s);
    st.in((const void**)&a.training, training, (size_t)B * O * s);
    st.inout((void**)&a.x_f, S->x_f, (size_t)B * D * s);
    st.inout((void**)&a.e_f, S->e_f, (size_t)B * O * s);
    st.inout((void**)&a.v, lif ? S->v : nullptr, (size_t)B * N * s);
    st.inout((void**)&a.ref, lif ? S->ref : nullptr, (size_t)B * N * s);
    st.inout((void**)&a.a_f, S->a_f, (size_t)B * N * s);
    st.inout((void**)&a.W, S->W, (size_t)B * O * N * s);
    st.inout((void**)&a.out_f, S->out_f, (size_t)B * O * s);
    st.out((void**)&a.out, out, (size_t)B * O * s);
    st.inout((void**)&a.u_add, u_add, (size_t)B * O * s);
    if (int rc = st.reserve()) return rc;
    return dispatch(st, nullptr, dtype, [=](const void*) { return launch_adapt_step(type, a, hs); });
  };
  return dtype == ABRK_F64 ? run(0.0) : run(0.0f);
}

// ------------------------------------------------------------------------------- measurement channel
extern "C" int abrk_channel_step_batch(int dtype, const abrk_channel_params* P, int64_t B, const void* in0, int32_t w0,
                                       const void* in1, int32_t w1, void* out0, void* out1, void* dy,
                                       const abrk_channel_state* S, int device, void* stream) {
  if (int rc = check_batch(dtype, B)) return rc;
  if (!P || !S) return fail(ABRK_EINVAL, "params and state are required");
  if (B > 2147483647) return fail(ABRK_EINVAL, "batch %lld outside 0..2^31-1", (long long)B);
  if (P->width < 1 || P->width > ABRK_CHANNEL_MAX_WIDTH)
    return fail(ABRK_EINVAL, "width=%d outside 1..%d", P->width, ABRK_CHANNEL_MAX_WIDTH);
  if (P->delay < 0 || P->delay > ABRK_CHANNEL_MAX_DELAY)
    return fail(ABRK_EINVAL, "delay=%d outside 0..%d", P->delay, ABRK_CHANNEL_MAX_DELAY);
  if (w0 < 1 || w1 < 0 || (int64_t)w0 + w1 != P->width)
    return fail(ABRK_EINVAL, "widths %d + %d do not make width=%d", w0, w1, P->width);
  if (w1 > 0 && (!in1 || !out1)) return fail(ABRK_EINVAL, "in1 and out1 are required when w1 > 0");
  for (int c = 0; c < P->width; c++) {
    if (!nonnegative_finite_at(&P->sigma[c])) return fail(ABRK_EINVAL, "sigma[%d] is negative or not finite", c);
    if (!nonnegative_finite_at(&P->resolution[c])) return fail(ABRK_EINVAL, "resolution[%d] is negative or not finite", c);
    if (!finite_at(&P->bias[c])) return fail(ABRK_EINVAL, "bias[%d] is not finite", c);
  }
  if (!positive_finite_at(&P->dt)) return fail(ABRK_EINVAL, "dt=%g is not a positive finite step", P->dt);
  if (dy && !nonnegative_finite_at(&P->tau_diff)) return fail(ABRK_EINVAL, "tau_diff=%g is negative or not finite", P->tau_diff);
  if (!in0 || !out0) return fail(ABRK_EINVAL, "in0 and out0 are required");
  if (!S->counter) return fail(ABRK_EINVAL, "counter is NULL");
  if (P->delay > 0 && !S->ring) return fail(ABRK_EINVAL, "delay=%d needs the ring", P->delay);
  if (dy && (!S->prev || !S->d_f)) return fail(ABRK_EINVAL, "dy needs prev and d_f");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype), W = (size_t)P->width;
  const hipStream_t hs = (hipStream_t)stream;
  // the arrays are bound straight into the typed block of the call's arithmetic type
  const auto run = [&](auto t) -> int {
    ChannelArgs<decltype(t)> a = channel_make_args<decltype(t)>(w0, w1, P->delay, (long)B, P->seed, P->row_offset, P->dt,
                                                                P->tau_diff, P->bias, P->sigma, P->resolution);
    Stager st{device, hs};
    st.in((const void**)&a.in0, in0, (size_t)B * w0 * s);
    st.in((const void**)&a.in1, w1 > 0 ? in1 : nullptr, (size_t)B * w1 * s);
    st.out((void**)&a.out0, out0, (size_t)B * w0 * s);
    st.out((void**)&a.out1, w1 > 0 ? out1 : nullptr, (size_t)B * w1 * s);
    st.out((void**)&a.dy, dy, (size_t)B * W * s);
    st.inout((void**)&a.counter, S->counter, (size_t)B * 4);
    st.inout((void**)&a.ring, P->delay > 0 ? S->ring : nullptr, ((size_t)P->delay + 1) * B * W * s);
    st.inout((void**)&a.prev, dy ? S->prev : nullptr, (size_t)B * W * s);
    st.inout((void**)&a.d_f, dy ? S->d_f : nullptr, (size_t)B * W * s);
    if (int rc = st.reserve()) return rc;
    return dispatch(st, nullptr, dtype, [=](const void*) { return launch_channel_step(a, hs); });
  };
  return dtype == ABRK_F64 ? run(0.0) : run(0.0f);
}

// hostsim_force.cpp - TEST AID ONLY.  The row program of the force-control law (abr_control_amd/csrc abrk_force.h
// force_body: exactly what one GPU lane executes) compiled for the HOST on one arm table, so that the law can be checked
// against the NumPy reference without a GPU.  Built per table by tests/hostsim_force/__init__.py like
// tests/hostsim_contact: a compile-time table comes in through `-include` and its name through HOSTSIM_FORCE_TAB; a
// runtime table is built with HOSTSIM_FORCE_RT_N = its joint count and takes the arm description with every call.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_force.h"
#include "../../abr_control_amd/csrc/abrk_rt.h"
#include "../../include/abrk.h"

using namespace abrk;

namespace {
template <class A, class T>
int run(const A& arm, const abrk_force_params* S, int64_t B, const void* q, const void* dq, const void* target,
        const void* tv, const void* cmd, const void* force, void* integ, void* u, int* status) {
  if (!S || S->frame < 0 || S->frame > 2 * A::N + 1 || S->force_ld < 3) return -5;
  ForceP<T> P;
  P.frame = S->frame;
  P.m = frame_joints(S->frame, A::N);
  for (int r = 0; r < 3; r++) P.off[r] = T(S->off[r]);
  P.kp = T(S->kp);
  P.kv = T(S->kv);
  P.kf = T(S->kf);
  P.ki = T(S->ki);
  P.i_max = T(S->i_max);
  P.kvf = T(S->kvf);
  P.f_touch = T(S->f_touch);
  P.v_app = T(S->v_app);
  P.kv_null = T(S->kv_null);
  P.dt = T(S->dt);
  P.use_g = S->use_g ? 1 : 0;
  P.accumulate = S->accumulate ? 1 : 0;
  P.force_ld = S->force_ld;
  P.status = status;
  const ForceIO<T> io{(const T*)q,   (const T*)dq,    (const T*)target, (const T*)tv,
                      (const T*)cmd, (const T*)force, (T*)integ,        (T*)u};
  for (long b = 0; b < B; b++) force_body<A, T>(b, arm, P, io);
  return 0;
}
}  // namespace

#if defined(HOSTSIM_FORCE_RT_N)
constexpr int kN = HOSTSIM_FORCE_RT_N;
extern "C" int hostsim_force_n(void) { return kN; }
extern "C" int hostsim_force(const abrk_arm_desc* d, int dtype, const abrk_force_params* S, int64_t B, const void* q,
                             const void* dq, const void* target, const void* tv, const void* cmd, const void* force,
                             void* integ, void* u, int* status) {
  if (!d || d->n_joints != kN) return -4;
  if (dtype == 0) {
    RtArm<kN, double> a;
    rt_fill<kN, double>(d, &a);
    return run<RtArm<kN, double>, double>(a, S, B, q, dq, target, tv, cmd, force, integ, u, status);
  }
  RtArm<kN, float> a;
  rt_fill<kN, float>(d, &a);
  return run<RtArm<kN, float>, float>(a, S, B, q, dq, target, tv, cmd, force, integ, u, status);
}
#else
using Arm = StaticArm<HOSTSIM_FORCE_TAB>;
extern "C" int hostsim_force_n(void) { return Arm::N; }
extern "C" int hostsim_force(const abrk_arm_desc*, int dtype, const abrk_force_params* S, int64_t B, const void* q,
                             const void* dq, const void* target, const void* tv, const void* cmd, const void* force,
                             void* integ, void* u, int* status) {
  Arm a;
  return dtype == 0 ? run<Arm, double>(a, S, B, q, dq, target, tv, cmd, force, integ, u, status)
                    : run<Arm, float>(a, S, B, q, dq, target, tv, cmd, force, integ, u, status);
}
#endif

// hostsim_contact.cpp - TEST AID ONLY.  The row program of the end-effector contact (abr_control_amd/csrc
// abrk_contact.h contact_body: exactly what one GPU lane executes) compiled for the HOST on one arm table, so that the
// contact law can be checked against the NumPy reference without a GPU.  Built per table by
// tests/hostsim_contact/__init__.py like tests/hostsim_payload: a compile-time table comes in through `-include` and its
// name through HOSTSIM_CONTACT_TAB; a runtime table is built with HOSTSIM_CONTACT_RT_N = its joint count and takes the arm
// description with every call.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_contact.h"
#include "../../abr_control_amd/csrc/abrk_rt.h"

using namespace abrk;

namespace {
template <class A, class T>
int run(const A& arm, int frame, const double* off, int S, double vs, int accumulate, int64_t B, const void* q,
        const void* dq, const void* surface, void* tau, void* report) {
  if (S < 1 || S > kContactMaxSurfaces || frame < 0 || frame > 2 * A::N + 1) return -5;
  ContactP<T> P;
  P.frame = frame;
  P.m = frame_joints(frame, A::N);
  for (int r = 0; r < 3; r++) P.off[r] = T(off[r]);
  P.S = S;
  P.vs2 = T(vs * vs);
  P.accumulate = accumulate;
  const ContactIO<T> io{(const T*)q, (const T*)dq, (const T*)surface, (T*)tau, (T*)report};
  for (long b = 0; b < B; b++) contact_body<A, T>(b, arm, P, io);
  return 0;
}
}  // namespace

#if defined(HOSTSIM_CONTACT_RT_N)
constexpr int kN = HOSTSIM_CONTACT_RT_N;
extern "C" int hostsim_contact_n(void) { return kN; }
extern "C" int hostsim_contact(const abrk_arm_desc* d, int dtype, int frame, const double* off, int S, double vs,
                               int accumulate, int64_t B, const void* q, const void* dq, const void* surface, void* tau,
                               void* report) {
  if (!d || d->n_joints != kN) return -4;
  if (dtype == 0) {
    RtArm<kN, double> a;
    rt_fill<kN, double>(d, &a);
    return run<RtArm<kN, double>, double>(a, frame, off, S, vs, accumulate, B, q, dq, surface, tau, report);
  }
  RtArm<kN, float> a;
  rt_fill<kN, float>(d, &a);
  return run<RtArm<kN, float>, float>(a, frame, off, S, vs, accumulate, B, q, dq, surface, tau, report);
}
#else
using Arm = StaticArm<HOSTSIM_CONTACT_TAB>;
extern "C" int hostsim_contact_n(void) { return Arm::N; }
extern "C" int hostsim_contact(const abrk_arm_desc*, int dtype, int frame, const double* off, int S, double vs,
                               int accumulate, int64_t B, const void* q, const void* dq, const void* surface, void* tau,
                               void* report) {
  Arm a;
  return dtype == 0 ? run<Arm, double>(a, frame, off, S, vs, accumulate, B, q, dq, surface, tau, report)
                    : run<Arm, float>(a, frame, off, S, vs, accumulate, B, q, dq, surface, tau, report);
}
#endif

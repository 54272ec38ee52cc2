// hostsim_link_contact.cpp - TEST AID ONLY.  The row program of the whole-arm contact (abr_control_amd/csrc
// abrk_link_contact.h link_contact_body: exactly what one GPU lane executes) compiled for the HOST on one arm table, so
// that the law can be checked against the NumPy reference without a GPU.  Built per table by
// tests/hostsim_link_contact/__init__.py like tests/hostsim_force: a compile-time table comes in through `-include` and
// its name through HOSTSIM_LINK_CONTACT_TAB; a runtime table is built with HOSTSIM_LINK_CONTACT_RT_N = its joint count
// and takes the arm description with every call.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_link_contact.h"
#include "../../abr_control_amd/csrc/abrk_rt.h"

using namespace abrk;

namespace {
template <class A, class T>
int run(const A& arm, int K, const double* radius, double vs, int accumulate, int64_t B, const void* q, const void* dq,
        const void* obstacle, void* tau, void* report) {
  if (K < 1 || K > kLinkContactMaxObstacles) return -5;
  LinkContactP<T> P;
  P.K = K;
  for (int i = 0; i < kLinkContactMaxSegments; i++) P.radius[i] = i < A::N ? T(radius[i]) : T(-1);
  P.vs2 = T(vs * vs);
  P.accumulate = accumulate;
  const LinkContactIO<T> io{(const T*)q, (const T*)dq, (const T*)obstacle, (T*)tau, (T*)report};
  for (long b = 0; b < B; b++) link_contact_body<A, T>(b, arm, P, io);
  return 0;
}
}  // namespace

#if defined(HOSTSIM_LINK_CONTACT_RT_N)
constexpr int kN = HOSTSIM_LINK_CONTACT_RT_N;
extern "C" int hostsim_link_contact_n(void) { return kN; }
extern "C" int hostsim_link_contact(const abrk_arm_desc* d, int dtype, int K, const double* radius, double vs,
                                    int accumulate, int64_t B, const void* q, const void* dq, const void* obstacle,
                                    void* tau, void* report) {
  if (!d || d->n_joints != kN) return -4;
  if (dtype == 0) {
    RtArm<kN, double> a;
    rt_fill<kN, double>(d, &a);
    return run<RtArm<kN, double>, double>(a, K, radius, vs, accumulate, B, q, dq, obstacle, tau, report);
  }
  RtArm<kN, float> a;
  rt_fill<kN, float>(d, &a);
  return run<RtArm<kN, float>, float>(a, K, radius, vs, accumulate, B, q, dq, obstacle, tau, report);
}
#else
using Arm = StaticArm<HOSTSIM_LINK_CONTACT_TAB>;
extern "C" int hostsim_link_contact_n(void) { return Arm::N; }
extern "C" int hostsim_link_contact(const abrk_arm_desc*, int dtype, int K, const double* radius, double vs,
                                    int accumulate, int64_t B, const void* q, const void* dq, const void* obstacle,
                                    void* tau, void* report) {
  Arm a;
  return dtype == 0 ? run<Arm, double>(a, K, radius, vs, accumulate, B, q, dq, obstacle, tau, report)
                    : run<Arm, float>(a, K, radius, vs, accumulate, B, q, dq, obstacle, tau, report);
}
#endif

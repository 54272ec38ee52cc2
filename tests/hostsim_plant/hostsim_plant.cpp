// hostsim_plant.cpp - TEST AID ONLY.  The plant row program of abr_control_amd/csrc (abrk_ctrl.h plant_row, through
// abrk_rows.h plant_body: exactly what one GPU lane executes) compiled for the HOST on one arm table, so that forward
// dynamics and the Euler steps can be checked against the oracle without a GPU.  Built per table by
// tests/hostsim_plant/__init__.py: a compile-time table comes in through `-include` (rendered by
// abr_control_amd/_abi.py render_tab_struct) and its name through HOSTSIM_PLANT_TAB; a runtime table is built with
// HOSTSIM_PLANT_RT_N = its joint count and takes the arm description with every call.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_rows.h"
#include "../../abr_control_amd/csrc/abrk_rt.h"

using namespace abrk;

namespace {
template <class A, class T>
int run(const A& arm, int mode, double dt, int substeps, int gravity, int64_t B, void* q, void* dq, const void* u,
        void* ddq) {
  int status = 0;
  PlantP<T> P;
  P.h = T(dt / substeps);
  P.substeps = substeps;
  P.gravity = gravity;
  P.mode = mode;
  P.status = &status;
  for (long b = 0; b < B; b++) {
    RegScratch<T, A::N> scr;
    plant_body<A, T>(b, arm, P, (T*)q, (T*)dq, (const T*)u, (T*)ddq, scr);
  }
  return status;  // 1: some row met a non-positive pivot
}
}  // namespace

#if defined(HOSTSIM_PLANT_RT_N)
constexpr int kN = HOSTSIM_PLANT_RT_N;
extern "C" int hostsim_plant_n(void) { return kN; }
extern "C" int hostsim_plant(const abrk_arm_desc* d, int dtype, int mode, double dt, int substeps, int gravity, int64_t B,
                             void* q, void* dq, const void* u, void* ddq) {
  if (!d || d->n_joints != kN) return -4;
  if (dtype == 0) {
    RtArm<kN, double> a;
    rt_fill<kN, double>(d, &a);
    return run<RtArm<kN, double>, double>(a, mode, dt, substeps, gravity, B, q, dq, u, ddq);
  }
  RtArm<kN, float> a;
  rt_fill<kN, float>(d, &a);
  return run<RtArm<kN, float>, float>(a, mode, dt, substeps, gravity, B, q, dq, u, ddq);
}
#else
using Arm = StaticArm<HOSTSIM_PLANT_TAB>;
extern "C" int hostsim_plant_n(void) { return Arm::N; }
extern "C" int hostsim_plant(const abrk_arm_desc*, int dtype, int mode, double dt, int substeps, int gravity, int64_t B,
                             void* q, void* dq, const void* u, void* ddq) {
  Arm a;
  return dtype == 0 ? run<Arm, double>(a, mode, dt, substeps, gravity, B, q, dq, u, ddq)
                    : run<Arm, float>(a, mode, dt, substeps, gravity, B, q, dq, u, ddq);
}
#endif

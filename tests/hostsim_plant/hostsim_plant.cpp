// hostsim_plant.cpp - TEST AID ONLY.  The two plant row programs of abr_control_amd/csrc (abrk_ctrl.h plant_row and
// plant_fx_row, through abrk_rows.h plant_body and plant_fx_body: exactly what one GPU lane executes) compiled for the
// HOST on one arm table, so that forward dynamics, the Euler steps, friction, saturation, loads and joint limits can be
// checked against the oracle and the NumPy reference without a GPU.  Built per table by tests/hostsim_plant/__init__.py:
// a compile-time table comes in through `-include` (rendered by abr_control_amd/_abi.py render_tab_struct) and its name
// through HOSTSIM_PLANT_TAB; a runtime table is built with HOSTSIM_PLANT_RT_N = its joint count and takes the arm
// description with every call.
// `plain` != 0 runs plant_body (fx, tau_ext and wrench ignored), else plant_fx_body: the two row programs side by side
// in one build.  With HOSTSIM_PLANT_PLAIN_ONLY the build holds plant_body alone (plant_fx_body is not instantiated) and
// refuses `plain` == 0.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_params.h"
#include "../../abr_control_amd/csrc/abrk_rows.h"
#include "../../abr_control_amd/csrc/abrk_rt.h"

using namespace abrk;

namespace {
template <class A, class T>
int run(const A& arm, int plain, int mode, double dt, int substeps, int gravity, const abrk_plant_effects* fx, int64_t B,
        void* q, void* dq, const void* u, const void* ext, const void* w, void* ddq) {
  int status = 0;
  PlantP<T> P;
  P.h = T(dt / substeps);
  P.substeps = substeps;
  P.gravity = gravity;
  P.mode = mode;
  P.status = &status;
#if defined(HOSTSIM_PLANT_PLAIN_ONLY)
  if (!plain) return -5;
  for (long b = 0; b < B; b++) {
    RegScratch<T, A::N> scr;
    plant_body<A, T>(b, arm, P, (T*)q, (T*)dq, (const T*)u, (T*)ddq, scr);
  }
#else
  const PlantFxP<T> F = make_plantfx<T>(fx, A::N, ext != nullptr, w != nullptr);
  for (long b = 0; b < B; b++) {
    RegScratch<T, A::N> scr;
    T tau[A::N];
    const FxPark<T> park{tau, 1};
    if (plain) plant_body<A, T>(b, arm, P, (T*)q, (T*)dq, (const T*)u, (T*)ddq, scr);
    else plant_fx_body<A, T>(b, arm, P, F.c, (T*)q, (T*)dq, (const T*)u, (const T*)ext, (const T*)w, (T*)ddq, park, scr);
  }
#endif
  return status;  // 1: some row met a non-positive pivot
}
}  // namespace

#if defined(HOSTSIM_PLANT_RT_N)
constexpr int kN = HOSTSIM_PLANT_RT_N;
extern "C" int hostsim_plant_n(void) { return kN; }
extern "C" int hostsim_plant(const abrk_arm_desc* d, int dtype, int plain, int mode, double dt, int substeps, int gravity,
                             const abrk_plant_effects* fx, int64_t B, void* q, void* dq, const void* u, const void* ext,
                             const void* w, void* ddq) {
  if (!d || d->n_joints != kN) return -4;
  if (dtype == 0) {
    RtArm<kN, double> a;
    rt_fill<kN, double>(d, &a);
    return run<RtArm<kN, double>, double>(a, plain, mode, dt, substeps, gravity, fx, B, q, dq, u, ext, w, ddq);
  }
  RtArm<kN, float> a;
  rt_fill<kN, float>(d, &a);
  return run<RtArm<kN, float>, float>(a, plain, mode, dt, substeps, gravity, fx, B, q, dq, u, ext, w, ddq);
}
#else
using Arm = StaticArm<HOSTSIM_PLANT_TAB>;
extern "C" int hostsim_plant_n(void) { return Arm::N; }
extern "C" int hostsim_plant(const abrk_arm_desc*, int dtype, int plain, int mode, double dt, int substeps, int gravity,
                             const abrk_plant_effects* fx, int64_t B, void* q, void* dq, const void* u, const void* ext,
                             const void* w, void* ddq) {
  Arm a;
  return dtype == 0 ? run<Arm, double>(a, plain, mode, dt, substeps, gravity, fx, B, q, dq, u, ext, w, ddq)
                    : run<Arm, float>(a, plain, mode, dt, substeps, gravity, fx, B, q, dq, u, ext, w, ddq);
}
#endif

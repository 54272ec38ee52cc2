// hostsim_plant_fx.cpp - TEST AID ONLY.  The row program of the plant with non-ideal effects (abrk_ctrl.h plant_fx_row,
// through abrk_rows.h plant_fx_body: exactly what one GPU lane executes) compiled for the HOST on one arm table, so that
// friction, saturation, loads and joint limits can be checked against the NumPy reference without a GPU.  Built per table
// by tests/hostsim_plant_fx/__init__.py exactly as tests/hostsim_plant builds the plain row program: a compile-time table
// comes in through `-include` and its name through HOSTSIM_PLANT_TAB; a runtime table is built with HOSTSIM_PLANT_RT_N.
// `plain` != 0 runs plant_body instead (fx, tau_ext and wrench ignored): the two row programs side by side in one build.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "../../abr_control_amd/csrc/abrk_rows.h"
#include "../../abr_control_amd/csrc/abrk_rt.h"
#include "../../include/abrk.h"

using namespace abrk;

namespace {
// abrk_host.cpp make_plantfx: an effect that is off becomes the constant that leaves the row as it is
template <class T>
PlantFxP<T> make_fx(const abrk_plant_effects* fx, int n, bool have_ext, bool have_w) {
  using F = PlantFxP<T>;
  F f{};
  const uint32_t flags = fx ? fx->flags : 0;
  const T big = std::numeric_limits<T>::max();
  for (int i = 0; i < n; i++) {
    f.c[F::DAMP + i] = (flags & ABRK_FX_VISCOUS) ? T(fx->damping[i]) : T(0);
    f.c[F::COUL + i] = (flags & ABRK_FX_COULOMB) ? T(fx->coulomb[i]) : T(0);
    f.c[F::TMAX + i] = (flags & ABRK_FX_SATURATION) ? T(fx->tau_max[i]) : big;
    f.c[F::QMIN + i] = (flags & ABRK_FX_LIMITS) ? T(fx->q_min[i]) : -big;
    f.c[F::QMAX + i] = (flags & ABRK_FX_LIMITS) ? T(fx->q_max[i]) : big;
  }
  f.c[F::VS2] = (flags & ABRK_FX_COULOMB) ? T(fx->coulomb_vs) * T(fx->coulomb_vs) : T(1);
  f.c[F::REST] = (flags & ABRK_FX_LIMITS) ? T(fx->restitution) : T(0);
  f.c[F::ON_EXT] = have_ext ? T(1) : T(0);
  f.c[F::ON_W] = have_w ? T(1) : T(0);
  return f;
}
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
  const PlantFxP<T> F = make_fx<T>(fx, A::N, ext != nullptr, w != nullptr);
  for (long b = 0; b < B; b++) {
    RegScratch<T, A::N> scr;
    T tau[A::N];
    const FxPark<T> park{tau, 1};
    if (plain) plant_body<A, T>(b, arm, P, (T*)q, (T*)dq, (const T*)u, (T*)ddq, scr);
    else plant_fx_body<A, T>(b, arm, P, F.c, (T*)q, (T*)dq, (const T*)u, (const T*)ext, (const T*)w, (T*)ddq, park, scr);
  }
  return status;  // 1: some row met a non-positive pivot
}
}  // namespace

#if defined(HOSTSIM_PLANT_RT_N)
constexpr int kN = HOSTSIM_PLANT_RT_N;
extern "C" int hostsim_plant_fx_n(void) { return kN; }
extern "C" int hostsim_plant_fx(const abrk_arm_desc* d, int dtype, int plain, int mode, double dt, int substeps,
                                int gravity, const abrk_plant_effects* fx, int64_t B, void* q, void* dq, const void* u,
                                const void* ext, const void* w, void* ddq) {
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
extern "C" int hostsim_plant_fx_n(void) { return Arm::N; }
extern "C" int hostsim_plant_fx(const abrk_arm_desc*, int dtype, int plain, int mode, double dt, int substeps,
                                int gravity, const abrk_plant_effects* fx, int64_t B, void* q, void* dq, const void* u,
                                const void* ext, const void* w, void* ddq) {
  Arm a;
  return dtype == 0 ? run<Arm, double>(a, plain, mode, dt, substeps, gravity, fx, B, q, dq, u, ext, w, ddq)
                    : run<Arm, float>(a, plain, mode, dt, substeps, gravity, fx, B, q, dq, u, ext, w, ddq);
}
#endif

// hostsim_gi.cpp - TEST AID ONLY.  The row programs of abr_control_amd/csrc compiled for the HOST on one
// general-inertia arm table (StaticArm<Tab>::kGI, the table a compiled plugin is instantiated on), so that the extra
// inertia terms of M, g, C and the Coriolis vector can be checked against the reference's fixtures without a GPU.
// Built per table by tests/hostsim_gi/__init__.py: the table struct comes in through `-include` (rendered by
// abr_control_amd/_abi.py render_tab_struct) and its name through HOSTSIM_GI_TAB.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_rows.h"

using namespace abrk;
using Arm = StaticArm<HOSTSIM_GI_TAB>;
static_assert(Arm::kGI, "hostsim_gi is built on general-inertia tables");

namespace {
template <class T>
int run_dyn(int64_t B, const void* q, const void* dq, int frame, uint32_t want, void* const* outs) {
  constexpr int N = Arm::N;
  DynOutP<T> o;
  T** po = reinterpret_cast<T**>(&o);
  for (int i = 0; i < 10; i++) po[i] = static_cast<T*>(outs[i]);
  const int m = frame_joints(frame, N);
  DirectStore<T> st;
  Arm arm;
  for (long b = 0; b < B; b++) {
    if (want & (W_C | W_DJ))
      dyn_body<Arm, T, true>(b, true, st, arm, frame, m, T(0), T(0), T(0), want, (long)B, (const T*)q, (const T*)dq, o);
    else
      dyn_body<Arm, T, false>(b, true, st, arm, frame, m, T(0), T(0), T(0), want, (long)B, (const T*)q, (const T*)dq,
                              o);
  }
  return 0;
}
// C(q, dq) dq as the fused OSC kernels of general-inertia arms accumulate it (CMODE_VEC)
template <class T>
int run_cvec(int64_t B, const void* qv, const void* dqv, void* out) {
  constexpr int N = Arm::N;
  Arm arm;
  for (long b = 0; b < B; b++) {
    T q[N], dq[N];
    load_row<N>((const T*)qv, b, q);
    load_row<N>((const T*)dqv, b, dq);
    Joints<Arm, T> jt;
    Dyn<Arm, T, CMODE_VEC> d;
    T XR[9], xo[3];
    NoCap nc;
    kin_dyn(arm, q, dq, jt, d, XR, xo, nc);
    store_row<N>((T*)out, b, d.cv);
  }
  return 0;
}
}  // namespace

extern "C" int hostsim_gi_n(void) { return Arm::N; }
extern "C" int hostsim_gi_dynamics(int dtype, int64_t B, const void* q, const void* dq, int frame, uint32_t want,
                                   void* const* outs) {
  return dtype == 0 ? run_dyn<double>(B, q, dq, frame, want, outs) : run_dyn<float>(B, q, dq, frame, want, outs);
}
extern "C" int hostsim_gi_cvec(int dtype, int64_t B, const void* q, const void* dq, void* out) {
  return dtype == 0 ? run_cvec<double>(B, q, dq, out) : run_cvec<float>(B, q, dq, out);
}

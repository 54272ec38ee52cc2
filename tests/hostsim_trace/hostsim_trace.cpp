// hostsim_trace.cpp - TEST AID ONLY.  The loop recorder's row program (abr_control_amd/csrc/abrk_trace.h trace_body with
// the row-per-lane store policy: what one GPU lane executes when its wavefront's rows do not share a slot) compiled for
// the HOST on one arm table, so that positions, errors, history slots and statistics can be checked without a GPU.
// Built per table by tests/hostsim_trace/__init__.py: a compile-time table comes in through `-include` (rendered by
// abr_control_amd/_abi.py render_tab_struct) and its name through HOSTSIM_TRACE_TAB; a runtime table is built with
// HOSTSIM_TRACE_RT_N = its joint count and takes the arm description with every call.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_trace.h"
#include "../../abr_control_amd/csrc/abrk_rt.h"

using namespace abrk;

namespace {
// one tick of B rows
template <class A, class T>
int run(const A& arm, int frame, const double* off, int every, int capacity, unsigned columns, double tol, int64_t B,
        const void* q, const void* dq, const void* u, const void* target, int* counter, void* history, double* stats,
        int* settle) {
  TraceP<T> P;
  P.frame = frame;
  for (int r = 0; r < 3; r++) P.off[r] = T(off[r]);
  P.every = every;
  P.capacity = capacity;
  P.columns = columns;
  P.W = trace_width(columns, A::N);
  P.lds = 0;
  P.tol = tol;
  const TraceIO<T> io{(const T*)q, (const T*)dq, (const T*)u, (const T*)target, counter, (T*)history, stats, settle};
  for (long b = 0; b < B; b++) {
    TraceDirect<T> st;
    trace_body<A, T>(b, true, st, arm, P, (long)B, io);
  }
  return 0;
}
}  // namespace

#if defined(HOSTSIM_TRACE_RT_N)
constexpr int kN = HOSTSIM_TRACE_RT_N;
extern "C" int hostsim_trace_n(void) { return kN; }
extern "C" int hostsim_trace(const abrk_arm_desc* d, int dtype, int frame, const double* off, int every, int capacity,
                             unsigned columns, double tol, int64_t B, const void* q, const void* dq, const void* u,
                             const void* target, int* counter, void* history, double* stats, int* settle) {
  if (!d || d->n_joints != kN) return -4;
  if (dtype == 0) {
    RtArm<kN, double> a;
    rt_fill<kN, double>(d, &a);
    return run<RtArm<kN, double>, double>(a, frame, off, every, capacity, columns, tol, B, q, dq, u, target, counter,
                                          history, stats, settle);
  }
  RtArm<kN, float> a;
  rt_fill<kN, float>(d, &a);
  return run<RtArm<kN, float>, float>(a, frame, off, every, capacity, columns, tol, B, q, dq, u, target, counter, history,
                                      stats, settle);
}
#else
using Arm = StaticArm<HOSTSIM_TRACE_TAB>;
extern "C" int hostsim_trace_n(void) { return Arm::N; }
extern "C" int hostsim_trace(const abrk_arm_desc*, int dtype, int frame, const double* off, int every, int capacity,
                             unsigned columns, double tol, int64_t B, const void* q, const void* dq, const void* u,
                             const void* target, int* counter, void* history, double* stats, int* settle) {
  Arm a;
  return dtype == 0 ? run<Arm, double>(a, frame, off, every, capacity, columns, tol, B, q, dq, u, target, counter,
                                       history, stats, settle)
                    : run<Arm, float>(a, frame, off, every, capacity, columns, tol, B, q, dq, u, target, counter,
                                      history, stats, settle);
}
#endif

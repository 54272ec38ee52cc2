// Law-only OSC kernels (caller-supplied J, M, g, ...) for 1..7 joints, both arithmetic types.
#include "abrk_finish.h"
namespace abrk {
template <int N, class T>
static hipError_t law_launch(const LaunchArgs& la, const LawArgs& a) {
  hipLaunchKernelGGL((osc_law_kernel<N, T>), grid_for(la.B), dim3(kBlock), 0, la.stream,
                     *static_cast<const OscP<T>*>(a.P), la.B, (const T*)a.J, (const T*)a.M, (const T*)a.g,
                     (const T*)a.c, (const T*)a.xyz, (const T*)a.R, (const T*)a.q, (const T*)a.dq, (const T*)a.target,
                     (const T*)a.tv, (T*)a.ierr, (const T*)a.une, (T*)a.u, (T*)a.ts);
  return hipGetLastError();
}
hipError_t launch_osc_law(int n, int dtype, const LaunchArgs& la, const LawArgs& a) {
  return for_joints_and_dtype(
      n, dtype, [&](auto nn, auto t) { return law_launch<nn(), decltype(t)>(la, a); }, hipErrorInvalidValue);
}
// ---- finish kernels of the six-row law's hand-over forms (abrk_finish.h), launched as the plan says
template <int N, class T>
static hipError_t finish_launch(const LaunchArgs& la, const FinishArgs& a) {
  const unsigned nchunk = (unsigned)((la.B + kBlock - 1) / kBlock);
  const auto* masks = (const unsigned long long*)a.masks;
  switch (a.plan.form) {
    case Osc6Form::HandoverDense:
      hipLaunchKernelGGL((osc6_finish_dense_kernel<N, T>), dim3((nchunk + kBlock - 1) / kBlock, 4u), dim3(kBlock), 0,
                         la.stream, masks, (const T*)a.rec, a.nulls, (long)nchunk, la.B, (T*)a.u, (T*)a.ts);
      break;
    case Osc6Form::HandoverGroup: {
      // four wavefronts per chunk; a group with more than rounds x its wavefronts goes one record per lane
      const int gc = a.plan.group, wg = 4 * gc;
      hipLaunchKernelGGL((osc6_finish_group_kernel<N, T>), dim3((nchunk + gc - 1) / gc, (unsigned)wg), dim3(kBlock), 0,
                         la.stream, masks, (const T*)a.rec, a.nulls, gc, (long)nchunk, a.plan.rounds * wg, la.B,
                         (T*)a.u, (T*)a.ts);
      break;
    }
    default:
      hipLaunchKernelGGL((osc6_finish_kernel<N, T>), dim3(nchunk, (unsigned)a.plan.slots), dim3(kBlock), 0, la.stream,
                         masks, (const T*)a.rec, a.nulls, a.plan.rounds, la.B, (T*)a.u, (T*)a.ts);
  }
  return hipGetLastError();
}
hipError_t launch_osc6_finish(int n, int dtype, const LaunchArgs& la, const FinishArgs& a) {
  const Osc6Plan& p = a.plan;
  bool ok = la.B >= 1;
  switch (p.form) {
    case Osc6Form::HandoverChunk:
      ok = ok && p.slots >= 1 && p.slots <= kBlock && la.B <= kOsc6ChunkFinishMaxRows;
      break;
    case Osc6Form::HandoverGroup:  // (one lane per chunk holds the group's masks)
      ok = ok && p.group >= 1 && p.group <= kOsc6MaxGroup && la.B <= kOsc6ChunkFinishMaxRows;
      break;
    case Osc6Form::HandoverDense:
      break;
    default:
      ok = false;
  }
  if (!ok) return hipErrorInvalidValue;
  return for_joints_and_dtype(
      n, dtype, [&](auto nn, auto t) { return finish_launch<nn(), decltype(t)>(la, a); }, hipErrorInvalidValue);
}
template <int N, class T>
static hipError_t limits_launch(const LaunchArgs& la, const void* P, const void* q, void* u, int acc) {
  hipLaunchKernelGGL((limits_kernel<N, T>), grid_for(la.B), dim3(kBlock), 0, la.stream,
                     *static_cast<const LimitsP<T>*>(P), la.B, (const T*)q, (T*)u, acc);
  return hipGetLastError();
}
hipError_t launch_limits(int n, int dtype, const LaunchArgs& la, const void* P, const void* q, void* u, int acc) {
  return for_joints_and_dtype(
      n, dtype, [&](auto nn, auto t) { return limits_launch<nn(), decltype(t)>(la, P, q, u, acc); },
      hipErrorInvalidValue);
}
template <int N, class T>
static hipError_t mx_launch(const LaunchArgs& la, int k, double thr, const void* M, const void* J, void* Mx, void* Minv) {
  hipLaunchKernelGGL((mx_kernel<N, T>), grid_for(la.B), dim3(kBlock), 0, la.stream, la.B, k, T(thr), (const T*)M,
                     (const T*)J, (T*)Mx, (T*)Minv);
  return hipGetLastError();
}
hipError_t launch_osc_mx(int n, int dtype, const LaunchArgs& la, int k, double thr, const void* M, const void* J,
                         void* Mx, void* Minv) {
  return for_joints_and_dtype(
      n, dtype, [&](auto nn, auto t) { return mx_launch<nn(), decltype(t)>(la, k, thr, M, J, Mx, Minv); },
      hipErrorInvalidValue);
}
hipError_t launch_velocity_limiting(int dtype, const LaunchArgs& la, const double (&g)[5], const void* in, void* out) {
  for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((velocity_limiting_kernel<T>), grid_for(la.B), dim3(kBlock), 0, la.stream, la.B, T(g[0]), T(g[1]),
                       T(g[2]), T(g[3]), T(g[4]), (const T*)in, (T*)out);
  });
  return hipGetLastError();
}
hipError_t launch_orientation_forces(int dtype, const LaunchArgs& la, int alg, const void* R, const void* abg, void* out) {
  for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((orientation_forces_kernel<T>), grid_for(la.B), dim3(kBlock), 0, la.stream, la.B, alg,
                       (const T*)R, (const T*)abg, (T*)out);
  });
  return hipGetLastError();
}
hipError_t launch_transformations(int dtype, const LaunchArgs& la, int op, const void* a, const void* b, void* out) {
  for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((transformations_kernel<T>), grid_for(la.B), dim3(kBlock), 0, la.stream, la.B, op, (const T*)a,
                       (const T*)b, (T*)out);
  });
  return hipGetLastError();
}
hipError_t launch_twolink_step(int dtype, const LaunchArgs& la, const void* K, void* q, void* dq, const void* u) {
  for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((twolink_step_kernel<T>), grid_for(la.B), dim3(kBlock), 0, la.stream,
                       *static_cast<const TwoLinkP<T>*>(K), la.B, (T*)q, (T*)dq, (const T*)u);
  });
  return hipGetLastError();
}
}  // namespace abrk

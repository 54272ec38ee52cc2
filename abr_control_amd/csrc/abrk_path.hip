// abrk_path.hip - kernels of the batched PathPlanner (row programs: abrk_path.h).
//
//   path_plan_kernel      one lane per row: cumulative chord lengths of the warped curve -> dist_steps [B,S] (global),
//                         first candidate max_v whose ramps fit -> rowplan, n_timesteps; rows without a path raise the
//                         path-error word.
//   path_fill_kernel      one workgroup per row, lanes striding over the row's steps so that a wavefront's stores walk
//                         the row's contiguous [T, W] block.  The row's dist_steps - what every step binary-searches -
//                         sits in LDS (8 S bytes: S = 1000 takes 8 KB, so eight rows fit a CU's 160 KiB beside each
//                         other); S > kPathLdsSamples searches the global copy instead.  The warped samples themselves
//                         are NOT staged: a step needs two of them, each nine multiply-adds on the sample table that all
//                         rows share and the caches hold.
//   path_gradient_kernel  np.gradient of the position and Euler columns into the velocity columns, then the padding of
//                         steps [T, Tmax) with the row's last point.  A padding lane recomputes the last point's
//                         one-sided difference itself: nothing it reads is written by this kernel.
//   path_next_kernel      the path feed of a recorded loop: one lane per row copies path[b, counter[b]] into the
//                         controller's target / target_velocity (fp64 or fp32) and advances the counter, clamped.
#include "abrk_path.h"

namespace abrk {
namespace {

__global__ void __launch_bounds__(64) path_plan_kernel(PathArgs a) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  int kc[2];
  const int T = path_plan_row(a, a.start + 3 * b, a.target + 3 * b, a.dist_steps + b * (long)a.S, kc);
  a.rowplan[2 * b] = kc[0];
  a.rowplan[2 * b + 1] = kc[1];
  a.n_timesteps[b] = T;
  if (T == 0 && a.status) *a.status = 1;
}

template <bool LDS>
__global__ void __launch_bounds__(kPathBlock) path_fill_kernel(PathArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const long b = blockIdx.x;
  const int T = a.n_timesteps[b];
  if (T < 2 || T > a.Tmax) return;  // (uniform over the workgroup)  T > Tmax: the gradient pass skips the row as well
  {  // a rowplan that is not the plan pass's own for this table would index past the ramps: such a row is left alone
    const int k = a.rowplan[2 * b], c = a.rowplan[2 * b + 1];
    if (k < 0 || k >= a.K || c < 0 || a.off[2 + 4 * k + 1] + c + a.off[2 + 4 * k + 3] != T) return;
  }
  const double* gds = a.dist_steps + b * (long)a.S;
  if (LDS) {
    for (int s = threadIdx.x; s < a.S; s += kPathBlock) lds[s] = gds[s];
    __syncthreads();
  }
  auto ds = [&](int s) { return LDS ? lds[s] : gds[s]; };
  PathFillRow f;
  path_fill_setup(a, b, T, ds, f);
  double* row = a.path + b * (long)a.Tmax * a.W;
  for (int i = threadIdx.x; i < T; i += kPathBlock) {
    double out[12];
    path_fill_step(a, f, ds, i, out);
    double* o = row + (long)i * a.W;
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
    if (a.W == 12) {
      o[6] = out[6];
      o[7] = out[7];
      o[8] = out[8];
    }
  }
}

__global__ void __launch_bounds__(kPathBlock) path_gradient_kernel(PathArgs a) {
  const long b = blockIdx.x;
  const int T = a.n_timesteps[b];
  if (T < 2 || T > a.Tmax) return;
  double* row = a.path + b * (long)a.Tmax * a.W;
  for (int i = threadIdx.x; i < a.Tmax; i += kPathBlock) {
    const int ie = i < T ? i : T - 1;
    double* o = row + (long)i * a.W;
    for (int h = 0; h < a.W; h += 6) {  // columns h..h+3: values, h+3..h+6: their gradient
      for (int c = 0; c < 3; c++) o[h + 3 + c] = path_gradient_at(row + h + c, a.W, T, ie, a.dt);
      if (i >= T)
        for (int c = 0; c < 3; c++) o[h + c] = row[(long)(T - 1) * a.W + h + c];
    }
  }
}

template <class TO>
__global__ void __launch_bounds__(64) path_next_kernel(PathNextArgs a) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int T = a.n_timesteps[b] < a.Tmax ? a.n_timesteps[b] : a.Tmax;
  if (T < 1) return;
  int n = a.counter[b];
  n = n < 0 ? 0 : (n > T - 1 ? T - 1 : n);
  const double* p = a.path + (b * (long)a.Tmax + n) * a.W;
  TO* tg = (TO*)a.target + 6 * b;
  TO* tv = a.target_velocity ? (TO*)a.target_velocity + 6 * b : nullptr;
  for (int h = 0; h < a.W; h += 6)
    for (int c = 0; c < 3; c++) {
      tg[h / 2 + c] = (TO)p[h + c];
      if (tv) tv[h / 2 + c] = (TO)p[h + 3 + c];
    }
  a.counter[b] = n + 1 < T - 1 ? n + 1 : T - 1;
}

}  // namespace

hipError_t launch_path_plan(const PathArgs& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(path_plan_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_path_fill(const PathArgs& a, hipStream_t stream) {
  if (a.B <= 0 || a.Tmax <= 0) return hipSuccess;
  if (a.S <= kPathLdsSamples)
    hipLaunchKernelGGL(path_fill_kernel<true>, dim3((unsigned)a.B), dim3(kPathBlock), (size_t)a.S * sizeof(double), stream,
                       a);
  else
    hipLaunchKernelGGL(path_fill_kernel<false>, dim3((unsigned)a.B), dim3(kPathBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_path_gradient(const PathArgs& a, hipStream_t stream) {
  if (a.B <= 0 || a.Tmax <= 0) return hipSuccess;
  hipLaunchKernelGGL(path_gradient_kernel, dim3((unsigned)a.B), dim3(kPathBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_path_next(int out_dtype, const PathNextArgs& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  const dim3 grid((unsigned)((a.B + 63) / 64)), block(64);
  if (out_dtype == 0) hipLaunchKernelGGL(path_next_kernel<double>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(path_next_kernel<float>, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace abrk

// hostsim_path.cpp - TEST AID ONLY.  The per-row programs of the batched path planner (abr_control_amd/csrc/abrk_path.h:
// exactly what the lanes of path_plan_kernel / path_fill_kernel / path_gradient_kernel execute) compiled for the HOST,
// so that parity with the reference's PathPlanner is checked without a GPU.  Built on first use by
// tests/hostsim_path/__init__.py.
#define ABRK_PATH_HD __host__ __device__
#include <cmath>
#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_path.h"

using namespace abrk;

namespace {
PathArgs make(double dt, int S, int K, int axes, int W, const double* tab, const int64_t* off, int64_t B,
              const double* start, const double* target) {
  PathArgs a{};
  a.tab = tab;
  a.off = off;
  a.dt = dt;
  a.S = S;
  a.K = K;
  a.axes = axes;
  a.W = W;
  a.B = (long)B;
  a.start = start;
  a.target = target;
  return a;
}
}  // namespace

// -> number of rows without a path
extern "C" int hostsim_path_plan(double dt, int S, int K, int axes, int W, const double* tab, const int64_t* off,
                                 int64_t B, const double* start, const double* target, int* n_timesteps, int* rowplan,
                                 double* dist_steps) {
  const PathArgs a = make(dt, S, K, axes, W, tab, off, B, start, target);
  int bad = 0;
  for (long b = 0; b < B; b++) {
    n_timesteps[b] = path_plan_row(a, start + 3 * b, target + 3 * b, dist_steps + b * (long)S, rowplan + 2 * b);
    bad += n_timesteps[b] == 0;
  }
  return bad;
}

extern "C" int hostsim_path_fill(double dt, int S, int K, int axes, int W, const double* tab, const int64_t* off,
                                 int64_t B, int Tmax, const double* start, const double* target, const double* start_o,
                                 const double* target_o, const int* n_timesteps, const int* rowplan,
                                 const double* dist_steps, double* path) {
  PathArgs a = make(dt, S, K, axes, W, tab, off, B, start, target);
  a.Tmax = Tmax;
  a.start_o = start_o;
  a.target_o = target_o;
  a.n_timesteps = const_cast<int*>(n_timesteps);
  a.rowplan = const_cast<int*>(rowplan);
  a.dist_steps = const_cast<double*>(dist_steps);
  a.path = path;
  for (long b = 0; b < B; b++) {
    const int T = n_timesteps[b];
    if (T < 2 || T > Tmax) continue;
    const double* gds = dist_steps + b * (long)S;
    auto ds = [&](int s) { return gds[s]; };
    PathFillRow f;
    path_fill_setup(a, b, T, ds, f);
    double* row = path + b * (long)Tmax * W;
    for (int i = 0; i < T; i++) {  // fill pass
      double out[12];
      path_fill_step(a, f, ds, i, out);
      for (int h = 0; h < W; h += 6)
        for (int c = 0; c < 3; c++) row[(long)i * W + h + c] = out[h + c];
    }
    for (int i = 0; i < Tmax; i++) {  // gradient pass, then the padding
      const int ie = i < T ? i : T - 1;
      for (int h = 0; h < W; h += 6) {
        for (int c = 0; c < 3; c++) row[(long)i * W + h + 3 + c] = path_gradient_at(row + h + c, W, T, ie, dt);
        if (i >= T)
          for (int c = 0; c < 3; c++) row[(long)i * W + h + c] = row[(long)(T - 1) * W + h + c];
      }
    }
  }
  return 0;
}

// abrk_path.h - the batched PathPlanner (abr_control/controllers/path_planners/path_planner.py:99-452 with
// orientation.py:130-198 and the transformations.py functions they call): the per-row programs, the argument block of
// the kernels in abrk_path.hip and their launchers.  Arm-independent and fp64 only: a path sums thousands of increments.
//
// The host/device split (DESIGN.md "Path planner"): everything that depends on the user's profile OBJECTS - the sampled
// position profile, one velocity ramp pair per candidate max_v, their np.sum distances and np.cumsum prefixes - is
// evaluated once per call on the host by the profiles' own Python and arrives here as one packed table of doubles with
// an offsets array; everything that depends on a ROW (start, target, orientations) runs here.
//
//   off[0]            -> S x 3 samples of pos_profile.step(linspace(0, 1, S))
//   off[1]            -> K x 3 scalars per candidate: max_v, starting_dist, ending_dist
//   off[2 + 4k + 0/1] -> cumsum(starting_vel_profile * dt) of candidate k, its length
//   off[2 + 4k + 2/3] -> cumsum(ending_vel_profile * dt) of candidate k, its length
//
// The row functions are plain C++ and compile for the host as well (tests/hostsim_path defines ABRK_PATH_HD as
// __host__ __device__), so that parity with the reference is checked without a GPU.
#ifndef ABRK_PATH_H
#define ABRK_PATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef ABRK_PATH_HD
#define ABRK_PATH_HD __device__
#endif
#define ABRK_PATH_INL ABRK_PATH_HD inline

namespace abrk {

constexpr int kPathBlock = 256;        // lanes of a fill / gradient workgroup (one workgroup per row)
constexpr int kPathLdsSamples = 8192;  // dist_steps of up to this many samples sit in LDS (64 KiB); beyond: global scratch

struct PathArgs {
  const double* tab;
  const int64_t* off;
  double dt;
  int S, K, axes, W;  // samples, candidates, Euler axes code (firstaxis | parity << 2 | repetition << 3 | frame << 4), 6 | 12
  long B;
  int Tmax;                // steps per row of `path`
  const double* start;     // [B,3]
  const double* target;    // [B,3]
  const double* start_o;   // [B,3] or null (W == 6)
  const double* target_o;  // [B,3] or null
  int* n_timesteps;        // [B]   0 = the row has no path (ABRK_EPATH)
  int* rowplan;            // [B,2] candidate index, constant-speed steps
  double* dist_steps;      // [B,S] cumulative chord lengths of the warped curve
  double* path;            // [B,Tmax,W]
  int* status;             // the stream's / thread's path-error word, or null
};

struct PathNextArgs {
  const double* path;
  const int* n_timesteps;
  int* counter;
  void* target;           // [B,6] of the output type
  void* target_velocity;  // [B,6] or null
  long B;
  int Tmax, W;
};

hipError_t launch_path_plan(const PathArgs& a, hipStream_t stream);
hipError_t launch_path_fill(const PathArgs& a, hipStream_t stream);      // positions and Euler angles
hipError_t launch_path_gradient(const PathArgs& a, hipStream_t stream);  // velocity columns, then the padding
hipError_t launch_path_next(int out_dtype, const PathNextArgs& a, hipStream_t stream);

// ---------------------------------------------------------------------------------------------- row programs
constexpr double kPathEps = 2.220446049250313e-16 * 4.0;  // transformations.py:1559 _EPS

// what a row needs of the packed table and of its own start / target
struct PathRow {
  double R[9];      // align_vectors(base_norm, target_norm), path_planner.py:75-97
  double dist;      // |target - start|
  double start[3];
};

// path_planner.py:184-192.  false: start == target (the reference divides by zero there), or a movement exactly
// towards -(1,1,1)/sqrt(3), where align_vectors divides by 1 + cs = 0 (the reference raises from generate_path).  The
// library is built with -ffinite-math-only, so 1 + cs itself is tested, not the h it would give.
ABRK_PATH_INL bool path_row_setup(const double* sp, const double* tp, PathRow& r) {
  double d[3];
  for (int c = 0; c < 3; c++) {
    d[c] = tp[c] - sp[c];
    r.start[c] = sp[c];
  }
  r.dist = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (int c = 0; c < 9; c++) r.R[c] = c % 4 == 0 ? 1.0 : 0.0;
  if (!(r.dist > 0.0)) return false;
  double b[3], a[3];
  for (int c = 0; c < 3; c++) b[c] = d[c] / r.dist;
  const double a0 = 1.0 / sqrt(3.0);
  // align_vectors normalises both arguments again
  const double nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  const double na = sqrt(a0 * a0 + a0 * a0 + a0 * a0);
  for (int c = 0; c < 3; c++) {
    b[c] = b[c] / nb;
    a[c] = a0 / na;
  }
  const double v1 = a[1] * b[2] - a[2] * b[1], v2 = a[2] * b[0] - a[0] * b[2], v3 = a[0] * b[1] - a[1] * b[0];
  const double cs = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  if (!(1.0 + cs > 0.0)) return false;
  const double h = 1.0 / (1.0 + cs);
  const double V[9] = {0.0, -v3, v2, v3, 0.0, -v1, -v2, v1, 0.0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double vv = 0.0;
      for (int k = 0; k < 3; k++) vv += V[3 * i + k] * V[3 * k + j];
      r.R[3 * i + j] = (i == j ? 1.0 : 0.0) + V[3 * i + j] + vv * h;
    }
  return true;
}

// sample s of the warped curve: R . ((1/sqrt(3)) step(t_s) dist) + start   (path_planner.py:202-205)
ABRK_PATH_INL void path_warp(const PathRow& r, const double* samples, int s, double* w) {
  const double a0 = 1.0 / sqrt(3.0);
  double p[3];
  for (int c = 0; c < 3; c++) p[c] = a0 * samples[3 * s + c] * r.dist;
  for (int i = 0; i < 3; i++) w[i] = r.R[3 * i] * p[0] + r.R[3 * i + 1] * p[1] + r.R[3 * i + 2] * p[2] + r.start[i];
}

// The plan of one row (path_planner.py:194-302): cumulative chord lengths into ds[0..S), then the first candidate whose
// ramps fit the curve.  -> n_timesteps, or 0 when the row has no path: start == target, no candidate left (the
// reference's `max_v <= 0: raise ValueError`), fewer than the two steps np.gradient needs, or more than an int holds.
ABRK_PATH_INL int path_plan_row(const PathArgs& a, const double* sp, const double* tp, double* ds, int* kc) {
  kc[0] = kc[1] = 0;
  PathRow r;
  const bool ok = path_row_setup(sp, tp, r);
  const double* samples = a.tab + a.off[0];
  double prev[3], cur[3], cum = 0.0;
  path_warp(r, samples, 0, prev);
  ds[0] = 0.0;
  for (int s = 1; s < a.S; s++) {
    path_warp(r, samples, s, cur);
    const double e0 = cur[0] - prev[0], e1 = cur[1] - prev[1], e2 = cur[2] - prev[2];
    cum += sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    ds[s] = cum;
    for (int c = 0; c < 3; c++) prev[c] = cur[c];
  }
  if (!ok) return 0;
  const double* scal = a.tab + a.off[1];
  for (int k = 0; k < a.K; k++) {
    const double max_v = scal[3 * k], sd = scal[3 * k + 1], ed = scal[3 * k + 2];
    const int64_t ls = a.off[2 + 4 * k + 1], le = a.off[2 + 4 * k + 3];
    double steps = 0.0;
    if (cum > sd + ed) {
      const double remaining = cum - (ed + sd);
      steps = remaining / max_v / a.dt;  // int() of it below: plain IEEE divisions in the reference's order
    } else if (!(cum == sd + ed)) {
      continue;
    }
    if (!(steps < 2.0e9)) return 0;
    const int64_t c = (int64_t)steps, T = ls + c + le;
    if (T < 2 || T > 2000000000) return 0;
    kc[0] = k;
    kc[1] = (int)c;
    return (int)T;
  }
  return 0;
}

// distance along the curve at step i: np.cumsum(stacked_vel_profile * dt)[i] (path_planner.py:316) from the uploaded
// prefixes of the two ramps and the constant-speed segment between them
ABRK_PATH_INL double path_step_dist(const PathArgs& a, int k, int c, int i) {
  const double* sp = a.tab + a.off[2 + 4 * k];
  const double* ep = a.tab + a.off[2 + 4 * k + 2];
  const int ls = (int)a.off[2 + 4 * k + 1];
  if (i < ls) return sp[i];
  const double base = ls > 0 ? sp[ls - 1] : 0.0;
  const double inc = a.tab[a.off[1] + 3 * k] * a.dt;
  if (i < ls + c) return base + (double)(i - ls + 1) * inc;
  return base + (double)c * inc + ep[i - ls - c];
}

// scipy.interpolate.interp1d(kind="linear", fill_value="extrapolate") of the warped curve over dist_steps:
// searchsorted (left), index clipped to [1, S-1], slope form - so both ends extrapolate.  DS: ds(s) -> dist_steps[s]
template <class DS>
ABRK_PATH_INL void path_position(const PathArgs& a, const PathRow& r, DS&& ds, double x, double* p) {
  int lo = 0, hi = a.S;  // first index with ds(idx) >= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ds(mid) < x) lo = mid + 1;
    else hi = mid;
  }
  int idx = lo < 1 ? 1 : lo;
  if (idx > a.S - 1) idx = a.S - 1;
  const double x_lo = ds(idx - 1), x_hi = ds(idx);
  double w_lo[3], w_hi[3];
  const double* samples = a.tab + a.off[0];
  path_warp(r, samples, idx - 1, w_lo);
  path_warp(r, samples, idx, w_hi);
  for (int c = 0; c < 3; c++) {
    const double slope = (w_hi[c] - w_lo[c]) / (x_hi - x_lo);
    p[c] = slope * (x - x_lo) + w_lo[c];
  }
}

// ---- the Euler / quaternion functions of transformations.py, for all 24 axis sequences
struct EulerAxes {
  int i, j, k, parity, repetition, frame;  // matrix indices 0..2
};
ABRK_PATH_INL EulerAxes euler_axes(int code) {
  const int next[4] = {1, 2, 0, 1};  // transformations.py:1562
  EulerAxes e;
  e.i = code & 3;
  e.parity = (code >> 2) & 1;
  e.repetition = (code >> 3) & 1;
  e.frame = (code >> 4) & 1;
  e.j = next[e.i + e.parity];
  e.k = next[e.i - e.parity + 1];
  return e;
}

// quaternion_from_euler (transformations.py:1096-1147), q = (w, x, y, z)
ABRK_PATH_INL void path_quat_from_euler(const EulerAxes& e, double ai, double aj, double ak, double* q) {
  if (e.frame) {
    const double t = ai;
    ai = ak;
    ak = t;
  }
  if (e.parity) aj = -aj;
  ai /= 2.0;
  aj /= 2.0;
  ak /= 2.0;
  const double ci = cos(ai), si = sin(ai), cj = cos(aj), sj = sin(aj), ck = cos(ak), sk = sin(ak);
  const double cc = ci * ck, cs = ci * sk, sc = si * ck, ss = si * sk;
  const int i = e.i + 1, j = e.j + 1, k = e.k + 1;
  if (e.repetition) {
    q[0] = cj * (cc - ss);
    q[i] = cj * (cs + sc);
    q[j] = sj * (cc + ss);
    q[k] = sj * (cs - sc);
  } else {
    q[0] = cj * cc + sj * ss;
    q[i] = cj * sc - sj * cs;
    q[j] = cj * ss + sj * cc;
    q[k] = cj * cs - sj * sc;
  }
  if (e.parity) q[j] *= -1.0;
}

ABRK_PATH_INL void path_unit4(const double* q, double* u) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int c = 0; c < 4; c++) u[c] = q[c] / n;
}

// quaternion_slerp(quat0, quat1, fraction) with every early return of transformations.py:1349-1369
ABRK_PATH_INL void path_slerp(const double* quat0, const double* quat1, double fraction, double* out) {
  double q0[4], q1[4];
  path_unit4(quat0, q0);
  path_unit4(quat1, q1);
  for (int c = 0; c < 4; c++) out[c] = q0[c];
  if (fraction == 0.0) return;
  if (fraction == 1.0) {
    for (int c = 0; c < 4; c++) out[c] = q1[c];
    return;
  }
  double d = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
  if (fabs(fabs(d) - 1.0) < kPathEps) return;
  if (d < 0.0) {
    d = -d;
    for (int c = 0; c < 4; c++) q1[c] = -q1[c];
  }
  const double angle = acos(d);
  if (fabs(angle) < kPathEps) return;
  const double isin = 1.0 / sin(angle);
  const double s0 = sin((1.0 - fraction) * angle) * isin, s1 = sin(fraction * angle) * isin;
  for (int c = 0; c < 4; c++) out[c] = q0[c] * s0 + q1[c] * s1;
}

// euler_from_quaternion = euler_from_matrix(quaternion_matrix(q)) (transformations.py:1033-1093, 1164-1189)
ABRK_PATH_INL void path_euler_from_quat(const EulerAxes& e, const double* quat, double* abg) {
  double M[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  const double n = quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3];
  if (!(n < kPathEps)) {
    const double s = sqrt(2.0 / n);
    double q[4], o[16];
    for (int c = 0; c < 4; c++) q[c] = quat[c] * s;
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) o[4 * r + c] = q[r] * q[c];
    M[0] = 1.0 - o[10] - o[15];
    M[1] = o[6] - o[12];
    M[2] = o[7] + o[8];
    M[3] = o[6] + o[12];
    M[4] = 1.0 - o[5] - o[15];
    M[5] = o[11] - o[4];
    M[6] = o[7] - o[8];
    M[7] = o[11] + o[4];
    M[8] = 1.0 - o[5] - o[10];
  }
  const int i = e.i, j = e.j, k = e.k;
  double ax, ay, az;
  if (e.repetition) {
    const double sy = sqrt(M[3 * i + j] * M[3 * i + j] + M[3 * i + k] * M[3 * i + k]);
    if (sy > kPathEps) {
      ax = atan2(M[3 * i + j], M[3 * i + k]);
      ay = atan2(sy, M[3 * i + i]);
      az = atan2(M[3 * j + i], -M[3 * k + i]);
    } else {
      ax = atan2(-M[3 * j + k], M[3 * j + j]);
      ay = atan2(sy, M[3 * i + i]);
      az = 0.0;
    }
  } else {
    const double cy = sqrt(M[3 * i + i] * M[3 * i + i] + M[3 * j + i] * M[3 * j + i]);
    if (cy > kPathEps) {
      ax = atan2(M[3 * k + j], M[3 * k + k]);
      ay = atan2(-M[3 * k + i], cy);
      az = atan2(M[3 * j + i], M[3 * i + i]);
    } else {
      ax = atan2(-M[3 * j + k], M[3 * j + j]);
      ay = atan2(-M[3 * k + i], cy);
      az = 0.0;
    }
  }
  if (e.parity) {
    ax = -ax;
    ay = -ay;
    az = -az;
  }
  if (e.frame) {
    const double t = ax;
    ax = az;
    az = t;
  }
  abg[0] = ax;
  abg[1] = ay;
  abg[2] = az;
}

// what every step of a row shares in the fill pass
struct PathFillRow {
  PathRow r;
  int k, c, T;
  double p_last[3], span;  // position_path[-1], |position_path[-1] - position_path[0]| (orientation.py:182)
  double q0[4], q1[4];
  EulerAxes e;
};

template <class DS>
ABRK_PATH_INL void path_fill_setup(const PathArgs& a, long b, int T, DS&& ds, PathFillRow& f) {
  path_row_setup(a.start + 3 * b, a.target + 3 * b, f.r);
  f.k = a.rowplan[2 * b];
  f.c = a.rowplan[2 * b + 1];
  f.T = T;
  f.span = 0.0;
  if (a.W != 12) return;
  double p0[3];
  path_position(a, f.r, ds, path_step_dist(a, f.k, f.c, 0), p0);
  path_position(a, f.r, ds, path_step_dist(a, f.k, f.c, T - 1), f.p_last);
  const double e0 = f.p_last[0] - p0[0], e1 = f.p_last[1] - p0[1], e2 = f.p_last[2] - p0[2];
  f.span = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
  f.e = euler_axes(a.axes);
  const double *so = a.start_o + 3 * b, *to = a.target_o + 3 * b;
  path_quat_from_euler(f.e, so[0], so[1], so[2], f.q0);
  path_quat_from_euler(f.e, to[0], to[1], to[2], f.q1);
}

// step i of a row: position columns 0:3 and (W == 12) Euler angles 6:9 of out[0..W)
template <class DS>
ABRK_PATH_INL void path_fill_step(const PathArgs& a, const PathFillRow& f, DS&& ds, int i, double* out) {
  double p[3];
  path_position(a, f.r, ds, path_step_dist(a, f.k, f.c, i), p);
  for (int c = 0; c < 3; c++) out[c] = p[c];
  if (a.W != 12) return;
  const double e0 = f.p_last[0] - p[0], e1 = f.p_last[1] - p[1], e2 = f.p_last[2] - p[2];
  const double fraction = 1.0 - sqrt(e0 * e0 + e1 * e1 + e2 * e2) / f.span;  // orientation.py:184-190
  double q[4];
  path_slerp(f.q0, f.q1, fraction, q);
  path_euler_from_quat(f.e, q, out + 6);
}

// np.gradient(column, dt, axis=0) at step i of a row of T >= 2 steps: central differences inside, one-sided first
// order at both ends.  col: the row's path + the column
ABRK_PATH_INL double path_gradient_at(const double* col, int W, int T, int i, double dt) {
  if (i == 0) return (col[(long)W] - col[0]) / dt;
  if (i == T - 1) return (col[(long)W * (T - 1)] - col[(long)W * (T - 2)]) / dt;
  return (col[(long)W * (i + 1)] - col[(long)W * (i - 1)]) / (2.0 * dt);
}

}  // namespace abrk
#endif  // ABRK_PATH_H

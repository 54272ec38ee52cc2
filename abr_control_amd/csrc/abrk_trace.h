// abrk_trace.h - the output side of a device-resident control loop: one row program that, once per tick, snapshots
// chosen columns of an arm's state into a time-major history and keeps per-row tracking-error statistics.  The
// counterpart of path_next_kernel (abrk_path.hip): recorded into a plan behind { path_next; law; plant step } it lets a
// graph replay of K ticks come back with trajectories and statistics instead of the final state alone.
// Like the other row programs it compiles for the host (tests/hostsim_trace).
#pragma once
#include "abrk_rows.h"

namespace abrk {

// history columns, in their fixed order (include/abrk_types.h ABRK_TR_*): q, dq, u [n], target [6], xyz [3], err [1]
enum { TR_Q = 1u << 0, TR_DQ = 1u << 1, TR_U = 1u << 2, TR_TARGET = 1u << 3, TR_XYZ = 1u << 4, TR_ERR = 1u << 5, TR_ALL = 63u };
constexpr int trace_width(unsigned cols, int n) {
  return ((cols & TR_Q) ? n : 0) + ((cols & TR_DQ) ? n : 0) + ((cols & TR_U) ? n : 0) + ((cols & TR_TARGET) ? 6 : 0) +
         ((cols & TR_XYZ) ? 3 : 0) + ((cols & TR_ERR) ? 1 : 0);
}

template <class T>
struct TraceP {
  int frame;        // link_i -> 2i, joint_i -> 2i+1, EE -> 2N+1 (FrameCap)
  T off[3];         // point in that frame
  int every, capacity;
  unsigned columns;
  int W;            // trace_width(columns, N)
  int lds;          // != 0: a wavefront whose rows share one slot writes it through LDS (device only)
  double tol;       // settling tolerance on err
};
template <class T>
struct TraceIO {
  const T *q, *dq, *u, *target;
  int* counter;     // [B] the row's tick
  T* history;       // [capacity, B, W] or null
  double* stats;    // [B, 4] err_last, err_max, err_min, err_sumsq, or null
  int* settle;      // [B]: 0 = outside the tolerance now, k > 0 = inside since tick k - 1
};

// Tx of `frame` with offset `off`: the forward kinematics of dyn_body (abrk_rows.h) without its dynamics
template <class A, class T>
ABRK_INL void trace_xyz(const A& arm, int frame, const T (&off)[3], const T (&q)[A::N], T (&p)[3]) {
  constexpr int N = A::N;
  Joints<A, T> jt;
  T XR[9], xo[3];
  FrameCap<T> cap;
  cap.frame = frame;
  sfor<9>([&](auto e) ABRK_LAMBDA { cap.R[e()] = T(0); });
  sfor<3>([&](auto r) ABRK_LAMBDA { cap.o[r()] = T(0); });
  T sv[N][2];
  sincos_all<N>(q, sv);
  fk_forward(arm, q, jt, XR, xo, cap, [](auto, const T(&)[3]) ABRK_LAMBDA {}, ScUse<T, N>{sv});
  sfor<3>([&](auto r) ABRK_LAMBDA {
    p[r()] = cap.o[r()] + cap.R[r() * 3] * off[0] + cap.R[r() * 3 + 1] * off[1] + cap.R[r() * 3 + 2] * off[2];
  });
}

// History store policies.  put() hands `emit` a sink(offset, value) that takes the row's W values in column order.
// TraceDirect: every lane writes its own row, W elements at a stride of W (host build; the device's fallback).  The
// GPU kernel's TraceLds (abrk_kernels.h) transposes a wavefront's rows through LDS.
template <class T>
struct TraceDirect {
  template <class Emit>
  ABRK_INL void put(T* __restrict__ hist, bool due, int slot, long b, bool active, long B, int W, Emit&& emit) {
    if (active && due) {
      T* p = hist + ((long)slot * B + b) * W;
      emit([&](int o, T v) ABRK_LAMBDA { p[o] = v; });
    }
  }
};

// One tick of row b (t = counter[b]): position and error, the history slot t / every if it is due, the statistics, then
// counter[b] = t + 1.  Every output is the lane's own.  `active` is false for the padding lanes of the last wavefront,
// which only take part in the cooperative store.
template <class A, class T, class St>
ABRK_INL void trace_body(long b, bool active, St& st, const A& arm, const TraceP<T>& P, long B, const TraceIO<T>& io) {
  constexpr int N = A::N;
  const unsigned cols = io.history ? P.columns : 0u;
  const bool want_err = (cols & TR_ERR) || io.stats;
  const bool want_xyz = (cols & TR_XYZ) || want_err;
  int t = 0;
  T q[N], tgt[6], xyz[3] = {T(0), T(0), T(0)}, err = T(0);
  sfor<N>([&](auto i) ABRK_LAMBDA { q[i()] = T(0); });
  sfor<6>([&](auto i) ABRK_LAMBDA { tgt[i()] = T(0); });
  if (active) {
    t = io.counter[b];
    t = t < 0 ? 0 : t;
    if (want_xyz || (cols & TR_Q)) load_row<N>(io.q, b, q);
    if (want_err || (cols & TR_TARGET)) load_row<6>(io.target, b, tgt);
    if (want_xyz) trace_xyz<A, T>(arm, P.frame, P.off, q, xyz);
    if (want_err) {
      const T dx = tgt[0] - xyz[0], dy = tgt[1] - xyz[1], dz = tgt[2] - xyz[2];
      err = Rm<T>::sqrt(dx * dx + dy * dy + dz * dz);
    }
  }
  const int slot = t / P.every;
  const bool due = io.history && t % P.every == 0 && slot < P.capacity;
  if (io.history) {
    st.put(io.history, due, slot, b, active, B, P.W, [&](auto&& sink) ABRK_LAMBDA {
      int o = 0;
      if (cols & TR_Q) {
        sfor<N>([&](auto i) ABRK_LAMBDA { sink(o + i(), q[i()]); });
        o += N;
      }
      // dq and u are only copied: read where they are stored, not held across the kinematics
      if (cols & TR_DQ) {
        T v[N];
        load_row<N>(io.dq, b, v);
        sfor<N>([&](auto i) ABRK_LAMBDA { sink(o + i(), v[i()]); });
        o += N;
      }
      if (cols & TR_U) {
        T v[N];
        load_row<N>(io.u, b, v);
        sfor<N>([&](auto i) ABRK_LAMBDA { sink(o + i(), v[i()]); });
        o += N;
      }
      if (cols & TR_TARGET) {
        sfor<6>([&](auto i) ABRK_LAMBDA { sink(o + i(), tgt[i()]); });
        o += 6;
      }
      if (cols & TR_XYZ) {
        sfor<3>([&](auto i) ABRK_LAMBDA { sink(o + i(), xyz[i()]); });
        o += 3;
      }
      if (cols & TR_ERR) sink(o, err);
    });
  }
  if (!active) return;
  if (io.stats) {
    // assigned at tick 0, combined after it: a reset is a zero fill (no infinities: -ffinite-math-only)
    double* s = io.stats + 4 * b;
    const double e = (double)err;
    double mx = e, mn = e, ss = e * e;
    if (t != 0) {
      const double omx = s[1], omn = s[2];
      mx = omx > e ? omx : e;
      mn = omn < e ? omn : e;
      ss += s[3];
    }
    s[0] = e;
    s[1] = mx;
    s[2] = mn;
    s[3] = ss;
    const int was = io.settle[b];
    io.settle[b] = e <= P.tol ? (was ? was : t + 1) : 0;
  }
  io.counter[b] = t + 1;
}

}  // namespace abrk

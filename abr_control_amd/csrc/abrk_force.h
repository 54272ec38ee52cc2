// abrk_force.h - force-controlled contact of a device-resident control loop: one row program that, once per tick, turns
// the state, a Cartesian target, a per-row command (surface normal n, desired force f_des) and the sensed force on the
// tip into the joint torque of Khatib's unified motion/force law - motion control in the plane tangent to n, a force PI
// loop along n while the tip is in contact, a guarded approach along -n while it is free.  Recorded into a plan where the
// motion law would be - { path_next; force law; contact; plant step } - it reads the contact report of the previous tick.
// The skeleton is floating_row's task-space branch (abrk_ctrl.h) with contact_body's frame capture and offset: one
// dynamics pass without Coriolis terms, the point Jacobian, one Cholesky factor of M, point_inertia, one symv for M dq.
// Like the other row programs it compiles for the host (tests/hostsim_force).
#pragma once
#include "abrk_rows.h"

namespace abrk {

constexpr int kForceCmdW = 4;  // nx, ny, nz, f_des

template <class T>
struct ForceP {
  int frame;  // link_i -> 2i, joint_i -> 2i+1, EE -> 2N+1 (FrameCap)
  int m;      // the joints the point hangs off (frame_joints(frame, N); the host's frame_m)
  T off[3];   // the point in that frame
  T kp, kv;   // motion gains
  T kf, ki, i_max;  // force PI and its anti-windup clamp
  T kvf;            // damping along n while in contact
  T f_touch;        // in contact where n.F exceeds it
  T v_app;          // approach speed along -n while free
  T kv_null;        // null-space damping; 0: off
  T dt;
  int use_g, accumulate;
  int force_ld;  // values per row of `force` (>= 3; 8: a contact report)
  int* status;   // as OscP::status: a non-positive Cholesky pivot of M -> ABRK_ESINGULAR
};
template <class T>
struct ForceIO {
  const T *q, *dq;   // [B, N]
  const T* target;   // [B, 6]: columns 0..2 are x_d
  const T* tv;       // [B, 6] or null: columns 0..2 are v_d
  const T* cmd;      // [B, 4] = nx, ny, nz, f_des: read with ordinary loads at every launch
  const T* force;    // [B, force_ld]: columns 0..2 are the force ON the tip, world frame
  T* integ;          // [B]: the force integral, in/out
  T* u;              // [B, N]
};

// One tick of row b (include/abrk.h has the law with its signs).  The mode - in contact where n.F > f_touch - is a
// per-lane select between two scalars along n and two values of the integral: both modes share the whole dynamics pass.
template <class A, class T>
ABRK_INL void force_body(long b, const A& arm, const ForceP<T>& P, const ForceIO<T>& io) {
  constexpr int N = A::N;
  T q[N];
  load_row<N>(io.q, b, q);
  Joints<A, T> jt;
  Dyn<A, T, CMODE_NONE> d;
  T XR[9], xo[3];
  FrameCap<T> cap;
  cap.frame = P.frame;
  sfor<9>([&](auto e) ABRK_LAMBDA { cap.R[e()] = T(0); });
  sfor<3>([&](auto r) ABRK_LAMBDA { cap.o[r()] = T(0); });
  {
    T zero[N];
    sfor<N>([&](auto i) ABRK_LAMBDA { zero[i()] = T(0); });
    kin_dyn(arm, q, zero, jt, d, XR, xo, cap);
  }
  T p[3];
  sfor<3>([&](auto r) ABRK_LAMBDA {
    p[r()] = cap.o[r()] + cap.R[r() * 3] * P.off[0] + cap.R[r() * 3 + 1] * P.off[1] + cap.R[r() * 3 + 2] * P.off[2];
  });
  T Jv[N][3], Jw[N][3];
  jacobian(jt, p, P.m, Jv, Jw);
  T L[N * (N + 1) / 2], il[N], Mx[6], minpiv = T(1);
  chol<N>(d.Ms, L, il, &minpiv);
  point_inertia<N, T, true>(L, il, Jv, T(1e-3), T(1e-4), T(0), Mx);
  // the row's inputs, asked for after the dynamics pass: nothing of them is held across it
  T dq[N], xd[3], vd[3], c[kForceCmdW], F[3];
  load_row<N>(io.dq, b, dq);
  sfor<3>([&](auto r) ABRK_LAMBDA {
    xd[r()] = io.target[b * 6 + r()];
    vd[r()] = io.tv ? io.tv[b * 6 + r()] : T(0);
    F[r()] = io.force[b * (long)P.force_ld + r()];
  });
  load_row<kForceCmdW>(io.cmd, b, c);
  const T integ = io.integ[b];
  T v[3] = {T(0), T(0), T(0)};
  sfor<N>([&](auto i) ABRK_LAMBDA { sfor<3>([&](auto r) ABRK_LAMBDA { v[r()] += Jv[i()][r()] * dq[i()]; }); });
  T a[3];
  sfor<3>([&](auto r) ABRK_LAMBDA { a[r()] = P.kp * (xd[r()] - p[r()]) + P.kv * (vd[r()] - v[r()]); });
  const T a_n = c[0] * a[0] + c[1] * a[1] + c[2] * a[2];
  const T v_n = c[0] * v[0] + c[1] * v[1] + c[2] * v[2];
  const T f_m = c[0] * F[0] + c[1] * F[1] + c[2] * F[2];
  const T f_des = c[3];
  const bool touching = f_m > P.f_touch;
  const T e = f_des - f_m;
  T wound = integ + P.ki * e * P.dt;
  wound = wound > P.i_max ? P.i_max : wound;
  wound = wound < -P.i_max ? -P.i_max : wound;
  const T integ_new = touching ? wound : T(0);
  // along n: the motion law's own part is taken out (a - a_n n) and replaced by damping (contact) or the approach (free)
  const T along = (touching ? -P.kvf * v_n : P.kv * (-P.v_app - v_n)) - a_n;
  const T push = touching ? -(f_des + P.kf * e + wound) : T(0);
  T w[3], Fc[3], mv[3];
  sfor<3>([&](auto r) ABRK_LAMBDA { w[r()] = a[r()] + along * c[r()]; });
  symv<3>(Mx, w, Fc);
  symv<3>(Mx, v, mv);
  // u = Jp^T F_c - [use_g] g - kv_null (M dq - Jp^T Mx v),  g = -9.81 gz
  T Mdq[N], u[N];
  symv<N>(d.Ms, dq, Mdq);
  sfor<3>([&](auto r) ABRK_LAMBDA { Fc[r()] += push * c[r()]; });
  sfor<N>([&](auto i) ABRK_LAMBDA {
    const T jf = Jv[i()][0] * Fc[0] + Jv[i()][1] * Fc[1] + Jv[i()][2] * Fc[2];
    const T jm = Jv[i()][0] * mv[0] + Jv[i()][1] * mv[1] + Jv[i()][2] * mv[2];
    T ui = jf - P.kv_null * (Mdq[i()] - jm);
    if (P.use_g) ui += T(9.81) * d.gz[i()];
    u[i()] = ui;
  });
  io.integ[b] = integ_new;
  put_row<N>(io.u, b, u, P.accumulate);
  // ABRK_ESINGULAR (abrk_ctrl.h flag_singular), after the row's outputs
  if (any_lane(!(minpiv > T(0))) && P.status) *P.status = 1;
}

}  // namespace abrk

// abrk_contact.h - end-effector contact of a device-resident control loop: one row program that, once per tick, turns
// the penetration of a sphere tip into per-row half-spaces into the joint torque tau_c = Jp^T F, which the plant reads
// as its tau_ext.  Recorded into a plan between the law and the plant step - { path_next; law; contact; plant step } -
// it lets an arm press on a table, slide along it with friction and lift off without the host.  Forward kinematics and
// the point Jacobian only: no dynamics pass.  The force is that of the state at the START of the tick; the plant holds it
// over its substeps like u (include/abrk.h has the stability bound this implies).
// Like the other row programs it compiles for the host (tests/hostsim_contact).
#pragma once
#include "abrk_rows.h"

namespace abrk {

constexpr int kContactMaxSurfaces = 4;  // include/abrk.h ABRK_CONTACT_MAX_SURFACES
constexpr int kContactSurfaceW = 8;     // nx, ny, nz, d, k, c, mu, rho
constexpr int kContactReportW = 8;      // F world [3], F in the frame [3], deepest delta, surfaces penetrated

template <class T>
struct ContactP {
  int frame;       // link_i -> 2i, joint_i -> 2i+1, EE -> 2N+1 (FrameCap)
  int m;           // the joints the point hangs off (frame_joints(frame, N); the host's frame_m)
  T off[3];        // the point in that frame
  int S;           // surfaces per row, 1..kContactMaxSurfaces
  T vs2;           // square of the smoothing speed of the friction law
  int accumulate;  // != 0: tau += tau_c
};
template <class T>
struct ContactIO {
  const T *q, *dq;   // [B, N]
  const T* surface;  // [B, S, 8]: read with ordinary loads at every launch
  T* tau;            // [B, N]
  T* report;         // [B, 8] or null
};

// The force of one half-space on the tip at p moving with v (world frame), added to F; -> its penetration delta.
//   delta = d + rho - n.p;  vn = n.v;  fn = max(0, k delta - c vn) where delta > 0, else 0
//   F += fn n - mu fn vt / sqrt(|vt|^2 + vs^2),  vt = v - vn n
// n is used as given.  A surface that does not push adds exact zeros.
template <class T>
ABRK_INL T contact_surface(const T (&s)[kContactSurfaceW], const T (&p)[3], const T (&v)[3], T vs2, T (&F)[3]) {
  const T delta = s[3] + s[7] - (s[0] * p[0] + s[1] * p[1] + s[2] * p[2]);
  const T vn = s[0] * v[0] + s[1] * v[1] + s[2] * v[2];
  const T push = s[4] * delta - s[5] * vn;
  const T fn = (delta > T(0) && push > T(0)) ? push : T(0);
  T vt[3];
  sfor<3>([&](auto r) ABRK_LAMBDA { vt[r()] = v[r()] - vn * s[r()]; });
  const T ft = s[6] * fn * Rm<T>::rsqrt(vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2] + vs2);
  sfor<3>([&](auto r) ABRK_LAMBDA { F[r()] += fn * s[r()] - ft * vt[r()]; });
  return delta;
}

// One tick of row b: p = Tx(frame, q, off), Jp = J(frame, q, off)[:3], v = Jp dq, F = the sum over the row's surfaces,
// tau[b] (+)= Jp^T F and, where asked for, the report.  Columns of Jp past the frame's joints are zero (jacobian()), so
// those entries of tau_c are exact zeros.
template <class A, class T>
ABRK_INL void contact_body(long b, const A& arm, const ContactP<T>& P, const ContactIO<T>& io) {
  constexpr int N = A::N;
  T q[N];
  load_row<N>(io.q, b, q);
  Joints<A, T> jt;
  T XR[9], xo[3];
  FrameCap<T> cap;
  cap.frame = P.frame;
  sfor<9>([&](auto e) ABRK_LAMBDA { cap.R[e()] = T(0); });
  sfor<3>([&](auto r) ABRK_LAMBDA { cap.o[r()] = T(0); });
  T sv[N][2];
  sincos_all<N>(q, sv);
  fk_forward(arm, q, jt, XR, xo, cap, [](auto, const T(&)[3]) ABRK_LAMBDA {}, ScUse<T, N>{sv});
  T p[3];
  sfor<3>([&](auto r) ABRK_LAMBDA {
    p[r()] = cap.o[r()] + cap.R[r() * 3] * P.off[0] + cap.R[r() * 3 + 1] * P.off[1] + cap.R[r() * 3 + 2] * P.off[2];
  });
  T Jv[N][3], Jw[N][3];
  jacobian(jt, p, P.m, Jv, Jw);
  T v[3] = {T(0), T(0), T(0)};
  {
    T dq[N];
    load_row<N>(io.dq, b, dq);
    sfor<N>([&](auto i) ABRK_LAMBDA { sfor<3>([&](auto r) ABRK_LAMBDA { v[r()] += Jv[i()][r()] * dq[i()]; }); });
  }
  // the row's surfaces, one after the other (S is uniform over the launch): 8 values each, contiguous per lane
  T F[3] = {T(0), T(0), T(0)}, deepest = T(0);
  int touching = 0;
  const T* sp = io.surface + b * (long)(P.S * kContactSurfaceW);
  sfor<kContactMaxSurfaces>([&](auto k) ABRK_LAMBDA {
    if (k() < P.S) {
      T s[kContactSurfaceW];
      sfor<kContactSurfaceW>([&](auto e) ABRK_LAMBDA { s[e()] = sp[k() * kContactSurfaceW + e()]; });
      const T delta = contact_surface(s, p, v, P.vs2, F);
      deepest = (k() == 0 || delta > deepest) ? delta : deepest;
      touching += delta > T(0) ? 1 : 0;
    }
  });
  T tau[N];
  sfor<N>([&](auto i) ABRK_LAMBDA { tau[i()] = Jv[i()][0] * F[0] + Jv[i()][1] * F[1] + Jv[i()][2] * F[2]; });
  put_row<N>(io.tau, b, tau, P.accumulate);
  if (io.report) {
    T rep[kContactReportW];
    sfor<3>([&](auto r) ABRK_LAMBDA {
      rep[r()] = F[r()];
      rep[3 + r()] = cap.R[r()] * F[0] + cap.R[3 + r()] * F[1] + cap.R[6 + r()] * F[2];  // R^T F
    });
    rep[6] = deepest;
    rep[7] = T(touching);
    store_row<kContactReportW>(io.report, b, rep);
  }
}

}  // namespace abrk

// abrk_link_contact.h - whole-arm contact of a device-resident control loop: one row program that, once per tick, treats
// every link segment of the arm as a capsule, finds its closest point to each of the row's own sphere obstacles (the
// geometry of obstacles_row, abrk_ctrl.h) and turns penetration into the joint torque tau_c = sum Jx^T f, which the plant
// reads as its tau_ext.  Recorded into a plan beside the end-effector contact - { law; [contact]; link contact; plant
// step } - it lets an elbow hit what AvoidObstacles avoids.  Forward kinematics and the columns W_j (x - o_j) of the
// point Jacobian only: no N x 3 Jacobian per pair and no dynamics pass.  The force is that of the state at the START of
// the tick, held by the plant over its substeps (include/abrk.h, the stability note of the contact section).
// Like the other row programs it compiles for the host (tests/hostsim_link_contact).
#pragma once
#include <limits>

#include "abrk_rows.h"

namespace abrk {

constexpr int kLinkContactMaxObstacles = 8;  // include/abrk.h ABRK_LINK_CONTACT_MAX_OBSTACLES
constexpr int kLinkContactMaxSegments = 7;   // the joints of the largest arm (link_radius[7])
constexpr int kLinkObstacleW = 7;            // cx, cy, cz, R, k, c, mu
constexpr int kLinkContactReportW = 8;       // F world [3], deepest delta, pairs penetrated, segment, obstacle, t

template <class T>
struct LinkContactP {
  int K;                              // obstacles per row, 1..kLinkContactMaxObstacles
  T radius[kLinkContactMaxSegments];  // of segment i; < 0: the segment is off
  T vs2;                              // square of the smoothing speed of the friction law
  int accumulate;                     // != 0: tau += tau_c
};
template <class T>
struct LinkContactIO {
  const T *q, *dq;    // [B, N]
  const T* obstacle;  // [B, K, 7]: read with ordinary loads at every launch
  T* tau;             // [B, N]
  T* report;          // [B, 8] or null
};

// One tick of row b.  Segment i runs from the origin of joint_i to that of joint_i+1 (the EE for the last one) and is a
// body of link i+1, so joints 0..i move it: the velocity of its material point x is v = sum_{j<=i} W_j (x - o_j) dq_j
// and a force f there gives tau_j = (W_j (x - o_j)) . f for j <= i and an exact zero for j > i.
//
// A pair that does not penetrate is skipped by a BRANCH, not by selects.  What the branch guards is the i+1 columns, v,
// the force and the i+1 dot products - 60 (segment 0) to 250 (segment 5) fp64 instructions - and a select form would run
// all of it for every pair and then pay two v_cndmask per fp64 value kept (N + 3 + 4 of them).  Rows clear of everything
// are the common case in a loop that avoids its obstacles, so most wavefronts skip the block with one s_cbranch_execz;
// a divergent wavefront pays the block once, which is what the select form pays always (profiles/link_contact.md).
// The exact zeros follow at once: a skipped pair touches neither tau nor F.
template <class A, class T>
ABRK_INL void link_contact_body(long b, const A& arm, const LinkContactP<T>& P, const LinkContactIO<T>& io) {
  constexpr int N = A::N;
  static_assert(N <= kLinkContactMaxSegments, "link_radius holds one radius per joint");
  T q[N], dq[N];
  load_row<N>(io.q, b, q);
  Joints<A, T> jt;
  T XR[9], xo[3], pe[3];
  NoCap nc;
  T sv[N][2];
  sincos_all<N>(q, sv);
  fk_forward(arm, q, jt, XR, xo, nc, [](auto, const T(&)[3]) ABRK_LAMBDA {}, ScUse<T, N>{sv});
  mulBE_pt<A, T>(arm, XR, xo, pe);
  load_row<N>(io.dq, b, dq);

  T tau[N], F[3] = {T(0), T(0), T(0)};
  sfor<N>([&](auto i) ABRK_LAMBDA { tau[i()] = T(0); });
  T deepest = T(0), tbest = T(0);
  int touching = 0, seg = -1, obs = -1;
  bool pushed = false;
  const T* op = io.obstacle + b * (long)(P.K * kLinkObstacleW);
  for (int ob = 0; ob < P.K; ob++) {  // (uniform over the launch)
    T s[kLinkObstacleW];
    sfor<kLinkObstacleW>([&](auto e) ABRK_LAMBDA { s[e()] = op[ob * kLinkObstacleW + e()]; });
    sfor<N>([&](auto iic) ABRK_LAMBDA {
      constexpr int ii = iic();
      if (P.radius[ii] >= T(0)) {  // (uniform: a kernel argument)
        T p2[3], vl[3], vo[3];
        sfor<3>([&](auto r) ABRK_LAMBDA {
          if constexpr (ii == N - 1) p2[r()] = pe[r()];
          else p2[r()] = jt.o[ii + 1 < N ? ii + 1 : ii][r()];
          vl[r()] = p2[r()] - jt.o[ii][r()];
          vo[r()] = s[r()] - jt.o[ii][r()];
        });
        const T len2 = dot3(vl, vl);
        if (len2 > T(0)) {  // a zero-length segment is skipped, as in obstacles_row
          T t = dot3(vo, vl) * Rm<T>::rcp(len2);
          t = t < T(0) ? T(0) : (t > T(1) ? T(1) : t);
          T x[3], e[3];
          sfor<3>([&](auto r) ABRK_LAMBDA {
            x[r()] = t == T(1) ? p2[r()] : jt.o[ii][r()] + t * vl[r()];
            e[r()] = x[r()] - s[r()];
          });
          const T d2 = dot3(e, e);
          const T id = d2 > T(0) ? Rm<T>::rsqrt(d2 > T(0) ? d2 : T(1)) : T(0);  // d == 0: n = 0
          const T delta = s[3] + P.radius[ii] - d2 * id;
          if (seg < 0 || delta > deepest) {
            deepest = delta;
            seg = ii;
            obs = ob;
            tbest = t;
          }
          if (delta > T(0)) {
            touching += 1;
            T col[ii + 1][3], v[3] = {T(0), T(0), T(0)};
            sfor<ii + 1>([&](auto j) ABRK_LAMBDA {
              const T dl[3] = {x[0] - jt.o[j()][0], x[1] - jt.o[j()][1], x[2] - jt.o[j()][2]};
              wapply<j()>(jt, dl, col[j()]);
              sfor<3>([&](auto r) ABRK_LAMBDA { v[r()] += col[j()][r()] * dq[j()]; });
            });
            const T n[3] = {e[0] * id, e[1] * id, e[2] * id};
            const T vn = dot3(n, v);
            const T push = s[4] * delta - s[5] * vn;
            const T fn = push > T(0) ? push : T(0);
            T vt[3], f[3];
            sfor<3>([&](auto r) ABRK_LAMBDA { vt[r()] = v[r()] - vn * n[r()]; });
            const T ft = s[6] * fn * Rm<T>::rsqrt(dot3(vt, vt) + P.vs2);
            sfor<3>([&](auto r) ABRK_LAMBDA {
              f[r()] = fn * n[r()] - ft * vt[r()];
              F[r()] += f[r()];
            });
            sfor<ii + 1>([&](auto j) ABRK_LAMBDA { tau[j()] += dot3(col[j()], f); });
            pushed = pushed || fn > T(0);
          }
        }
      }
    });
  }
  // a row that nothing pushes: tau_c = 0 exactly; with accumulate its tau is not rewritten (to the bit)
  if (pushed) {
    put_row<N>(io.tau, b, tau, P.accumulate);
  } else if (!P.accumulate) {
    store_row<N>(io.tau, b, tau);  // (a pair that penetrates with fn = 0 added +-0 to +0: still +0)
  }
  if (io.report) {
    T rep[kLinkContactReportW];
    sfor<3>([&](auto r) ABRK_LAMBDA { rep[r()] = F[r()]; });
    rep[3] = seg < 0 ? std::numeric_limits<T>::lowest() : deepest;  // (no active pair: every segment on has zero length)
    rep[4] = T(touching);
    rep[5] = T(seg);
    rep[6] = T(obs);
    rep[7] = tbest;
    store_row<kLinkContactReportW>(io.report, b, rep);
  }
}

}  // namespace abrk

// hostsim.cpp - TEST AID ONLY.  Compiles the row programs of abr_control_amd/csrc
// (abrk_rows.h: exactly what one GPU lane executes) for the HOST so that the kernel
// arithmetic can be checked against the oracle in a container without a GPU, before GPU
// minutes are spent.  Nothing in abr_control_amd/ loads this library; the product path is
// libabrk.so and fails loudly without a HIP device.
#define ABRK_HD __host__ __device__
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../abr_control_amd/csrc/abrk_osc6_plan.h"
#include "../../abr_control_amd/csrc/abrk_params.h"
#include "../../abr_control_amd/csrc/abrk_rows.h"
#include "../../abr_control_amd/csrc/abrk_rt.h"
#include "../../abr_control_amd/csrc/abrk_select.h"

using namespace abrk;

// The library is built in parts (parallel compilation, see tests/hostsim/__init__.py):
//   HOSTSIM_STATIC=1            the five built-in arms
//   HOSTSIM_RT_LO / HOSTSIM_RT_HI   runtime-table arms with LO..HI joints
//   HOSTSIM_LAW=1               the law-only row program
#ifndef HOSTSIM_STATIC
#define HOSTSIM_STATIC 0
#endif
#ifndef HOSTSIM_RT_LO
#define HOSTSIM_RT_LO 1
#define HOSTSIM_RT_HI 0
#endif
#ifndef HOSTSIM_LAW
#define HOSTSIM_LAW 0
#endif

namespace {
template <class A, class T>
int run_dyn(const A& arm, int n, int64_t B, const void* q, const void* dq, int frame, const double* off,
            unsigned want, void* const* outs) {
  DynOutP<T> o;
  T** po = reinterpret_cast<T**>(&o);
  for (int i = 0; i < 10; i++) po[i] = static_cast<T*>(outs[i]);
  int m = frame_m(frame, n);
  T ox = T(off ? off[0] : 0), oy = T(off ? off[1] : 0), oz = T(off ? off[2] : 0);
  DirectStore<T> st;
  auto rows = [&](auto with_dq) {
    for (long b = 0; b < B; b++)
      dyn_body<A, T, with_dq()>(b, true, st, arm, frame, m, ox, oy, oz, want, (long)B, (const T*)q, (const T*)dq, o);
  };
  if (dyn_with_dq(want)) rows(std::true_type{});
  else rows(std::false_type{});
  return 0;
}
// The variant of an OSC call, decided where the launcher decides it (abrk_select.h): the integral state is dropped for
// ki == 0 as the host layer stages it.  with_variant: f(OscV) for the law alone (FULL = false) or the fused row program;
// -1 for a variant of the other family (the aid has no EEF form: the same bits)
template <class T>
OscVariant variant_of(const abrk_osc_params& P, const OscP<T>& p, int n, const void* tv, void*& ie, const void* une,
                      const void* ts, unsigned want) {
  if (P.ki == 0) ie = nullptr;
  return osc_variant(osc_fast_rows(P, n, une != nullptr), n, P.use_C != 0, p.n_null, tv != nullptr, ie != nullptr,
                     une != nullptr, ts != nullptr, want);
}
template <class A, bool FULL, class F>
int with_variant(const OscVariant& v, F&& f) {
  return with_osc_variant<A>(v, [&](auto vt) {
    using V = decltype(vt);
    if constexpr (V::full == FULL && !V::eef) return f(vt);
    else return -1;
  });
}
template <class A, class T>
int run_osc(const A& arm, int n, const abrk_osc_params* P, int64_t B, const void* q, const void* dq,
            const void* tg, const void* tv, void* ie, const void* une, void* u, void* ts) {
  OscP<T> p = make_oscp<T>(*P, n);
  const OscVariant v = variant_of(*P, p, n, tv, ie, une, ts, 0);
  return with_variant<A, false>(v, [&](auto vt) {
    using V = decltype(vt);
    for (long b = 0; b < B; b++) {
      // (NOTS: what every pass of the plain six-row kernels runs when no training signal is asked for - the gravity
      //  term folded into the velocity term ahead of the factorisations)
      std::conditional_t<V::nots, NoTs<RegScratch<T, A::N>>, RegScratch<T, A::N>> scr;
      osc_body<A, T, V::km, V::use_c, V::feat>(b, arm, p, (long)B, (const T*)q, (const T*)dq, (const T*)tg,
                                               (const T*)tv, (T*)ie, (const T*)une, (T*)u, (T*)ts, scr);
    }
    return 0;
  });
}
// the six-row law in its two-pass, hand-over form (what libabrk launches for batches of up to 262144 rows): the first
// pass compiled WITHOUT the eigen-decomposition (DeferOnly), a deferring row parks itself in the worklist and leaves its
// record (osc_law6), osc6_finish_row then completes it from the record alone - here with all N + 2 columns on one
// "lane"; the GPU's wave-cooperative kernel runs the same arithmetic with one column per lane
template <class A, class T>
int run_osc_handover(const A& arm, int n, const abrk_osc_params* P, int64_t B, const void* q, const void* dq,
                     const void* tg, const void* tv, void* ie, const void* une, void* u, void* ts,
                     int64_t* n_deferred) {
  OscP<T> p = make_oscp<T>(*P, n);
  const OscVariant v = variant_of(*P, p, n, tv, ie, une, ts, 0);
  if (v.km != 6) return -1;
  const bool nulls = p.n_null > 0 || une != nullptr;
  // hand-over mode as on the device, rows one by one: the record of row b at rec[b] (the device packs a chunk's records
  // at the chunk's first slots - ScratchBase::record - and carries the row's index in the record); which rows deferred is
  // the kernel's business there (a ballot per 64-row chunk) and a plain flag array here
  std::vector<T> rec((size_t)B * rec_len(A::N), T(0));
  std::vector<char> flag((size_t)B, 0);
  const int rc = with_variant<A, false>(v, [&](auto vt) {
    using V = decltype(vt);
    if constexpr (V::km == 6) {
      for (long b = 0; b < B; b++) {
        using S = DeferOnly<RegScratch<T, A::N>>;
        std::conditional_t<V::nots, NoTs<S>, S> scr;
        scr.allow_defer = true;
        scr.rec_base = rec.data();
        scr.handover = true;
        scr.row = b;
        osc_body<A, T, 6, V::use_c, V::feat>(b, arm, p, (long)B, (const T*)q, (const T*)dq, (const T*)tg, (const T*)tv,
                                             (T*)ie, (const T*)une, (T*)u, (T*)ts, scr);
        flag[b] = scr.deferred;
      }
    }
    return 0;
  });
  if (rc != 0) return rc;
  int64_t total = 0;
  for (long b = 0; b < B; b++) {
    if (!flag[b]) continue;
    total++;
    T uu[A::N], tt[A::N];
    osc6_finish_row<A::N, T>(rec.data() + b * rec_len(A::N), nulls, uu, tt);
    store_row<A::N>((T*)u, b, uu);
    if (ts) store_row<A::N>((T*)ts, b, tt);
  }
  if (n_deferred) *n_deferred = total;
  return 0;
}
// the fused "u + Tx, J, M, g" row program (osc_full_body), the variant Launch::osc takes for `want`
template <class A, class T>
int run_osc_full(const A& arm, int n, const abrk_osc_params* P, int64_t B, const void* q, const void* dq,
                 const void* tg, const void* tv, void* ie, const void* une, void* u, void* ts, unsigned want,
                 void* const* outs) {
  OscP<T> p = make_oscp<T>(*P, n);
  const OscVariant v = variant_of(*P, p, n, tv, ie, une, ts, want);
  DynOutP<T> o{};
  o.Tx = (T*)outs[0];
  o.J = (T*)outs[1];
  o.M = (T*)outs[2];
  o.g = (T*)outs[3];
  o.C = (T*)outs[4];
  o.dJ = (T*)outs[5];
  DirectStore<T> st;
  RegScratch<T, A::N> scr;
  return with_variant<A, true>(v, [&](auto vt) {
    using V = decltype(vt);
    for (long b = 0; b < B; b++)
      osc_full_body<A, T, V::km, V::use_c, V::feat, V::vel>(b, true, st, arm, p, (long)B, (const T*)q, (const T*)dq,
                                                            (const T*)tg, (const T*)tv, (T*)ie, (const T*)une, (T*)u,
                                                            (T*)ts, want, o, scr);
    return 0;
  });
}
template <class A, class T>
int run_sliding(const A& arm, int n, const abrk_sliding_params* P, int64_t B, const void* q, const void* dq,
                const void* tg, const void* tv, const void* ta, void* u, void* s) {
  SlidingP<T> p = make_slidingp<T>(*P, n);
  for (long b = 0; b < B; b++)
    sliding_body<A, T>(b, arm, p, (long)B, (const T*)q, (const T*)dq, (const T*)tg, (const T*)tv, (const T*)ta,
                       (T*)u, (T*)s);
  return 0;
}
template <class A, class T>
int run_joint(const A& arm, int n, const abrk_null_ctrl* c, int grav, int64_t B, const void* q, const void* dq,
              const void* tg, const void* tv, void* u) {
  JointP<T> p = make_jointp<T>(*c, grav);
  for (long b = 0; b < B; b++)
    joint_body<A, T>(b, arm, p, (long)B, (const T*)q, (const T*)dq, (const T*)tg, (const T*)tv, (T*)u);
  return 0;
}

// dispatch over (arm kind, dtype): static built-in by name, or runtime table by joint count
template <class F>
int with_arm(const char* name, const abrk_arm_desc* d, int dtype, F&& f) {
#define STATIC_CASE(NM)                                                                     \
  if (name && !strcmp(name, #NM)) {                                                         \
    StaticArm<Tab_##NM> a;                                                                  \
    return dtype == 0 ? f(a, double(0), Tab_##NM::N) : f(a, float(0), Tab_##NM::N);         \
  }
#if HOSTSIM_STATIC
  STATIC_CASE(ur5) STATIC_CASE(jaco2) STATIC_CASE(twojoint) STATIC_CASE(threejoint) STATIC_CASE(onejoint)
#endif
#undef STATIC_CASE
  if (!d) return -4;
  return for_joints(d->n_joints, [&](auto nn) {
    constexpr int NN = decltype(nn)::value;
    if constexpr (HOSTSIM_RT_LO <= NN && NN <= HOSTSIM_RT_HI) {
      return for_dtype(dtype, [&](auto t) {
        RtArm<NN, decltype(t)> a;
        rt_fill<NN, decltype(t)>(d, &a);
        return f(a, t, NN);
      });
    } else {
      return -4;
    }
  }, -4);
}
}  // namespace

extern "C" int hostsim_dynamics(const char* builtin, const abrk_arm_desc* d, int dtype, int64_t B, const void* q,
                                const void* dq, int frame, const double* off, uint32_t want,
                                const abrk_dyn_out* out) {
  void* const* outs = reinterpret_cast<void* const*>(out);
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int n) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    return run_dyn<A, T>(a, n, B, q, dq, frame, off, want, outs);
  });
}
extern "C" int hostsim_osc(const char* builtin, const abrk_arm_desc* d, int dtype, const abrk_osc_params* P,
                           int64_t B, const void* q, const void* dq, const void* tg, const void* tv, void* ie,
                           const void* une, void* u, void* ts) {
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int n) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    return run_osc<A, T>(a, n, P, B, q, dq, tg, tv, ie, une, u, ts);
  });
}
extern "C" int hostsim_osc_handover(const char* builtin, const abrk_arm_desc* d, int dtype, const abrk_osc_params* P,
                                    int64_t B, const void* q, const void* dq, const void* tg, const void* tv, void* ie,
                                    const void* une, void* u, void* ts, int64_t* n_deferred) {
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int n) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    return run_osc_handover<A, T>(a, n, P, B, q, dq, tg, tv, ie, une, u, ts, n_deferred);
  });
}
extern "C" int hostsim_osc_full(const char* builtin, const abrk_arm_desc* d, int dtype, const abrk_osc_params* P,
                                int64_t B, const void* q, const void* dq, const void* tg, const void* tv, void* ie,
                                const void* une, void* u, void* ts, uint32_t want, const abrk_dyn_out* out) {
  void* const* outs = reinterpret_cast<void* const*>(out);
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int n) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    return run_osc_full<A, T>(a, n, P, B, q, dq, tg, tv, ie, une, u, ts, want, outs);
  });
}
extern "C" int hostsim_sliding(const char* builtin, const abrk_arm_desc* d, int dtype,
                               const abrk_sliding_params* P, int64_t B, const void* q, const void* dq,
                               const void* tg, const void* tv, const void* ta, void* u, void* s) {
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int n) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    return run_sliding<A, T>(a, n, P, B, q, dq, tg, tv, ta, u, s);
  });
}
extern "C" int hostsim_joint(const char* builtin, const abrk_arm_desc* d, int dtype, const abrk_null_ctrl* c,
                             int grav, int64_t B, const void* q, const void* dq, const void* tg, const void* tv,
                             void* u) {
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int n) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    return run_joint<A, T>(a, n, c, grav, B, q, dq, tg, tv, u);
  });
}

extern "C" int hostsim_floating(const char* builtin, const abrk_arm_desc* d, int dtype, int dynamic, int task_space,
                                int64_t B, const void* q, const void* dq, void* u, int acc) {
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    for (long b = 0; b < B; b++) floating_body<A, T>(b, a, dynamic, task_space, (const T*)q, (const T*)dq, (T*)u, acc);
    return 0;
  });
}
// plain != 0: the one-pass row program everywhere; else what libabrk dispatches - the split program (phase A, one heavy
// pair at a time, finish) on orthogonal chains of three joints and more with at most 64 heavy slots
extern "C" int hostsim_obstacles(const char* builtin, const abrk_arm_desc* d, int dtype,
                                 const abrk_obstacles_params* P, int64_t B, const void* q, void* u, int acc, int plain) {
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    ObsP<T> p = make_obsp<T>(*P);
    const bool split = !plain && obstacles_split<A>(p.n);
    for (long b = 0; b < B; b++) {
      if (split) obstacles_split_body<A, T>(b, a, p, (const T*)q, (T*)u, acc);
      else obstacles_body<A, T>(b, a, p, (const T*)q, (T*)u, acc);
    }
    return 0;
  });
}

#if HOSTSIM_LAW
// the form a six-row OSC call of B rows takes (abrk_osc6_plan.h).  sw: no_defer, no_handover, handover_max, dense_max,
// finish_slots, finish_rounds, finish_group - bit i of `given` set: sw[i] replaces what ships; out: form, slots, rounds, group
extern "C" int hostsim_osc6_plan(int64_t B, unsigned given, const int64_t* sw, int* out) {
  Osc6Switches s;
  if (given & 1) s.no_defer = sw[0] != 0;
  if (given & 2) s.no_handover = sw[1] != 0;
  if (given & 4) s.handover_max = (long)sw[2];
  if (given & 8) s.dense_max = (long)sw[3];
  if (given & 16) s.finish_slots = (int)sw[4];
  if (given & 32) s.finish_rounds = (int)sw[5];
  if (given & 64) s.finish_group = (int)sw[6];
  const Osc6Plan p = osc6_plan((long)B, s);
  out[0] = (int)p.form;
  out[1] = p.slots;
  out[2] = p.rounds;
  out[3] = p.group;
  return 0;
}

// the variant an OSC call takes (abrk_select.h `osc_variant`; integrated_error counts where ki != 0, as the host layer
// stages it); out: km, use_c, feat, nots, full, vel
extern "C" int hostsim_osc_variant(int fast, int n, int use_C, int n_null, int tv, int ki_nonzero, int ie, int une,
                                   int ts, unsigned want, int* out) {
  const OscVariant v = osc_variant(fast, n, use_C != 0, n_null, tv != 0, ki_nonzero && ie, une != 0, ts != 0, want);
  out[0] = v.km;
  out[1] = v.use_c;
  out[2] = v.feat;
  out[3] = v.nots;
  out[4] = v.full;
  out[5] = v.vel;
  return 0;
}

extern "C" int hostsim_limits(int n, int dtype, const abrk_limits_params* P, int64_t B, const void* q, void* u,
                              int acc) {
  return for_joints_and_dtype(n, dtype, [&](auto nn, auto t) {
    using T = decltype(t);
    LimitsP<T> p = make_limitsp<T>(*P);
    for (long b = 0; b < B; b++) limits_body<nn(), T>(b, p, (const T*)q, (T*)u, acc);
    return 0;
  }, -1);
}

extern "C" int hostsim_osc_mx(int n, int k, int dtype, int64_t B, const void* M, const void* J, double thr, void* Mx,
                              void* Minv) {
  return for_joints_and_dtype(n, dtype, [&](auto nn, auto t) {
    using T = decltype(t);
    for (long b = 0; b < B; b++) mx_body<nn(), T>(b, k, T(thr), (const T*)M, (const T*)J, (T*)Mx, (T*)Minv);
    return 0;
  }, -1);
}
// the direct symmetric 3x3 eigen-solver on its own (A: [B,3,3] symmetric; lam [B,3], V [B,3,3] columns = eigenvectors)
// the 6 x 6 eigen-solvers behind the six-row law's truncating pinv: method 0 = cyclic Jacobi, 1 = Householder + QL
extern "C" int hostsim_sym6_eig(int method, int64_t B, const double* A, double* lam, double* V) {
  for (long b = 0; b < B; b++) {
    double S[21], Vv[6][6], l[6];
    for (int r = 0; r < 6; r++)
      for (int c = 0; c <= r; c++) S[tri(r, c)] = A[b * 36 + r * 6 + c];
    if (method == 0) jacobi_eig<6, double>(S, Vv, l);
    else ql_eig<6, double>(S, Vv, l);
    for (int r = 0; r < 6; r++) {
      lam[b * 6 + r] = l[r];
      for (int c = 0; c < 6; c++) V[b * 36 + r * 6 + c] = Vv[r][c];
    }
  }
  return 0;
}
// the truncating pseudo-inverse + tail of the six-row law on its own (abrk_ctrl.h osc6_tail: early-exit QL + tridiagonal
// solve): A [B,6,6] symmetric, G [B,8,6] (columns of [J | u_task | J v], six joints), b [B,12] (b1, b2) -> out [B,12]
// (u, ts), info [B,2] (index of the last eigenvalue the iteration isolated: -1 none ... 5 all; the cut-off it used)
extern "C" int hostsim_osc6_tail(int64_t B, const double* A, const double* G, const double* b, double* out, double* info) {
  for (long k = 0; k < B; k++) {
    double S[21], Gm[8][6], b1[6], b2[6], u[6], ts[6];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j <= i; j++) S[tri(i, j)] = A[k * 36 + i * 6 + j];
    for (int c = 0; c < 8; c++)
      for (int r = 0; r < 6; r++) Gm[c][r] = G[k * 48 + c * 6 + r];
    for (int i = 0; i < 6; i++) {
      b1[i] = b[k * 12 + i];
      b2[i] = b[k * 12 + 6 + i];
    }
    {
      double G2[1][6] = {{0, 0, 0, 0, 0, 0}}, lam[6];
      QlTail<6, double> t;
      t.rcond = 1e-4;
      ql_core<6, double, 1, false, false, true>(S, G2, lam, &t);
      info[k * 2] = t.lexit;
      info[k * 2 + 1] = t.cut;
    }
    osc6_tail<6, double>(S, Gm, b1, b2, true, u, ts);
    for (int i = 0; i < 6; i++) {
      out[k * 12 + i] = u[i];
      out[k * 12 + 6 + i] = ts[i];
    }
  }
  return 0;
}
// the cofactor inverse of the x,y,z / x,y law (abrk_ctrl.h `spd_inverse_small`): A [B,K,K] symmetric -> inv [B,K,K],
// det [B], ok [B]
extern "C" int hostsim_spd_inverse_small(int K, int64_t B, const double* A, double* inv, double* det, int* ok) {
  for (long b = 0; b < B; b++) {
    if (K == 3) {
      double S[6], I[6], d;
      for (int r = 0; r < 3; r++)
        for (int c = 0; c <= r; c++) S[tri(r, c)] = A[b * 9 + r * 3 + c];
      ok[b] = spd_inverse_small<3, double>(S, I, d) ? 1 : 0;
      det[b] = d;
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) inv[b * 9 + r * 3 + c] = I[tri(r > c ? r : c, r > c ? c : r)];
    } else if (K == 2) {
      double S[3], I[3], d;
      for (int r = 0; r < 2; r++)
        for (int c = 0; c <= r; c++) S[tri(r, c)] = A[b * 4 + r * 2 + c];
      ok[b] = spd_inverse_small<2, double>(S, I, d) ? 1 : 0;
      det[b] = d;
      for (int r = 0; r < 2; r++)
        for (int c = 0; c < 2; c++) inv[b * 4 + r * 2 + c] = I[tri(r > c ? r : c, r > c ? c : r)];
    } else {
      return -1;
    }
  }
  return 0;
}
extern "C" int hostsim_sym3_eig(int dtype, int64_t B, const void* A, void* lam, void* V) {
  auto run = [&](auto tag) {
    using T = decltype(tag);
    const T* a = (const T*)A;
    for (long b = 0; b < B; b++) {
      T S[6], Vv[3][3], l[3];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c <= r; c++) S[tri(r, c)] = a[b * 9 + r * 3 + c];
      sym3_eig<T>(S, Vv, l);
      for (int r = 0; r < 3; r++) {
        ((T*)lam)[b * 3 + r] = l[r];
        for (int c = 0; c < 3; c++) ((T*)V)[b * 9 + r * 3 + c] = Vv[r][c];
      }
    }
  };
  if (dtype == 0) run(double{});
  else run(float{});
  return 0;
}
extern "C" int hostsim_velocity_limiting(int dtype, const abrk_osc_params* P, int64_t B, const void* in, void* out) {
  for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    for (long b = 0; b < B; b++)
      velocity_limiting_body<T>(b, T(P->kp), T(P->ko), T(P->kv), T(P->vmax[0]), T(P->vmax[1]), (const T*)in, (T*)out);
  });
  return 0;
}
extern "C" int hostsim_orientation_forces(int alg, int dtype, int64_t B, const void* R, const void* abg, void* out) {
  for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    for (long b = 0; b < B; b++) orientation_forces_body<T>(b, alg, (const T*)R, (const T*)abg, (T*)out);
  });
  return 0;
}

extern "C" int hostsim_osc_law(int n, int dtype, const abrk_osc_params* P, int64_t B, const void* J, const void* M,
                               const void* g, const void* c, const void* xyz, const void* R, const void* q,
                               const void* dq, const void* tg, const void* tv, void* ie, const void* une, void* u,
                               void* ts) {
  if (P->ki == 0) ie = nullptr;
  if (!P->use_g) g = nullptr;
  if (!P->use_C) c = nullptr;
  return for_joints_and_dtype(n, dtype, [&](auto nn, auto t) {
    using T = decltype(t);
    OscP<T> p = make_oscp<T>(*P, n);
    for (long b = 0; b < B; b++)
      osc_law_body<nn(), T>(b, p, (long)B, (const T*)J, (const T*)M, (const T*)g, (const T*)c, (const T*)xyz,
                            (const T*)R, (const T*)q, (const T*)dq, (const T*)tg, (const T*)tv, (T*)ie, (const T*)une,
                            (T*)u, (T*)ts);
    return 0;
  }, -1);
}

#endif

extern "C" int hostsim_rollout(const char* builtin, const abrk_arm_desc* d, int dtype, const abrk_osc_params* P,
                               const abrk_twolink_plant* plant, int64_t B, int n_steps, int every, void* q, void* dq,
                               const void* tg, void* qt, void* dqt, void* ut) {
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int n) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    if constexpr (A::N == 2) {
      OscP<T> p = make_oscp<T>(*P, n);
      TwoLinkP<T> k{T(plant->K1), T(plant->K2), T(plant->K3), T(plant->K4), T(plant->dt)};
      with_rollout_variant(osc_fast_rows(*P, n, false), P->use_C != 0, [&](auto uc, auto km) {
        for (long b = 0; b < B; b++)
          rollout_body<A, T, uc(), km()>(b, a, p, k, (long)B, n_steps, every, (T*)q, (T*)dq, (const T*)tg, (T*)nullptr,
                                         (T*)qt, (T*)dqt, (T*)ut);
      });
      return 0;
    } else {
      return -1;
    }
  });
}

extern "C" int hostsim_ik(const char* builtin, const abrk_arm_desc* d, int dtype, const abrk_ik_params* P, int64_t B,
                          const void* q, const void* tg, void* pp, void* vp) {
  return with_arm(builtin, d, dtype, [&](const auto& a, auto t, int n) {
    using A = std::decay_t<decltype(a)>;
    using T = decltype(t);
    IkP<T> p{T(P->max_dx * P->dt), T(P->max_dr * P->dt), T(P->max_dq * P->dt), P->n_timesteps, P->method};
    for (long b = 0; b < B; b++) ik_body<A, T>(b, a, p, (long)B, (const T*)q, (const T*)tg, (T*)pp, (T*)vp);
    return 0;
  });
}

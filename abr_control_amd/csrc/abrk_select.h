// abrk_select.h - which template instantiation a call runs: the OSC kernel variant <KM, USE_C, FEAT, NOTS / VEL>, the
// rollout's (use_C, KM), the dynamics' WITH_DQ, the AvoidObstacles split, and the "1..7 joints x double / float" switches.
// Plain C++17, no HIP types: the launchers (abrk_kernels.h, abrk_law.hip), tests/hostsim and tools/microbench all ask
// here - the ONLY place where `fast`, `use_C`, the optional inputs and `want` are turned into template arguments
// (tests/test_osc_variant.py pins the rule).
#pragma once
#include <type_traits>

namespace abrk {

template <int I>
using int_c = std::integral_constant<int, I>;  // (abrk_device.h `ic<I>`)

constexpr unsigned kWantVelocityOutputs = 1u << 4 | 1u << 5;  // W_C | W_DJ (abrk_rows.h)
// dyn_kernel / dyn_body<.., WITH_DQ>: the velocity-dependent outputs are asked for
constexpr bool dyn_with_dq(unsigned want) { return (want & kWantVelocityOutputs) != 0; }

// km: task rows the kernel is specialised for - 3 (x,y,z), 2 (x,y; arms of up to three joints), 6 (the masked six-row law).
// feat: 0 no optional input, 1 fused null controllers only, 2 anything else.  nots: the plain six-row law of a caller who
// asks for no training signal (ScratchBase::kNoTs).  full: the fused kernel that also writes Tx / J / M / g / C / dJ
// (osc_full_kernel), vel: with C / dJ among them.
struct OscVariant {
  int km;
  bool use_c;
  int feat;
  bool nots, full, vel;
};
// EVERY form of the plain six-row law runs the NOTS arithmetic when no training signal is asked for (gravity joins the
// velocity term before the factorisations) - first pass, recompute pass, one-pass: a row's bits do not depend on the
// batch it arrives in
constexpr bool osc_nots(int km, int feat, bool ts) { return km == 6 && feat == 0 && !ts; }
// fast: abrk_params.h osc_fast_rows.  tv / ierr / une: target_velocity, integrated_error (nulled by the caller where
// ki == 0) and u_null_ext are present; ts: a training signal is asked for; want: W_* bits of the fused outputs.
constexpr OscVariant osc_variant(int fast, int n_joints, bool use_c, int n_null, bool tv, bool ierr, bool une, bool ts,
                                 unsigned want) {
  OscVariant v{6, use_c, 0, false, want != 0, false};
  const bool other = tv || ierr || une;
  if (v.full) {
    // the two-row kernel of the planar examples is not duplicated: x,y control of a small arm takes the six-row form.
    // C / dJ among the outputs: the variant whose dynamics pass assembles the Christoffel matrix (FEAT 2 only: the
    // velocity-dependent outputs are the rarer request and one instantiation per (KM, use_C) keeps the build in bounds)
    if (fast == 3) v.km = 3;
    v.vel = dyn_with_dq(want);
    v.feat = v.vel || other || n_null > 0 ? 2 : 0;
    return v;
  }
  if (fast == 3) v.km = 3;
  else if (fast == 2 && n_joints <= 3) v.km = 2;
  v.feat = other ? 2 : n_null > 0 ? 1 : 0;
  v.nots = osc_nots(v.km, v.feat, ts);
  return v;
}

// The first pass of the plain six-row law has an instantiation for "ref_frame is the end effector" (EEF: no frame
// capture in the forward kinematics; the same bits) - the reference benchmark's setting.  Built for orthogonal
// built-in / compiled chains, whose first pass holds two waves per SIMD (where it was measured, UR5 8 M rows -1.6 %);
// general chains keep the capture (their EEF first pass faulted on the four-joint test arm: profiles/round6/NOTES.md
// section 2), and so do general-inertia arms (measured on plain chains only).  EVERY pass of such a launch takes the
// EEF form: the capture changes the basic-block structure of the forward kinematics, and with it which multiply the
// compiler fuses with which add - a row's bits must not depend on the pass that evaluates it.
template <class A>
constexpr bool osc_eef_built(int km, int feat) { return A::kOrtho && !A::kGI && km == 6 && feat == 0; }
template <class A>
constexpr bool osc_eef(const OscVariant& v, int ref_frame) {
  return !v.full && osc_eef_built<A>(v.km, v.feat) && ref_frame == 2 * A::N + 1;
}

// A variant as a type: what the visitors below hand to `f`
template <int KM, bool UC, int FEAT, bool NOTS = false, bool EEF = false, bool FULL = false, bool VEL = false>
struct OscV {
  static constexpr int km = KM, feat = FEAT;
  static constexpr bool use_c = UC, nots = NOTS, eef = EEF, full = FULL, vel = VEL;
};
// the NOTS / EEF twins of one kernel <KM, UC, FEAT>: they exist for the plain six-row law alone
template <class A, int KM, bool UC, int FEAT, class F>
constexpr auto with_osc_twin(bool nots, bool eef, F&& f) {
  if constexpr (osc_eef_built<A>(KM, FEAT)) {
    if (eef) return nots ? f(OscV<KM, UC, FEAT, true, true>{}) : f(OscV<KM, UC, FEAT, false, true>{});
  }
  if constexpr (KM == 6 && FEAT == 0) {
    if (nots) return f(OscV<KM, UC, FEAT, true>{});
  }
  return f(OscV<KM, UC, FEAT>{});
}
// f(OscV<...>{}) for the variant `v` of arm policy A - exactly the instantiations that are built: KM 2 for arms of up
// to three joints, the fused kernel for KM 3 / 6 with FEAT 0, FEAT 2 and FEAT 2 + VEL
template <class A, class F>
constexpr auto with_osc_variant(const OscVariant& v, bool eef, F&& f) {
  auto on_feat = [&](auto km, auto uc) {
    constexpr int KM = decltype(km)::value;
    constexpr bool UC = decltype(uc)::value;
    if constexpr (KM != 2) {
      if (v.full) {
        if (v.vel) return f(OscV<KM, UC, 2, false, false, true, true>{});
        return v.feat == 0 ? f(OscV<KM, UC, 0, false, false, true>{}) : f(OscV<KM, UC, 2, false, false, true>{});
      }
    }
    if (v.feat == 2) return with_osc_twin<A, KM, UC, 2>(v.nots, eef, f);
    if (v.feat == 1) return with_osc_twin<A, KM, UC, 1>(v.nots, eef, f);
    return with_osc_twin<A, KM, UC, 0>(v.nots, eef, f);
  };
  auto on_use_c = [&](auto km) { return v.use_c ? on_feat(km, std::true_type{}) : on_feat(km, std::false_type{}); };
  if (v.km == 3) return on_use_c(int_c<3>{});
  if constexpr (A::N <= 3) {
    if (v.km == 2 && !v.full) return on_use_c(int_c<2>{});
  }
  return on_use_c(int_c<6>{});
}
template <class A, class F>
constexpr auto with_osc_variant(const OscVariant& v, F&& f) { return with_osc_variant<A>(v, false, f); }

// the fused rollout (two-joint arms): f(use_C, KM) - x,y takes the two-row law, everything else the six-row one
template <class F>
constexpr auto with_rollout_variant(int fast, bool use_c, F&& f) {
  auto on_km = [&](auto uc) { return fast == 2 ? f(uc, int_c<2>{}) : f(uc, int_c<6>{}); };
  return use_c ? on_km(std::true_type{}) : on_km(std::false_type{});
}

// AvoidObstacles with the heavy (obstacle, segment) pairs redistributed over the wavefront (obstacles_lds_kernel; row
// level: obstacles_split_body): orthogonal chains of three joints and more, up to 64 heavy slots
template <class A>
constexpr bool obstacles_split_built() { return A::kOrtho && A::N >= 3; }
template <class A>
constexpr bool obstacles_split(int n_obstacles) {
  if constexpr (obstacles_split_built<A>()) return n_obstacles * (A::N - 2) <= 64;
  else return false;
}

// f(T(0)) for the arithmetic type of dtype code 0 (double) / 1 (float)
template <class F>
constexpr auto for_dtype(int dtype, F&& f) { return dtype == 0 ? f(double(0)) : f(float(0)); }
// f(int_c<n>{}) for 1 .. 7 joints; `bad` for any other count
template <class F, class R>
constexpr auto for_joints(int n, F&& f, R bad) -> decltype(f(int_c<1>{})) {
  switch (n) {
    case 1: return f(int_c<1>{});
    case 2: return f(int_c<2>{});
    case 3: return f(int_c<3>{});
    case 4: return f(int_c<4>{});
    case 5: return f(int_c<5>{});
    case 6: return f(int_c<6>{});
    case 7: return f(int_c<7>{});
  }
  return bad;
}
// f(int_c<n>{}, T(0)): the arm-independent kernels, instantiated per joint count and arithmetic type
template <class F, class R>
constexpr auto for_joints_and_dtype(int n, int dtype, F&& f, R bad) {
  return for_joints(n, [&](auto nn) { return for_dtype(dtype, [&](auto t) { return f(nn, t); }); }, bad);
}

}  // namespace abrk

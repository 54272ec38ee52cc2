// abrk_adapt.h - the adaptive signal of a recorded loop: B independent populations of LIF neurons whose decoders learn
// by PES (what the reference's controllers/signals/DynamicsAdaptation builds out of Nengo's Lowpass, LIF / LIFRate and
// PES operators), one tick per launch.  The per-neuron row program, the argument block of the kernels in abrk_adapt.hip
// and their launchers.  Arm-independent: a translation unit of its own, not part of the plugin ABI tag.
//
// One tick of row b (DESIGN.md "Adaptive signal"); a(tau) = 1 - exp(-dt / tau), a(0) = 1:
//   1  x = (concat(in0[b], in1[b]) - shift) * scale;  x_f += a(tau_input) (x - x_f)
//   2  e_f += a(tau_training) (training[b] - e_f)
//   3  per neuron i: J = gain_i (enc_i . x_f) + bias_i;  s_i = the LIF / LIFRate step           (adapt_lif / adapt_lif_rate)
//   4  y_o = sum_i W[o,i] s_i                   with the weights from before this tick's update
//   5  out_f += a(tau_output) (y - out_f);  out[b] = out_f;  u_add[b] += out_f
//   6  a_f,i += a(tau_pre) (s_i - a_f,i)
//   7  W[o,i] += kappa e_f[o] a_f,i             kappa = pes_learning_rate dt / n_per_ensemble
// Steps 3, 4, 6 and 7 touch each neuron's state once: W[o,i] is read, used for y_o, updated and written back in one pass.
//
// The neuron functions are plain C++ and compile for the host as well (tests/hostsim_adapt defines ABRK_ADAPT_HD as
// __host__ __device__), so that the tick is checked against its NumPy statement without a GPU.
#ifndef ABRK_ADAPT_H
#define ABRK_ADAPT_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef ABRK_ADAPT_HD
#define ABRK_ADAPT_HD __device__
#endif
#define ABRK_ADAPT_INL ABRK_ADAPT_HD inline

namespace abrk {

constexpr int kAdaptBlock = 256;  // lanes of a workgroup (one workgroup per row): four wavefronts
constexpr int kAdaptWaves = kAdaptBlock / 64;
constexpr int kAdaptMaxD = 64;    // inputs: x_f of a row sits in LDS
constexpr int kAdaptMaxO = 16;    // outputs: one accumulator per output and lane, in registers
constexpr double kAdaptTauPre = 0.005;  // the PES pre-synaptic filter (Nengo's default pre_synapse)
enum { kAdaptLif = 0, kAdaptLifRate = 1 };

template <class T>
struct AdaptArgs {
  int D, O, N, w0, w1;
  long B;
  T a_in, a_tr, a_out, a_pre;  // a(tau) of the four filters
  T kappa, dt, inv_dt, tau_rc, tau_ref;
  const T *enc, *gain, *bias, *shift, *scale;  // shared: [N,D], [N], [N], [D], [D]
  const T *in0, *in1, *training;               // [B,w0], [B,w1] or null, [B,O]
  T *x_f, *e_f, *v, *ref, *a_f, *W, *out_f;    // per-row state: [B,D], [B,O], [B,N] x 3, [B,O,N], [B,O]
  T *out, *u_add;                              // [B,O]; u_add may be null
};

// launches the tick of a.B rows on `stream`; neuron_type: kAdaptLif | kAdaptLifRate.  No allocation, no sync.
hipError_t launch_adapt_step(int neuron_type, const AdaptArgs<double>& a, hipStream_t stream);
hipError_t launch_adapt_step(int neuron_type, const AdaptArgs<float>& a, hipStream_t stream);

// the argument block without its arrays (host side: the C entry point, and the host build of the tests).
// a(tau) = 1 - exp(-dt / tau), a(0) = 1; evaluated in double, then rounded to T
inline double adapt_lowpass_gain(double dt, double tau) { return tau > 0.0 ? -expm1(-dt / tau) : 1.0; }
template <class T>
inline AdaptArgs<T> adapt_make_args(int D, int O, int N, int n_per, int w0, int w1, long B, double dt, double tau_input,
                                    double tau_training, double tau_output, double tau_rc, double tau_ref,
                                    double pes_learning_rate) {
  AdaptArgs<T> a{};
  a.D = D;
  a.O = O;
  a.N = N;
  a.w0 = w0;
  a.w1 = w1;
  a.B = B;
  a.a_in = (T)adapt_lowpass_gain(dt, tau_input);
  a.a_tr = (T)adapt_lowpass_gain(dt, tau_training);
  a.a_out = (T)adapt_lowpass_gain(dt, tau_output);
  a.a_pre = (T)adapt_lowpass_gain(dt, kAdaptTauPre);
  a.kappa = (T)(pes_learning_rate * dt / (double)n_per);
  a.dt = (T)dt;
  a.inv_dt = (T)(1.0 / dt);
  a.tau_rc = (T)tau_rc;
  a.tau_ref = (T)tau_ref;
  return a;
}

// ---------------------------------------------------------------------------------------------- row program
// one first-order low-pass step, y += a (x - y)
template <class T>
ABRK_ADAPT_INL T adapt_lowpass(T y, T x, T a) {
  return y + a * (x - y);
}

// step 1 for input column d of a row -> the new x_f[d]
template <class T>
ABRK_ADAPT_INL T adapt_input(const AdaptArgs<T>& a, long b, int d, T x_f) {
  const T raw = d < a.w0 ? a.in0[b * a.w0 + d] : a.in1[b * a.w1 + (d - a.w0)];
  return adapt_lowpass(x_f, (raw - a.shift[d]) * a.scale[d], a.a_in);
}

// enc_i . x_f of neuron i (xf: LDS on the device, the state array on the host); J = gain_i * it + bias_i
template <class T>
ABRK_ADAPT_INL T adapt_dot(const AdaptArgs<T>& a, int i, const T* xf) {
  const T* e = a.enc + (long)i * a.D;
  T dot = T(0);
  for (int d = 0; d < a.D; d++) dot += e[d] * xf[d];
  return dot;
}

// Nengo's LIF step for one neuron -> s (spikes / dt).  The library is built with -ffinite-math-only: J - 1 is only
// divided by where a spike's overshoot v - 1 lies below it (always, for a voltage that rose towards J from below the
// threshold), and a quotient that rounds to 1 - log1p(-1) - counts as no overshoot; the spike then falls on the step's end.
template <class T>
ABRK_ADAPT_INL T adapt_lif(const AdaptArgs<T>& a, T J, T& v, T& ref) {
  ref -= a.dt;
  T delta = a.dt - ref;
  delta = delta < T(0) ? T(0) : (delta > a.dt ? a.dt : delta);
  v -= (J - v) * expm1(-delta / a.tau_rc);
  if (v > T(1)) {
    const T over = v - T(1), den = J - T(1);
    const bool ok = den > over;
    T r = ok ? over / (ok ? den : T(1)) : T(0);
    if (!(r < T(1))) r = T(0);
    const T t_s = a.dt + a.tau_rc * log1p(-r);
    v = T(0);
    ref = a.tau_ref + t_s;
    return a.inv_dt;
  }
  v = v < T(0) ? T(0) : v;
  return T(0);
}

// Nengo's LIFRate: the steady-state rate of the same neuron under a constant J
template <class T>
ABRK_ADAPT_INL T adapt_lif_rate(const AdaptArgs<T>& a, T J) {
  const T jm = J - T(1);
  const bool on = jm > T(0);
  const T safe = on ? jm : T(1);
  return on ? T(1) / (a.tau_ref + a.tau_rc * log1p(T(1) / safe)) : T(0);
}

// steps 4 and 7 for one weight: -> its contribution to y_o; w is updated
template <class T>
ABRK_ADAPT_INL T adapt_weight(T& w, T s, T ke, T a_f) {
  const T y = w * s;
  w += ke * a_f;
  return y;
}

// steps 2 / 5 of output o once y_o is known are adapt_lowpass with a_tr / a_out

}  // namespace abrk
#endif  // ABRK_ADAPT_H

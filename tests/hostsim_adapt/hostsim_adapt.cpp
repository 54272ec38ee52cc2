// hostsim_adapt.cpp - TEST AID ONLY.  The row program of the adaptive signal (abr_control_amd/csrc/abrk_adapt.h: what
// the lanes of adapt_kernel execute per neuron, per input and per output) compiled for the HOST and run one neuron after
// the other, so that the tick is checked against tests/adapt_ref.py without a GPU.  Built on first use by
// tests/hostsim_adapt/__init__.py.
#define ABRK_ADAPT_HD __host__ __device__
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../abr_control_amd/csrc/abrk_adapt.h"

using namespace abrk;

// one tick of B rows in fp64; the arrays as abrk_adapt_step_batch takes them (host memory)
extern "C" int hostsim_adapt_step(int neuron_type, int D, int O, int N, int n_per, int w0, int w1, double dt,
                                  double tau_input, double tau_training, double tau_output, double tau_rc,
                                  double tau_ref, double pes_learning_rate, int64_t B, const double* enc,
                                  const double* gain, const double* bias, const double* shift, const double* scale,
                                  const double* in0, const double* in1, const double* training, double* x_f, double* e_f,
                                  double* v, double* ref, double* a_f, double* W, double* out_f, double* out,
                                  double* u_add) {
  AdaptArgs<double> a = adapt_make_args<double>(D, O, N, n_per, w0, w1, (long)B, dt, tau_input, tau_training, tau_output,
                                                tau_rc, tau_ref, pes_learning_rate);
  a.enc = enc;
  a.gain = gain;
  a.bias = bias;
  a.shift = shift;
  a.scale = scale;
  a.in0 = in0;
  a.in1 = in1;
  a.training = training;
  const bool lif = neuron_type == kAdaptLif;
  std::vector<double> ke(O), acc(O);
  for (long b = 0; b < B; b++) {
    double* xf = x_f + b * D;
    for (int d = 0; d < D; d++) xf[d] = adapt_input(a, b, d, xf[d]);
    for (int o = 0; o < O; o++) {
      e_f[b * O + o] = adapt_lowpass(e_f[b * O + o], training[b * O + o], a.a_tr);
      ke[o] = a.kappa * e_f[b * O + o];
      acc[o] = 0.0;
    }
    const long row = b * (long)N;
    for (int i = 0; i < N; i++) {
      const double J = gain[i] * adapt_dot(a, i, xf) + bias[i];
      const double s = lif ? adapt_lif(a, J, v[row + i], ref[row + i]) : adapt_lif_rate(a, J);
      a_f[row + i] = adapt_lowpass(a_f[row + i], s, a.a_pre);
      for (int o = 0; o < O; o++) acc[o] += adapt_weight(W[(row * O) + (long)o * N + i], s, ke[o], a_f[row + i]);
    }
    for (int o = 0; o < O; o++) {
      const double of = adapt_lowpass(out_f[b * O + o], acc[o], a.a_out);
      out_f[b * O + o] = of;
      out[b * O + o] = of;
      if (u_add) u_add[b * O + o] += of;
    }
  }
  return 0;
}

// abrk_channel.h - the measurement and actuation channel of a recorded loop: a [B, W] signal passed through noise, bias,
// quantisation, latency and (optionally) a filtered difference, one tick per launch.  The row program, the argument block
// of the kernels in abrk_channel.hip and their launchers.  Arm-independent: a translation unit of its own, not part of
// the plugin ABI tag.
//
// One tick of row b, column c (DESIGN.md "Measurement channel"); t = max(counter[b], 0), d = delay:
//   1  x = concat(in0[b], in1[b])[c];  v = fma(sigma[c], n, x + bias[c])      n: the standard normal below; sigma[c] == 0:
//                                                                             nothing is drawn, v = x + bias[c]
//   2  resolution[c] > 0:  v = rint(v * inv_res[c]) * resolution[c]           rint: half to even
//   3  d > 0:  ring[t % (d + 1), b, c] = v;  out = ring[max(t - d, 0) % (d + 1), b, c]      ring [d + 1, B, W], time-major
//      d == 0: out = v (the ring is not touched)
//   4  y = out -> out0[b, c] | out1[b, c - w0]
//   5  with dy:  t == 0: g = 0, d_f = 0;  else g = (out - prev[b,c]) * inv_dt, d_f = fma(a, g - d_f, d_f);
//      dy[b,c] = d_f, prev[b,c] = out
//   6  counter[b] = t + 1
// n is computed in fp64 whatever T is - Philox4x32-10 keyed by the seed, counter (row + row_offset (64 bit), t, c), two
// 53-bit uniforms, Box-Muller's cosine branch - and rounded to T at the fma: the fp32 kernels see the same realisation.
//
// The row program is plain C++ and compiles for the host as well (tests/hostsim_channel defines ABRK_CHANNEL_HD as
// __host__ __device__), so that the tick is checked against its NumPy statement without a GPU.
#ifndef ABRK_CHANNEL_H
#define ABRK_CHANNEL_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef ABRK_CHANNEL_HD
#define ABRK_CHANNEL_HD __device__
#endif
#define ABRK_CHANNEL_INL ABRK_CHANNEL_HD inline

namespace abrk {

constexpr int kChannelBlock = 256;     // lanes of a workgroup: one lane per element, whole rows only
constexpr int kChannelMaxW = 16;       // columns (ABRK_CHANNEL_MAX_WIDTH)
constexpr int kChannelMaxDelay = 4096;  // ticks (ABRK_CHANNEL_MAX_DELAY)

template <class T>
struct ChannelArgs {
  int W, w0, w1, delay;
  long B;
  uint32_t key0, key1;  // the seed's low and high word
  int64_t row_offset;
  T a_diff, inv_dt;     // a(tau_diff), 1 / dt
  T bias[kChannelMaxW], sigma[kChannelMaxW], res[kChannelMaxW], inv_res[kChannelMaxW];
  const T *in0, *in1;   // [B,w0], [B,w1] or null
  T *out0, *out1, *dy;  // [B,w0], [B,w1] or null, [B,W] or null
  int32_t* counter;     // [B]
  T *ring, *prev, *d_f;  // [delay + 1, B, W] (null with delay == 0), [B,W], [B,W] (null without dy)
};

// launches the tick of a.B rows on `stream`; a launch in which every sigma is zero runs the instantiation without the
// generator.  No allocation, no sync.
hipError_t launch_channel_step(const ChannelArgs<double>& a, hipStream_t stream);
hipError_t launch_channel_step(const ChannelArgs<float>& a, hipStream_t stream);

// a(tau) = 1 - exp(-dt / tau), a(0) = 1; evaluated in double (as adapt_lowpass_gain), then rounded to T
inline double channel_lowpass_gain(double dt, double tau) { return tau > 0.0 ? -expm1(-dt / tau) : 1.0; }

// the argument block without its arrays (host side: the C entry point, and the host build of the tests)
template <class T>
inline ChannelArgs<T> channel_make_args(int w0, int w1, int delay, long B, uint64_t seed, int64_t row_offset, double dt,
                                        double tau_diff, const double* bias, const double* sigma,
                                        const double* resolution) {
  ChannelArgs<T> a{};
  a.W = w0 + w1;
  a.w0 = w0;
  a.w1 = w1;
  a.delay = delay;
  a.B = B;
  a.key0 = (uint32_t)seed;
  a.key1 = (uint32_t)(seed >> 32);
  a.row_offset = row_offset;
  a.a_diff = (T)channel_lowpass_gain(dt, tau_diff);
  a.inv_dt = (T)(1.0 / dt);
  for (int c = 0; c < a.W && c < kChannelMaxW; c++) {
    a.bias[c] = (T)bias[c];
    a.sigma[c] = (T)sigma[c];
    a.res[c] = (T)resolution[c];
    a.inv_res[c] = resolution[c] > 0.0 ? (T)(1.0 / resolution[c]) : T(0);
  }
  return a;
}
template <class T>
inline bool channel_has_noise(const ChannelArgs<T>& a) {
  for (int c = 0; c < a.W; c++)
    if (a.sigma[c] != T(0)) return true;
  return false;
}

// ---------------------------------------------------------------------------------------------- row program
ABRK_CHANNEL_INL double channel_fma(double a, double b, double c) { return ::fma(a, b, c); }
ABRK_CHANNEL_INL float channel_fma(float a, float b, float c) { return ::fmaf(a, b, c); }
ABRK_CHANNEL_INL double channel_rint(double x) { return ::rint(x); }
ABRK_CHANNEL_INL float channel_rint(float x) { return ::rintf(x); }

// Philox4x32-10: counter c[4], key (k0, k1) -> c
ABRK_CHANNEL_INL void channel_philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the standard normal of (seed, global row r, tick t, column c), in fp64
ABRK_CHANNEL_INL double channel_normal(uint32_t k0, uint32_t k1, uint64_t r, uint32_t t, uint32_t c) {
  uint32_t w[4] = {(uint32_t)r, (uint32_t)(r >> 32), t, c};
  channel_philox(w, k0, k1);
  const double two26 = 67108864.0, two_m53 = 1.1102230246251565404e-16, two_pi = 6.283185307179586476925;
  const double u1 = ((double)(w[0] >> 5) * two26 + (double)(w[1] >> 6) + 1.0) * two_m53;  // (0, 1]
  const double u2 = ((double)(w[2] >> 5) * two26 + (double)(w[3] >> 6)) * two_m53;        // [0, 1)
  return sqrt(-2.0 * log(u1)) * cos(two_pi * u2);
}

// t of row b: read before any lane may write counter[b]
template <class T>
ABRK_CHANNEL_INL int channel_tick(const ChannelArgs<T>& a, long b) {
  const int t = a.counter[b];
  return t < 0 ? 0 : t;
}

// steps 1 and 2 for column c of row b at tick t: x -> v.  NOISE = false: no column has noise (no generator)
template <class T, bool NOISE>
ABRK_CHANNEL_INL T channel_sample(const ChannelArgs<T>& a, long b, int c, int t, T x) {
  T v = x + a.bias[c];
  if (NOISE) {
    const T sigma = a.sigma[c];
    if (sigma != T(0)) {
      const uint64_t r = (uint64_t)((int64_t)b + a.row_offset);
      v = channel_fma(sigma, (T)channel_normal(a.key0, a.key1, r, (uint32_t)t, (uint32_t)c), v);
    }
  }
  const T res = a.res[c];
  if (res > T(0)) v = channel_rint(v * a.inv_res[c]) * res;
  return v;
}

// steps 1 to 5 for column c of row b at tick t = channel_tick(a, b).  Everything the element reads - its input, the ring
// slot of tick t - d, prev and d_f - is loaded before anything is stored: the loads are independent of one another.
template <class T, bool NOISE>
ABRK_CHANNEL_INL void channel_element(const ChannelArgs<T>& a, long b, int c, int t) {
  const int slots = a.delay + 1;
  const int wslot = a.delay > 0 ? t % slots : 0, rslot = t > a.delay ? (t - a.delay) % slots : 0;
  const long e = b * a.W + c, slot_stride = a.B * (long)a.W;
  const bool held = rslot != wslot, diff = a.dy != nullptr && t > 0;  // (the same slot: the sample written now)
  const T x = c < a.w0 ? a.in0[b * a.w0 + c] : a.in1[b * a.w1 + (c - a.w0)];
  const T old = held ? a.ring[rslot * slot_stride + e] : T(0);
  const T prev = diff ? a.prev[e] : T(0);
  T df = diff ? a.d_f[e] : T(0);
  const T v = channel_sample<T, NOISE>(a, b, c, t, x);
  if (a.delay > 0) a.ring[wslot * slot_stride + e] = v;
  const T out = held ? old : v;
  if (c < a.w0) a.out0[b * a.w0 + c] = out;
  else a.out1[b * a.w1 + (c - a.w0)] = out;
  if (a.dy) {
    if (diff) {
#pragma clang fp contract(off)  // g is rounded before d_f is taken from it: the only fma of this step is the stated one
      const T g = (out - prev) * a.inv_dt;
      df = channel_fma(a.a_diff, g - df, df);
    }
    a.d_f[e] = df;
    a.dy[e] = df;
    a.prev[e] = out;
  }
}

// one tick of row b, column after column (the host build of the tests; the kernels give every element a lane)
template <class T, bool NOISE>
ABRK_CHANNEL_INL void channel_row(const ChannelArgs<T>& a, long b) {
  const int t = channel_tick(a, b);
  for (int c = 0; c < a.W; c++) channel_element<T, NOISE>(a, b, c, t);
  a.counter[b] = t + 1;
}

}  // namespace abrk
#endif  // ABRK_CHANNEL_H

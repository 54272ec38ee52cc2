// hostsim_channel.cpp - TEST AID ONLY.  The row program of the measurement channel (abr_control_amd/csrc/abrk_channel.h:
// what a lane of channel_kernel executes for its element) compiled for the HOST and run one row after the other, column
// after column, so that the tick is checked against tests/channel_ref.py without a GPU.  Built on first use by
// tests/hostsim_channel/__init__.py.
#define ABRK_CHANNEL_HD __host__ __device__
#include <cmath>
#include <cstdint>

#include "../../abr_control_amd/csrc/abrk_channel.h"

using namespace abrk;

// one tick of B rows in fp64; the arrays as abrk_channel_step_batch takes them (host memory)
extern "C" int hostsim_channel_step(int w0, int w1, int delay, int64_t B, uint64_t seed, int64_t row_offset, double dt,
                                    double tau_diff, const double* bias, const double* sigma, const double* resolution,
                                    const double* in0, const double* in1, double* out0, double* out1, double* dy,
                                    int32_t* counter, double* ring, double* prev, double* d_f) {
  ChannelArgs<double> a =
      channel_make_args<double>(w0, w1, delay, (long)B, seed, row_offset, dt, tau_diff, bias, sigma, resolution);
  a.in0 = in0;
  a.in1 = in1;
  a.out0 = out0;
  a.out1 = out1;
  a.dy = dy;
  a.counter = counter;
  a.ring = ring;
  a.prev = prev;
  a.d_f = d_f;
  const bool noise = channel_has_noise(a);
  for (long b = 0; b < B; b++) {
    if (noise) channel_row<double, true>(a, b);
    else channel_row<double, false>(a, b);
  }
  return 0;
}

// the generator alone: the four Philox words and the normal of (seed, row, tick, column)
extern "C" double hostsim_channel_normal(uint64_t seed, int64_t row, uint32_t tick, uint32_t col, uint32_t* words) {
  uint32_t w[4] = {(uint32_t)(uint64_t)row, (uint32_t)((uint64_t)row >> 32), tick, col};
  channel_philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
  for (int i = 0; i < 4; i++) words[i] = w[i];
  return channel_normal((uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)row, tick, col);
}

// Philox4x32-10 on a caller's counter and key
extern "C" void hostsim_channel_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  uint32_t w[4] = {counter[0], counter[1], counter[2], counter[3]};
  channel_philox(w, key[0], key[1]);
  for (int i = 0; i < 4; i++) out[i] = w[i];
}

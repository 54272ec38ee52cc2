// abrk_adapt.hip - kernels of the adaptive signal (row program: abrk_adapt.h).
//
//   adapt_kernel<T, LIF, V>  one workgroup of kAdaptBlock lanes per row, neurons across lanes: lane t of pass p owns the V
//                            consecutive neurons starting at (p kAdaptBlock + t) V, so every per-neuron array - v, ref,
//                            a_f, each row of W, gain, bias - is read and written by consecutive lanes on consecutive
//                            addresses, V elements (16 bytes) per lane.  V = 16 / sizeof(T) needs N % V == 0 and 16-byte
//                            aligned arrays (then every row of every array starts aligned); anything else runs V = 1.
//                            The first wavefront filters the row's input (x_f -> LDS), the second the training signal
//                            (kappa e_f -> LDS); after the barrier every lane reads them as broadcasts.  W[o,i] is read
//                            once, contributes W s to the lane's accumulator of output o, is updated and written back.
//                            The O sums: __shfl_down over the wavefront (32, 16, .. 1), one LDS slot per wavefront and
//                            output, then lane o < O adds the four slots in wavefront order.  No atomics: the order is
//                            fixed by (N, V) alone, never by B or the row's place in the batch.
//   LDS: (kAdaptMaxD + kAdaptMaxO + kAdaptWaves kAdaptMaxO) sizeof(T) = 1152 bytes in fp64, 576 in fp32.
//   The encoder table [N,D] is shared by all rows and comes from L2; with D sizeof(T) a multiple of 16 (and the table
//   aligned) a lane fetches its neuron's encoder in 16-byte pieces.
#include "abrk_adapt.h"

namespace abrk {
namespace {

template <class T, int V>
__device__ inline void ldv(const T* p, T (&r)[V]) {
  if constexpr (V == 1) {
    r[0] = *p;
  } else {
    typedef T vt __attribute__((ext_vector_type(V)));
    const vt x = *reinterpret_cast<const vt*>(p);
#pragma unroll
    for (int j = 0; j < V; j++) r[j] = x[j];
  }
}
template <class T, int V>
__device__ inline void stv(T* p, const T (&r)[V]) {
  if constexpr (V == 1) {
    *p = r[0];
  } else {
    typedef T vt __attribute__((ext_vector_type(V)));
    vt x;
#pragma unroll
    for (int j = 0; j < V; j++) x[j] = r[j];
    *reinterpret_cast<vt*>(p) = x;
  }
}

// adapt_dot with the encoder fetched 16 bytes at a time (the same products in the same order)
template <class T>
__device__ inline T dot_vec(const AdaptArgs<T>& a, int i, const T* xf) {
  constexpr int VT = 16 / (int)sizeof(T);
  const T* e = a.enc + (long)i * a.D;
  T dot = T(0);
  for (int d = 0; d < a.D; d += VT) {
    T r[VT];
    ldv<T, VT>(e + d, r);
#pragma unroll
    for (int k = 0; k < VT; k++) dot += r[k] * xf[d + k];
  }
  return dot;
}

}  // namespace

// (not in the unnamed namespace: tools/kernel_resources.py lists it by its name)
template <class T, bool LIF, int V>
__global__ void __launch_bounds__(kAdaptBlock) adapt_kernel(AdaptArgs<T> a, int enc_vec) {
  __shared__ T s_x[kAdaptMaxD];
  __shared__ T s_ke[kAdaptMaxO];
  __shared__ T s_red[kAdaptWaves * kAdaptMaxO];
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < a.D) {  // (kAdaptMaxD = 64: the first wavefront)
    const T xf = adapt_input(a, b, tid, a.x_f[b * a.D + tid]);
    a.x_f[b * a.D + tid] = xf;
    s_x[tid] = xf;
  } else if (tid >= 64 && tid < 64 + a.O) {
    const int o = tid - 64;
    const T ef = adapt_lowpass(a.e_f[b * a.O + o], a.training[b * a.O + o], a.a_tr);
    a.e_f[b * a.O + o] = ef;
    s_ke[o] = a.kappa * ef;
  }
  __syncthreads();

  T acc[kAdaptMaxO];
#pragma unroll
  for (int o = 0; o < kAdaptMaxO; o++) acc[o] = T(0);
  const long row = b * (long)a.N;
  T* Wb = a.W + row * a.O;
  for (int i0 = tid * V; i0 < a.N; i0 += kAdaptBlock * V) {
    T s[V], af[V], vv[V], rr[V], gain[V], bias[V];
    if (LIF) {
      ldv<T, V>(a.v + row + i0, vv);
      ldv<T, V>(a.ref + row + i0, rr);
    }
    ldv<T, V>(a.a_f + row + i0, af);
    ldv<T, V>(a.gain + i0, gain);
    ldv<T, V>(a.bias + i0, bias);
#pragma unroll
    for (int j = 0; j < V; j++) {
      const T J = gain[j] * (enc_vec ? dot_vec(a, i0 + j, s_x) : adapt_dot(a, i0 + j, s_x)) + bias[j];
      s[j] = LIF ? adapt_lif(a, J, vv[j], rr[j]) : adapt_lif_rate(a, J);
      af[j] = adapt_lowpass(af[j], s[j], a.a_pre);
    }
    if (LIF) {
      stv<T, V>(a.v + row + i0, vv);
      stv<T, V>(a.ref + row + i0, rr);
    }
    stv<T, V>(a.a_f + row + i0, af);
    // the weights, four outputs at a time: the four loads are issued together (an output past O repeats row O - 1 of W
    // and is dropped), then each is used, updated and stored
#pragma unroll
    for (int g = 0; g < kAdaptMaxO; g += 4) {
      if (g < a.O) {
        T w[4][V];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int o = g + k < a.O ? g + k : a.O - 1;
          ldv<T, V>(Wb + (long)o * a.N + i0, w[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (g + k < a.O) {
            const T ke = s_ke[g + k];
#pragma unroll
            for (int j = 0; j < V; j++) acc[g + k] += adapt_weight(w[k][j], s[j], ke, af[j]);
            stv<T, V>(Wb + (long)(g + k) * a.N + i0, w[k]);
          }
        }
      }
    }
  }

  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 0; o < kAdaptMaxO; o++) {
    if (o < a.O) {
      T val = acc[o];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) val += __shfl_down(val, off, 64);
      if (lane == 0) s_red[wave * kAdaptMaxO + o] = val;
    }
  }
  __syncthreads();
  if (tid < a.O) {
    T y = s_red[tid];
#pragma unroll
    for (int w = 1; w < kAdaptWaves; w++) y += s_red[w * kAdaptMaxO + tid];
    const T of = adapt_lowpass(a.out_f[b * a.O + tid], y, a.a_out);
    a.out_f[b * a.O + tid] = of;
    a.out[b * a.O + tid] = of;
    if (a.u_add) a.u_add[b * a.O + tid] += of;
  }
}

namespace {
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <class T>
hipError_t launch(int neuron_type, const AdaptArgs<T>& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  constexpr int VT = 16 / (int)sizeof(T);
  const bool lif = neuron_type == kAdaptLif;
  const bool vec = a.N % VT == 0 && aligned16(a.a_f) && aligned16(a.W) && aligned16(a.gain) && aligned16(a.bias) &&
                   (!lif || (aligned16(a.v) && aligned16(a.ref)));
  const int enc_vec = a.D % VT == 0 && aligned16(a.enc);
  const dim3 grid((unsigned)a.B), block(kAdaptBlock);
  if (lif) {
    if (vec) hipLaunchKernelGGL((adapt_kernel<T, true, VT>), grid, block, 0, stream, a, enc_vec);
    else hipLaunchKernelGGL((adapt_kernel<T, true, 1>), grid, block, 0, stream, a, enc_vec);
  } else {
    if (vec) hipLaunchKernelGGL((adapt_kernel<T, false, VT>), grid, block, 0, stream, a, enc_vec);
    else hipLaunchKernelGGL((adapt_kernel<T, false, 1>), grid, block, 0, stream, a, enc_vec);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_adapt_step(int neuron_type, const AdaptArgs<double>& a, hipStream_t stream) {
  return launch(neuron_type, a, stream);
}
hipError_t launch_adapt_step(int neuron_type, const AdaptArgs<float>& a, hipStream_t stream) {
  return launch(neuron_type, a, stream);
}

}  // namespace abrk

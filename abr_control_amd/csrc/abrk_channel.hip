// abrk_channel.hip - kernels of the measurement and actuation channel (row program: abrk_channel.h).
//
//   channel_kernel<T, NOISE>  one lane per element.  A workgroup of kChannelBlock lanes owns R = kChannelBlock / W whole
//                             rows: lane l works on column l % W of the workgroup's row l / W (the last kChannelBlock - R W
//                             lanes idle), so consecutive lanes touch consecutive addresses of every [B, W] array - the
//                             ring slots, prev, d_f, dy - and of in / out but for the seam between in0 and in1.  One lane
//                             per row with a loop over the columns, the mapping of the other row programs here, was
//                             measured first and lost by a factor of five at 1 M rows x 12 columns and of two inside a
//                             4096-row loop (profiles/sensing.md): a row is 12 independent elements, each with a normal
//                             of its own to compute, and 4096 rows are only 64 wavefronts.
//                             The W lanes of a row all read counter[b]; the lane of column 0 writes it.  No lane can read
//                             it after that write: a row never straddles workgroups, every read comes before the barrier
//                             and the write after it.
//                             NOISE = false is the launch in which every sigma is zero: no Philox, no log / cos.  The
//                             per-column tables (bias, sigma, resolution and its reciprocal) are kernel arguments.
//   No LDS, no scratch, no AGPRs.
#include "abrk_channel.h"

namespace abrk {

// (not in an unnamed namespace: tools/kernel_resources.py lists it by its name)
template <class T, bool NOISE>
__global__ void __launch_bounds__(kChannelBlock) channel_kernel(ChannelArgs<T> a, int rows_per_block) {
  const int l = threadIdx.x;
  const int rb = l / a.W, c = l - rb * a.W;
  const long b = (long)blockIdx.x * rows_per_block + rb;
  const bool active = rb < rows_per_block && b < a.B;
  const int t = active ? channel_tick(a, b) : 0;
  __syncthreads();  // counter[b] has been read by all lanes of its row
  if (!active) return;
  channel_element<T, NOISE>(a, b, c, t);
  if (c == 0) a.counter[b] = t + 1;
}

namespace {
template <class T>
hipError_t launch(const ChannelArgs<T>& a, hipStream_t stream) {
  if (a.B <= 0) return hipSuccess;
  const int rows_per_block = kChannelBlock / a.W;  // W <= kChannelMaxW: at least 16 rows
  const dim3 grid((unsigned)((a.B + rows_per_block - 1) / rows_per_block)), block(kChannelBlock);
  if (channel_has_noise(a)) hipLaunchKernelGGL((channel_kernel<T, true>), grid, block, 0, stream, a, rows_per_block);
  else hipLaunchKernelGGL((channel_kernel<T, false>), grid, block, 0, stream, a, rows_per_block);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_channel_step(const ChannelArgs<double>& a, hipStream_t stream) { return launch(a, stream); }
hipError_t launch_channel_step(const ChannelArgs<float>& a, hipStream_t stream) { return launch(a, stream); }

}  // namespace abrk

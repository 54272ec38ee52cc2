// abrk_finish.h - second pass of the six-row law on hand-over records: the three finish kernels (per chunk, grouped,
// dense; which one a batch takes: abrk_osc6_plan.h) and the two forms of the arithmetic they share.  Included by
// abrk_law.hip alone (and the fused-launch prototype under tools/microbench).
//
// The records (osc_law6's deferral branch wrote them; abrk_device.h rec_*, ScratchBase::record): those of a 64-row
// chunk are packed at the chunk's first slots, each carrying its row's index; the arithmetic: abrk_ctrl.h
// osc6_rec_solve.  Which rows deferred arrives as one 64-bit mask per 64-row chunk (the first pass's ballot).
//   * wave-cooperative form (osc6_finish_wave): one record per WAVEFRONT.  Every lane decomposes the record's 6 x 6
//     Mx_inv - redundantly, so nothing crosses lanes and every data-dependent branch of the QL iteration is uniform
//     (only the rotations that exist are executed: ~35 of the 68 slots the predicated per-lane form walks) - and applies
//     the transformations to ITS column of [J | u_task | J v]; lanes N and N + 1 then hand their column to the others
//     (v_readlane) and lane c < N finishes joint c.  A lone lane's eigen-decomposition was the critical path of every
//     small six-row step (4096 rows: 95 % of the 64 wavefronts have a truncating row, 21 us per step of which ~15 us are
//     ONE lane's 4800 dependent instructions); here the per-lane work is the scalar recurrence plus one vector, and a
//     4096-row step's ~190 such rows run on 190 of the 1024 SIMDs at once.
//   * lane form (osc6_finish_lane): one record per LANE, the same arithmetic with all N + 2 columns on the lane (arms
//     whose Mx_inv always truncates, large batches).
// Both are the same solver with contraction pinned off: a row's bits do not depend on which ran.
#pragma once
#include "abrk_kernels.h"

namespace abrk {

template <class T>
__device__ __forceinline__ T lane_bcast(T v, int src) {
  if constexpr (sizeof(T) == 8) {
    const long long x = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(x & 0xffffffffLL), src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(x >> 32), src);
    return __builtin_bit_cast(T, (long long)(((unsigned long long)hi << 32) | lo));
  } else {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
  }
}
// (keeps a value that was asked for ahead of a branch from being asked for behind it)
template <class T>
__device__ __forceinline__ void pin_loaded(T& v) {
  asm volatile("" : "+v"(v));
}

// wave-cooperative form: the wavefront finishes ONE record.  c = this lane's column (idle lanes shadow the last one); S,
// G, ridx, b1, b2 = what osc6_rec_load and the caller's own loads brought of it (ridx: the row's index, b1 / b2: the
// two joint-space sums of joint `lane`)
template <int N, class T>
__device__ __forceinline__ void osc6_finish_wave(const T* rec, int lane, int c, T (&S)[21], T (&G)[1][6], T ridx, T b1,
                                                 T b2, int nulls, long B, T* __restrict__ ug, T* __restrict__ tsg) {
  // (a record's row index is data: whatever a slot holds, nothing is stored outside [0, B))
  const bool row_ok = ridx >= T(0) && ridx < T(B);
  const long b = row_ok ? (long)ridx : 0;
  {
#pragma clang fp contract(off)  // the same bits as osc6_tail / osc6_finish_row
    T li[6], iq[6], y[6];
    osc6_rec_solve<N, T, 1, true>(rec, c, S, G, li, iq);
    ql_pinv_solve<6>(li, iq, G[0], y);  // this lane's column through the pseudo-inverse
    T a1 = T(-0.0), a2 = T(-0.0);
    sfor<6>([&](auto i) ABRK_LAMBDA {
      const T yu = lane_bcast(y[i()], N), yw = lane_bcast(y[i()], N + 1);
      a1 = Rm<T>::fma(G[0][i()], yu, a1);
      a2 = Rm<T>::fma(G[0][i()], yw, a2);
    });
    if (lane < N && row_ok) {
      const T ts = b1 - a1;
      ug[b * N + lane] = ts + b2 - (nulls ? a2 : T(0));
      if (tsg) tsg[b * N + lane] = ts;
    }
  }
}
// lane form: this lane finishes the record at `rec`
template <int N, class T>
__device__ __forceinline__ void osc6_finish_lane(const T* rec, int nulls, long B, T* __restrict__ ug, T* __restrict__ tsg) {
  const T rix = rec[21];
  if (rix >= T(0) && rix < T(B)) {  // (a record's row index is data: nothing is stored outside [0, B))
    T u[N], ts[N];
    osc6_finish_row<N, T>(rec, nulls != 0, u, ts);
    store_row<N>(ug, (long)rix, u);
    if (tsg) store_row<N>(tsg, (long)rix, ts);
  }
}

// ---- per-chunk form.  The grid is (chunks, slots): wavefront (j, s0) asks for chunk j's mask AND for the record in the
// chunk's slot s0 at once - one memory round trip; whether there is such a record it learns from the mask's popcount.
// (Round 4 began with a global compaction of all masks in every wavefront - a prefix sum, a second walk over the masks,
// a row list in LDS - and the dependent chain mask -> row -> record: ~1.5 us of an 8.9 us kernel.)  A chunk with at most
// coop_rounds x slots records: wavefront (j, s) takes records s, s + slots, ... in the wave-cooperative form; a chunk
// with more: wavefront (j, 0) takes them all, one per lane.
template <int N, class T>
__device__ __forceinline__ void osc6_finish_chunk(long j, int s0, int slots, const unsigned long long* __restrict__ masks,
                                                  const T* __restrict__ recs, int nulls, int coop_rounds, long B,
                                                  T* __restrict__ ug, T* __restrict__ tsg) {
  const int lane = (int)threadIdx.x;
  const int c = lane < N + 2 ? lane : N + 1;  // (idle lanes shadow the last column)
  const int jc = lane < N ? lane : 0;
  const T* rec = recs + (j * kBlock + s0) * rec_len(N);
  // mask and record together (the record's slot exists whatever it holds: the host sizes `recs` in whole chunks)
  // (the mask through the vector memory path, like the record's columns: as a scalar load the compiler queues it behind
  //  the wait for the record's scalar loads - two round trips again)
  long jv = j;
  pin_loaded(jv);
  unsigned long long mask = masks[jv];
  T S[21], G[1][6], ridx, b1, b2;
  auto load = [&]() ABRK_LAMBDA {
    osc6_rec_load<N, T, 1>(rec, c, S, G);
    ridx = rec[21];
    // the two joint-space sums are asked for with the rest of the record: one memory round trip, not two
    b1 = rec[rec_off_b1(N) + jc];
    b2 = rec[rec_off_b1(N) + N + jc];
  };
  load();
  sfor<21>([&](auto e) ABRK_LAMBDA { pin_loaded(S[e()]); });
  sfor<6>([&](auto r) ABRK_LAMBDA { pin_loaded(G[0][r()]); });
  pin_loaded(ridx);
  pin_loaded(b1);
  pin_loaded(b2);
  pin_loaded(mask);
  const int cnt = __builtin_amdgcn_readfirstlane(__popcll(mask));
  if (s0 >= cnt) return;  // nothing in this slot
  if (cnt <= coop_rounds * slots) {
    for (int s = s0;;) {
      osc6_finish_wave<N, T>(rec, lane, c, S, G, ridx, b1, b2, nulls, B, ug, tsg);
      s += slots;
      if (s >= cnt) break;
      rec = recs + (j * kBlock + s) * rec_len(N);
      load();
    }
  } else if (s0 == 0 && lane < cnt) {
    osc6_finish_lane<N, T>(recs + (j * kBlock + lane) * rec_len(N), nulls, B, ug, tsg);
  }
}
// Workgroups are single wavefronts: the wave-cooperative form is bound by ONE wavefront's instruction stream, and two
// of them on a SIMD halve each other's issue rate (measured with 512-thread workgroups: eight working wavefronts per
// CU, 14.4 us for 190 rows; the dispatcher spreads single-wavefront workgroups over the CUs).  blockIdx.x is the chunk:
// the wavefronts that have a record (slots 0, 1, 2 of most chunks) come first in dispatch order and spread over all XCDs.
template <int N, class T>
__global__ void __launch_bounds__(kBlock)
osc6_finish_kernel(const unsigned long long* __restrict__ masks, const T* __restrict__ recs, int nulls, int coop_rounds,
                   long B, T* __restrict__ ug, T* __restrict__ tsg) {
  osc6_finish_chunk<N, T>((long)blockIdx.x, (int)blockIdx.y, (int)gridDim.y, masks, recs, nulls, coop_rounds, B, ug, tsg);
}

// ---- grouped form (round 5): the batch sizes where the per-chunk grid (chunks x slots) puts two WORKING wavefronts on
// one SIMD.  At 16384 rows 256 chunks x 4 slots fill the 1024 SIMDs, and the wavefront of slot s >= 4 lands on the SIMD
// of slot s - 4 of the same chunk - busy whenever the chunk holds five records or more (17 % of the chunks of random UR5
// states): the kernel then lasts 12.0 us instead of 8.2 (profiles/round4/finish_per_chunk).  Here a GROUP of `gc`
// consecutive chunks shares 4 gc wavefronts: every wavefront reads the group's masks (one 8-byte value per lane, one
// coalesced request), numbers the group's records through - a pure function of the masks: no atomics, no counters - and
// wavefront i takes records i, i + 4 gc, ...: 46 +- 7 records on 64 wavefronts for gc = 16, so a second round is rare
// (0.6 % of the groups) where the per-chunk rule needed a fifth slot for every sixth chunk.  The price is the dependent
// chain mask -> record (one more memory round trip, ~0.8 us), which is why the smaller batches - every (chunk, slot)
// has a SIMD of its own there - keep the per-chunk form.
// A group with more records than `coop_max`: one record per lane, wavefront i < gc takes chunk i of the group.
template <int N, class T>
__global__ void __launch_bounds__(kBlock)
osc6_finish_group_kernel(const unsigned long long* __restrict__ masks, const T* __restrict__ recs, int nulls, int gc,
                         long nchunk, int coop_max, long B, T* __restrict__ ug, T* __restrict__ tsg) {
  const int lane = (int)threadIdx.x;
  const long c0 = (long)blockIdx.x * gc;
  const int wi = (int)blockIdx.y, wg = (int)gridDim.y;
  unsigned long long m = 0ull;
  if (lane < gc && c0 + lane < nchunk) m = masks[c0 + lane];
  const int cnt = __popcll(m);
  const int incl = wave_scan_incl(cnt, lane);
  const int total = __builtin_amdgcn_readlane(incl, kBlock - 1);
  if (total == 0) return;
  const int c = lane < N + 2 ? lane : N + 1;  // (idle lanes shadow the last column)
  const int jc = lane < N ? lane : 0;
  if (total <= coop_max) {
    // (a wavefront beyond the group's record count has nothing to do HERE; in the one-record-per-lane branch below
    //  wavefront wi owns CHUNK wi, whatever `total` is - coop_max == 0, i.e. ABRK_FINISH_ROUNDS=0, sends every group there)
    for (int r = wi; r < total; r += wg) {
      const unsigned long long above = __ballot(incl > r);  // the chunk that holds record r: the first lane whose count passes it
      const int ch = __builtin_ctzll(above);
      const int k = r - (__builtin_amdgcn_readlane(incl, ch) - __builtin_amdgcn_readlane(cnt, ch));
      const T* rec = recs + ((c0 + ch) * kBlock + k) * rec_len(N);
      T S[21], G[1][6];
      osc6_rec_load<N, T, 1>(rec, c, S, G);
      const T rix = rec[21];
      const T b1 = rec[rec_off_b1(N) + jc], b2 = rec[rec_off_b1(N) + N + jc];
      osc6_finish_wave<N, T>(rec, lane, c, S, G, rix, b1, b2, nulls, B, ug, tsg);
    }
  } else if (wi < gc && c0 + wi < nchunk) {
    const int mine = __builtin_amdgcn_readlane(cnt, wi);
    if (lane < mine) osc6_finish_lane<N, T>(recs + ((c0 + wi) * kBlock + lane) * rec_len(N), nulls, B, ug, tsg);
  }
}

// ---- dense form (round 6): batches beyond 65 536 rows, where the deferred rows are many enough to fill wavefronts ONE
// RECORD PER LANE.  Until round 5 such batches took the recompute form - a second pass of the complete row program over
// a worklist (kinematics, dynamics, Jacobian, the whole law again for 4.6 % of the rows: ~7000 instructions per row,
// 124 us of an 8 M-row step's 752).  Here a group of 64 consecutive chunks (4096 rows; 188 +- 13 records for random UR5
// states) is numbered through from its 64 masks - lane l holds chunk l's mask, one wave scan, no atomics - and wavefront
// w takes records 64 w .. 64 w + 63 of that numbering, each lane finding its record's chunk by a binary search over the
// scan (six __shfl) and finishing it from the record alone (the lane form, ~5200 instructions).  Lanes are 98 %
// occupied (the recompute pass packs 100 %, but runs the 1800-instruction kinematics on top).  Grid: groups x 4
// wavefronts, a wavefront loops while the group has more records (> 256 of 4096 rows deferring: dense fuzz arms,
// near-singular sets).
template <int N, class T>
__global__ void __launch_bounds__(kBlock)
osc6_finish_dense_kernel(const unsigned long long* __restrict__ masks, const T* __restrict__ recs, int nulls,
                         long nchunk, long B, T* __restrict__ ug, T* __restrict__ tsg) {
  const int lane = (int)threadIdx.x;
  const long c0 = (long)blockIdx.x * kBlock;
  unsigned long long m = 0ull;
  if (c0 + lane < nchunk) m = masks[c0 + lane];
  const int cnt = __popcll(m);
  // (wave_scan_incl written out: through the helper this kernel, and only this one, allocates other registers - 316 ->
  //  312 with 6 joints in fp64 - and the kernels' register counts are pinned build to build, tools/kernel_resources_diff.py)
  int incl = cnt;
  for (int d = 1; d < kBlock; d <<= 1) {
    const int v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
  }
  const int total = __builtin_amdgcn_readlane(incl, kBlock - 1);
  for (int w = (int)blockIdx.y; w * kBlock < total; w += (int)gridDim.y) {
    const int r = w * kBlock + lane;
    const int rr = r < total ? r : total - 1;  // (idle lanes of the last block shadow its last record: the shuffles stay uniform)
    int ch = 0;  // the chunk that holds record rr: the first lane whose inclusive count passes it
    for (int step = kBlock / 2; step >= 1; step >>= 1) {
      const int v = __shfl(incl, ch + step - 1);
      if (v <= rr) ch += step;
    }
    const int k = rr - (__shfl(incl, ch) - __shfl(cnt, ch));
    if (r < total) osc6_finish_lane<N, T>(recs + ((c0 + ch) * kBlock + k) * rec_len(N), nulls, B, ug, tsg);
  }
}

}  // namespace abrk

// abrk_osc6_plan.h - which form a six-row OSC call takes (every `ctrlr_dof` setting beyond x,y,z).
// Plain C++17, no HIP types: the host layer, the launchers, tests/hostsim and tools/microbench all read the decision
// from osc6_plan() below - the ONLY place where a batch size is compared with a band limit.
#pragma once

namespace abrk {

// OnePass: the complete row program, sweeps inline.  Recompute: first pass (osc_kernel mode 1) parks the rows whose
// pseudo-inverse truncates in a worklist, a dense second pass (mode 2) re-runs the row program on them.  Handover*:
// the first pass leaves a record per deferred row and one 64-bit mask per 64-row chunk; a finish kernel (abrk_finish.h)
// completes the rows from the records - per chunk, per group of chunks, or numbered through 64 chunks (dense).
enum class Osc6Form { OnePass, Recompute, HandoverChunk, HandoverGroup, HandoverDense };
constexpr bool osc6_uses_records(Osc6Form f) { return f >= Osc6Form::HandoverChunk; }  // `wl` holds masks, `rec` records
constexpr bool osc6_uses_worklist(Osc6Form f) { return f == Osc6Form::Recompute; }     // `wl` holds counters + row lists

constexpr int kOsc6ChunkRows = 64;            // one first-pass wavefront (abrk_kernels.h kBlock)
constexpr int kOsc6MaxGroup = 16;             // chunks per group at most: four wavefronts per chunk, one mask per lane
constexpr long kOsc6ChunkFinishMaxRows = 262144;  // the per-chunk / grouped finish kernels' grid: 4096 chunks x slots

// The measurement switches (ABRK_* variables, read by the host layer only under ABRK_MEASUREMENT=1) as
// data; the member initialisers are what ships.
struct Osc6Switches {
  bool no_defer = false;      // ABRK_NO_DEFER: always one pass (as before round 2)
  bool no_handover = false;   // ABRK_NO_HANDOVER: no records, recompute form from 16 384 rows (the round-3 scheme)
  long handover_max = 65536;  // ABRK_HANDOVER_MAX: largest batch of the per-chunk / grouped finish kernels (clamped to
                              // kOsc6ChunkFinishMaxRows)
  long dense_max = 1L << 20;  // ABRK_DENSE_MAX: largest batch of the dense finish kernel (0: recompute beyond handover_max)
  int finish_slots = 0;       // ABRK_FINISH_SLOTS: 1 .. 64 wavefronts per chunk; anything else = unset
  int finish_rounds = -1;     // ABRK_FINISH_ROUNDS: >= 0 records per wavefront at most (clamped to 64; 0: lane form only)
  int finish_group = -1;      // ABRK_FINISH_GROUP: 0 = never grouped, 1 .. 16 = always; anything else = unset
};

struct Osc6Plan {
  Osc6Form form = Osc6Form::OnePass;
  int slots = 0;   // HandoverChunk: wavefronts per 64-row chunk (the finish kernel's gridDim.y)
  int rounds = 0;  // HandoverChunk / HandoverGroup: records a wavefront takes at most in the wave-cooperative form; a
                   // chunk (group) with more than slots (4 x group) x rounds records goes one record per lane
  int group = 0;   // HandoverGroup: chunks that share 4 x group wavefronts
  constexpr bool uses_records() const { return osc6_uses_records(form); }
  constexpr bool uses_worklist() const { return osc6_uses_worklist(form); }
};

// Bands (shipped switches; chunks = ceil(B / 64)); random UR5 states with all six task rows: 4.6 % of the rows defer,
// 2.9 per chunk, more than 12 never.  Figures: same box, UR5, us per step.
//   B < 64                 OnePass        a single state truncates in 4.6 % of the calls: 0.7 us expected, against ~4 us
//                                         of a second launch + the finish kernel's scan
//   64 .. 65 536           HandoverChunk  slots x rounds = 12 x 2 up to 256 chunks (every (chunk, slot) has a SIMD of its
//                                         own up to 8192 rows), 8 x 1 up to 512 chunks, 2 x 1 beyond (working wavefronts
//                                         outnumber the SIMDs, a second round costs more than a second wavefront on the
//                                         SIMD).  Hand-over / recompute: 4096 rows 15.6 / 20.9, 16 k 19.4 / 32.6, 32 k
//                                         20.2 / 33.8, 64 k 27.6 / 37.0, 128 k 38.3 / 38.4 (profiles/round4/finish_per_chunk)
//   128 < chunks <= 256    HandoverGroup  16 chunks share 64 wavefronts: per chunk, 256 chunks x 4 slots fill the 1024
//                                         SIMDs and slot s >= 4 shares a SIMD with slot s - 4 (finish kernel 12.0 us
//                                         instead of 8.2).  16 384 rows 16.2 against 19.5, 12 288 rows 16.3 against 19.0,
//                                         32 768 rows 20.2 either way (profiles/round5/r5b/ab.txt)
//   65 537 .. 1 048 576    HandoverDense  one record per lane.  Recompute / dense: 131 072 rows 36.6 / 29.6, 262 144 rows
//                                         45.7 / 39.7, 524 288 rows 62.9 / 58.1, 1 M rows 96.0 / 94.0, 2 M rows 189.3 /
//                                         189.1, 8 M rows 708 / 758 - from HBM the records' traffic (2 x 253 MB) costs
//                                         more than the recomputation (profiles/round6/dense_finish_ab.txt)
//   beyond, to 2^31 - 1    Recompute      (without records it starts at 16 384 rows: below, the second launch costs more
//                                         than the divergence it removes, round 2)
//   2^31 and more          OnePass        row indices are parked as 32-bit ints (such batches fit the 288 GB for fp32 arms)
// A batch beyond handover_max that dense_max still admits goes to the dense kernel whatever its size (handover_max =
// 1000 sends 5000 rows there): the switches move the bands' edges, they do not add bands.
constexpr Osc6Plan osc6_plan(long B, const Osc6Switches& sw = Osc6Switches{}) {
  Osc6Plan p;
  if (sw.no_defer || B > 0x7fffffffL) return p;
  const long ho_max = sw.handover_max < kOsc6ChunkFinishMaxRows ? sw.handover_max : kOsc6ChunkFinishMaxRows;
  if (sw.no_handover || B < kOsc6ChunkRows || (B > ho_max && B > sw.dense_max)) {
    if (B >= 16384) p.form = Osc6Form::Recompute;
    return p;
  }
  if (B > ho_max) {
    p.form = Osc6Form::HandoverDense;
    return p;
  }
  const long nchunk = (B + kOsc6ChunkRows - 1) / kOsc6ChunkRows;
  p.slots = sw.finish_slots >= 1 && sw.finish_slots <= kOsc6ChunkRows ? sw.finish_slots
            : nchunk <= 256                                          ? 12
            : nchunk <= 512                                          ? 8
                                                                     : 2;
  p.rounds = sw.finish_rounds >= 0 ? (sw.finish_rounds > kOsc6ChunkRows ? kOsc6ChunkRows : sw.finish_rounds)
                                   : (nchunk <= 256 ? 2 : 1);
  p.group = sw.finish_group >= 0 && sw.finish_group <= kOsc6MaxGroup ? sw.finish_group
                                                                     : (nchunk > 128 && nchunk <= 256 ? kOsc6MaxGroup : 0);
  p.form = p.group > 0 ? Osc6Form::HandoverGroup : Osc6Form::HandoverChunk;
  return p;
}

}  // namespace abrk

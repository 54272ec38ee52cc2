// abrk_host.h - what the units of the host layer (abrk_host*.cpp) share; internal: not installed, not part of the
// plugin ABI tag.  No CPU fallback anywhere: without a HIP device every compute entry point fails with ABRK_ENODEV.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/abrk.h"
#include "abrk_kernels.h"

#pragma GCC visibility push(hidden)
namespace abrk {
namespace host {

// ------------------------------------------------------------------------------- errors
std::string& err_text();  // abrk_last_error() of this thread
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      (void)hipGetLastError();                                                             \
      return fail(e_ == hipErrorOutOfMemory ? ABRK_ENOMEM : ABRK_ENODEV, "%s: %s", #expr,  \
                  hipGetErrorString(e_));                                                  \
    }                                                                                      \
  } while (0)

// The sign and class of the double at `p`.  The library is built with -ffinite-math-only, under which the compiler
// folds std::isfinite, NaN compares and even an exponent test of a value it knows to be a double: the bits are read
// through an integer the optimiser is kept away from.
struct F64Bits {
  bool finite, negative, zero;
};
__attribute__((noinline, optnone)) inline F64Bits f64_bits_at(const void* p) {
  volatile uint64_t b;
  memcpy(const_cast<uint64_t*>(&b), p, sizeof(uint64_t));
  const uint64_t v = b;
  return {((v >> 52) & 0x7ff) != 0x7ff, (v >> 63) != 0, (v << 1) == 0};
}
inline bool finite_at(const void* p) { return f64_bits_at(p).finite; }
inline bool positive_finite_at(const void* p) {
  const F64Bits b = f64_bits_at(p);
  return b.finite && !b.negative && !b.zero;
}
inline bool nonnegative_finite_at(const void* p) {  // finite and >= 0 (a zero of either sign)
  const F64Bits b = f64_bits_at(p);
  return b.finite && (!b.negative || b.zero);
}

// ------------------------------------------------------------------------------- arm registry and the entry checks
struct ArmEntry {
  bool live = false;
  bool builtin = false;
  int gen = 0;  // user arms: bumped when the slot is freed - an id is slot | gen << kArmSlotBits, so a stale id (a copy of a
                // closed config, a handle cached past abrk_arm_destroy) never matches the slot's next tenant
  abrk_arm_desc desc;
  const ArmOps* ops = nullptr;
  std::vector<unsigned char> rt64, rt32;  // RtArm<N,double> / RtArm<N,float> images (user arms on the runtime-table
                                          // kernels; empty for built-in and compiled arms)
  std::shared_ptr<const abrk_arm_inertia> gi;  // full inertias of a general-inertia compiled arm; null: the plain form
};
// the live arm of this id or null; the pointer stays valid (entries are never moved after creation)
ArmEntry* get_arm(int id);
// the prologue of an entry: one wording per refusal
int check_batch(int dtype, int64_t B);  // ABRK_F64 / ABRK_F32, B >= 0
int check_joints(int n);                // 1..ABRK_MAX_JOINTS
int check_common(int arm_id, int dtype, int64_t B, ArmEntry** a);  // a live arm and check_batch
int check_helper(int dtype, int64_t B);  // check_batch for the entries that cannot be recorded into a plan

// ------------------------------------------------------------------------------- device and status words
int& current_device();  // what this thread last hipSetDevice'd (plan launches skip the call)
int use_device(int device);
struct StatusWord {
  volatile int* host = nullptr;
  int* dev = nullptr;
  bool take() {  // -> was it raised?  (cleared)
    if (!host || !*host) return false;
    *host = 0;
    return true;
  }
  // the second int of the slot: "a row has no path" of the path planner's plan pass (ABRK_EPATH), same life cycle
  volatile int* path_host() const { return host ? host + 1 : nullptr; }
  int* path_dev() const { return dev ? dev + 1 : nullptr; }
  bool take_path() {
    if (!host || !host[1]) return false;
    host[1] = 0;
    return true;
  }
};
// the word a call's kernels report to (nullptr: the allocation failed)
StatusWord* status_word(bool synchronous, int device, void* stream = nullptr);
void status_pool_stats(int64_t* words_out, int64_t* blocks);
int singular_error();
int path_error();

// ------------------------------------------------------------------------------- the array table of a law
// A family states its arrays once, as a function of what the call presents: elements per row, direction, and whether
// this call uses the array at all (one it does not use counts as absent whatever the caller passed).  The *_batch
// entry binds them, the *_sharded entry cuts and stages them, the *_resident entry names them from that statement.
struct ArraySpec {
  const char* name;
  size_t per_row;  // elements
  bool in, out, used;
};
enum { kRead = 1, kWritten = 2 };
constexpr int kMaxArrays = 16;
struct ArrayTable {
  int n = 0;
  ArraySpec a[kMaxArrays];
  void add(const char* name, size_t per_row, int mode, bool used = true) {
    a[n++] = {name, per_row, (mode & kRead) != 0, (mode & kWritten) != 0, used};
  }
};
// the outputs of `dynamics` (abrk_dyn_out, in its order); OSC's fused outputs are the first six
void add_dyn_outputs(ArrayTable& t, int n, uint32_t want, int count);

// The families with sharded and resident forms: their arrays and the one call all three forms go through (arr: the
// arrays in the table's order).  word: the ABRK_ESINGULAR word a sharded call hands its shards; null: the call's own
ArrayTable osc_arrays(int n, bool ki, uint32_t want);
int osc_call(int arm_id, int dtype, const abrk_osc_params* P, int64_t B, void* const* arr, uint32_t want, int device,
             void* stream, StatusWord* word);
ArrayTable sliding_arrays(int n, bool cartesian);
int sliding_call(int arm_id, int dtype, const abrk_sliding_params* P, int64_t B, void* const* arr, int device,
                 void* stream);
ArrayTable joint_arrays(int n);
int joint_call(int arm_id, int dtype, const abrk_null_ctrl* ctrl, int account_for_gravity, int64_t B, void* const* arr,
               int device, void* stream);
ArrayTable dynamics_arrays(int n, uint32_t want);
int dynamics_call(int arm_id, int dtype, int64_t B, void* const* arr, int frame, const double* x_off, uint32_t want,
                  int device, void* stream);

// ------------------------------------------------------------------------------- staging
void* device_view(const void* p);  // device-usable address of p, or nullptr for pageable host memory
// One call per array: bind() fills the kernel argument `field` with the device address of `host` - null stays null, a
// device-visible pointer is written at once, a pageable host array gets its staging copy's address from reserve().
struct Stager {
  int device;
  hipStream_t stream;
  struct Item {
    void* host;
    void* dev;
    size_t bytes;
    bool out, in;
    void** field;
  };
  std::vector<Item> items;
  size_t need = 0;
  bool staged = false, pinned = false;

  template <class P>
  void bind(P* field, const void* host, size_t bytes, bool in, bool out) {
    static_assert(std::is_same<P, void*>::value || std::is_same<P, const void*>::value, "a pointer argument");
    *field = nullptr;
    if (!host) return;
    if (void* d = device_view(host)) {
      *field = d;
      return;
    }
    items.push_back({const_cast<void*>(host), nullptr, bytes, out, in, const_cast<void**>(field)});
    need += (bytes + 255) & ~size_t(255);
  }
  void in(const void** field, const void* host, size_t bytes) { bind(field, host, bytes, true, false); }
  void out(void** field, void* host, size_t bytes) { bind(field, host, bytes, false, true); }
  void inout(void** field, void* host, size_t bytes) { bind(field, host, bytes, true, true); }
  // the arrays of a table, B rows of `elem` bytes per element, to the kernel arguments listed in the table's order
  void bind_table(const ArrayTable& t, void* const* arr, void** const* fields, int64_t B, size_t elem) {
    for (int k = 0; k < t.n; k++)
      bind(fields[k], t.a[k].used ? arr[k] : nullptr, (size_t)B * t.a[k].per_row * elem, t.a[k].in, t.a[k].out);
  }
  int reserve();
  int finish();
};

inline size_t esz(int dtype) { return dtype == ABRK_F64 ? 8 : 4; }

// ---- launch recording (abrk_plan_begin .. abrk_plan_end).  While a thread records, every abrk_*_batch call on it
// is validated and converted as usual but its kernel launch is kept as a closure instead of being enqueued; the
// closures own their parameter blocks and (for user arms) a private copy of the arm table.
struct Recorder {
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<std::function<hipError_t()>> steps;
  std::vector<std::unique_ptr<std::vector<unsigned char>>> tables;  // stable addresses
  std::vector<void*> dev_bufs;  // device scratch owned by the plan (worklists of the six-row OSC kernels)
};
Recorder*& recorder();  // this thread's, null outside abrk_plan_begin .. abrk_plan_end
inline bool recording() { return recorder() != nullptr; }  // is this thread inside abrk_plan_begin .. abrk_plan_end?

inline const void* arm_table(const ArmEntry* a, int dtype) {
  if (!a || a->rt64.empty()) return nullptr;  // built-in and compiled arms carry their table in the kernels
  return dtype == ABRK_F64 ? (const void*)a->rt64.data() : (const void*)a->rt32.data();
}

// A caller's grip on its (device, stream) scratch slot of the six-row kernels (worklist cache, abrk_host_osc.cpp): the
// slot's mutex AND a reference to the slot - a slot evicted or forgotten between the look-up and the lock stays alive
// (and simply leaves the cache) until the last holder lets go.
struct WorklistSlot;
struct WlHold {
  std::shared_ptr<WorklistSlot> slot;
  std::unique_lock<std::mutex> lk;
  void release() {
    if (lk.owns_lock()) lk.unlock();
    slot.reset();
  }
};
void wl_forget_stream(int device, hipStream_t stream);  // abrk_stream_destroy: the stream's slot leaves the cache

// enqueue now (and finish the staging), or keep the launch for the plan being recorded.  fn(arm_rt) launches the
// kernel; it captures its arguments by value.
template <class F>
int dispatch(Stager& st, const ArmEntry* a, int dtype, F&& fn, WlHold* held = nullptr) {
  if (Recorder* r = recorder()) {
    if (st.staged) return fail(ABRK_EINVAL, "plans take device pointers only (got a host pointer)");
    if (st.device != r->device || st.stream != r->stream)
      return fail(ABRK_EINVAL, "a recorded call must use the device and stream given to abrk_plan_begin");
    const void* rt = nullptr;
    if (a && !a->rt64.empty()) {
      r->tables.emplace_back(new std::vector<unsigned char>(dtype == ABRK_F64 ? a->rt64 : a->rt32));
      rt = r->tables.back()->data();
    }
    r->steps.emplace_back([fn, rt]() { return fn(rt); });
    return 0;
  }
  const hipError_t le = fn(arm_table(a, dtype));
  if (held) held->release();  // everything that uses the shared scratch is enqueued
  HIPCHK(le);
  return st.finish();
}

// a kernel's parameter block in both arithmetic types, make(T()) building the T one; of(dtype) is the one a launch reads
template <class B64, class B32>
struct Blocks {
  B64 f64;
  B32 f32;
  const void* of(int dtype) const { return dtype == ABRK_F64 ? (const void*)&f64 : (const void*)&f32; }
};
template <class Make>
auto blocks(Make make) -> Blocks<decltype(make(0.0)), decltype(make(0.0f))> {
  return {make(0.0), make(0.0f)};
}

// The tail of an arm entry: dispatch the launch of `op` (a member of ArmOps) on the bound arguments, their .P set to
// the parameter block of the call's dtype (NoBlocks: the kernel takes none).
struct NoBlocks {};
template <class Args, class PB = NoBlocks>
int launch_arm(Stager& st, const ArmEntry* a, int dtype, int64_t B,
               hipError_t (*ArmOps::*op)(int, const LaunchArgs&, const Args&), const Args& args, const PB& pb = PB()) {
  const ArmOps* ops = a->ops;
  const hipStream_t hs = st.stream;
  return dispatch(st, a, dtype, [=](const void* rt) {
    Args o = args;
    if constexpr (!std::is_same<PB, NoBlocks>::value) o.P = pb.of(dtype);
    return (ops->*op)(dtype, LaunchArgs{rt, (long)B, hs}, o);
  });
}

// The ABRK_ESINGULAR word of an OSC-law call, stored in both parameter blocks before run() dispatches the call.  Host
// arrays (st.staged): the calling thread's word, cleared first, and the call returns the code once its outputs are back.
// Device pointers: the word of their (device, stream), reported by whatever drains that stream next.  `given` (the
// shards of abrk_osc_generate_sharded): the caller's word, which the caller clears and takes itself.
template <class OscBlocks, class Run>
int with_status_word(const Stager& st, OscBlocks& pb, StatusWord* given, Run&& run) {
  StatusWord* sw = given ? given : status_word(st.staged, st.device, st.stream);
  const bool own = st.staged && !given;
  pb.f64.status = pb.f32.status = sw ? sw->dev : nullptr;
  if (sw && own) *sw->host = 0;  // (this thread's word: nothing of an earlier, failed call is left in it)
  const int rc = run();
  return rc == 0 && own && sw && sw->take() ? singular_error() : rc;
}

}  // namespace host
}  // namespace abrk
#pragma GCC visibility pop
using namespace abrk;  // (an internal header: only the host units include it)
using namespace abrk::host;

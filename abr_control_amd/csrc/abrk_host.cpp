// abrk_host.cpp - the runtime of the C ABI of libabrk.so (include/abrk.h): errors, arm registry and plugins, device /
// stream / event / memory wrappers, status words, the staging arenas behind Stager and the recorded plans.
#include <dlfcn.h>

#include <cstdarg>
#include <cstdio>
#include <map>

#include "abrk_host.h"
#include "abrk_plugin.h"

namespace abrk {
const ArmOps* ops_ur5();
const ArmOps* ops_jaco2();
const ArmOps* ops_twojoint();
const ArmOps* ops_threejoint();
const ArmOps* ops_onejoint();
const ArmOps* ops_rt(int n_joints);
size_t rt_table_size(int n_joints, int dtype);
void rt_table_fill(int n_joints, int dtype, const abrk_arm_desc* d, void* dst);
}  // namespace abrk

// ------------------------------------------------------------------------------- errors
// (thread-local state is defined here and nowhere else; the other units reach it through these accessors)
static thread_local std::string g_err;
std::string& host::err_text() { return g_err; }
int host::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

extern "C" const char* abrk_last_error(void) { return g_err.c_str(); }
extern "C" int abrk_version(void) { return ABRK_VERSION; }

// ------------------------------------------------------------------------------- arm registry
namespace {
// plugins stay loaded for the life of the process (their code objects are registered with the HIP runtime)
struct PluginLib {
  std::string path;
  const ArmOps* ops;
  abrk_arm_desc desc;
  std::shared_ptr<const abrk_arm_inertia> inertia;
};
std::vector<PluginLib> g_plugins;
std::mutex g_mu;
std::vector<ArmEntry> g_arms;
constexpr int kArmSlotBits = 12, kArmSlots = 1 << kArmSlotBits, kArmGenMask = (1 << (31 - kArmSlotBits)) - 1;
int arm_id_of(int slot) { return slot | (g_arms[slot].gen << kArmSlotBits); }
// slot of a live arm id, or -1 (caller holds g_mu)
int arm_slot(int id) {
  if (id < 0) return -1;
  const int slot = id & (kArmSlots - 1);
  if (slot >= (int)g_arms.size() || !g_arms[slot].live || g_arms[slot].gen != (id >> kArmSlotBits)) return -1;
  return slot;
}

void init_builtins() {
  if (!g_arms.empty()) return;
  g_arms.reserve(kArmSlots);  // entries are handed out by address: never reallocate
  g_arms.resize(5);
  desc_from_tab<Tab_ur5>(&g_arms[0].desc);
  g_arms[0].ops = ops_ur5();
  desc_from_tab<Tab_jaco2>(&g_arms[1].desc);
  g_arms[1].ops = ops_jaco2();
  desc_from_tab<Tab_twojoint>(&g_arms[2].desc);
  g_arms[2].ops = ops_twojoint();
  desc_from_tab<Tab_threejoint>(&g_arms[3].desc);
  g_arms[3].ops = ops_threejoint();
  desc_from_tab<Tab_onejoint>(&g_arms[4].desc);
  g_arms[4].ops = ops_onejoint();
  for (auto& a : g_arms) a.live = a.builtin = true;
}

// a new user arm -> its id (caller holds g_mu).  A destroyed user arm's slot is taken again (ids are handles, like file
// descriptors): a long-running process may register and drop any number of arms, 4096 at a time
int install_arm(ArmEntry&& e, const abrk_arm_desc& d) {
  int slot = -1;
  for (int i = 5; i < (int)g_arms.size() && slot < 0; i++)
    if (!g_arms[i].live) slot = i;
  if (slot < 0 && g_arms.size() >= (size_t)kArmSlots) return fail(ABRK_ENOMEM, "too many arms (%d live at once)", kArmSlots);
  e.live = true;
  e.desc = d;
  e.desc.name[sizeof e.desc.name - 1] = 0;
  if (slot < 0) {
    g_arms.emplace_back();
    slot = (int)g_arms.size() - 1;
  }
  e.gen = g_arms[slot].gen;
  g_arms[slot] = std::move(e);
  return arm_id_of(slot);
}
}  // namespace

// returns a COPY-safe pointer valid while the registry lock is not needed (entries are
// never moved after creation: vector of stable size is avoided by reserving)
ArmEntry* host::get_arm(int id) {
  std::lock_guard<std::mutex> lk(g_mu);
  init_builtins();
  const int slot = arm_slot(id);
  return slot < 0 ? nullptr : &g_arms[slot];
}

int host::check_batch(int dtype, int64_t B) {
  if (dtype != ABRK_F64 && dtype != ABRK_F32) return fail(ABRK_EINVAL, "dtype %d is not ABRK_F64/ABRK_F32", dtype);
  if (B < 0) return fail(ABRK_EINVAL, "negative batch %lld", (long long)B);
  return 0;
}
int host::check_joints(int n) {
  if (n < 1 || n > ABRK_MAX_JOINTS) return fail(ABRK_EINVAL, "n_joints=%d outside 1..%d", n, ABRK_MAX_JOINTS);
  return 0;
}
int host::check_common(int arm_id, int dtype, int64_t B, ArmEntry** a) {
  *a = get_arm(arm_id);
  if (!*a) return fail(ABRK_ENOARM, "unknown arm id %d", arm_id);
  return check_batch(dtype, B);
}
int host::check_helper(int dtype, int64_t B) {
  if (recording()) return fail(ABRK_EINVAL, "the OSC helper / transformations entry points cannot be recorded into a plan");
  return check_batch(dtype, B);
}

extern "C" int abrk_arm_builtin(const char* name) {
  std::lock_guard<std::mutex> lk(g_mu);
  init_builtins();
  if (!name) return fail(ABRK_EINVAL, "abrk_arm_builtin: NULL name");
  for (int i = 0; i < 5; i++)
    if (!strcmp(name, g_arms[i].desc.name)) return i;
  return fail(ABRK_ENOARM, "unknown built-in arm '%s'", name);
}

extern "C" int abrk_arm_create(const abrk_arm_desc* d) {
  if (!d) return fail(ABRK_EINVAL, "abrk_arm_create: NULL desc");
  if (int rc = check_joints(d->n_joints)) return rc;
  if (d->n_links_dyn < 0 || d->n_links_dyn > d->n_joints + 1)
    return fail(ABRK_EINVAL, "n_links_dyn=%d outside 0..n_joints+1", d->n_links_dyn);
  std::lock_guard<std::mutex> lk(g_mu);
  init_builtins();
  ArmEntry e;
  e.ops = ops_rt(d->n_joints);
  e.rt64.resize(rt_table_size(d->n_joints, ABRK_F64));
  e.rt32.resize(rt_table_size(d->n_joints, ABRK_F32));
  rt_table_fill(d->n_joints, ABRK_F64, d, e.rt64.data());
  rt_table_fill(d->n_joints, ABRK_F32, d, e.rt32.data());
  return install_arm(std::move(e), *d);
}

namespace {
bool same_table(const abrk_arm_desc& a, const abrk_arm_desc& b) {
  if (a.n_joints != b.n_joints || a.n_links_dyn != b.n_links_dyn || (a.has_ee != 0) != (b.has_ee != 0)) return false;
  const int n = a.n_joints;
  if (memcmp(a.A0, b.A0, sizeof a.A0)) return false;
  for (int i = 0; i < n; i++)
    if (memcmp(a.AJ[i], b.AJ[i], sizeof a.AJ[i]) || memcmp(a.B[i], b.B[i], sizeof a.B[i])) return false;
  if (a.has_ee && memcmp(a.E, b.E, sizeof a.E)) return false;
  for (int l = 0; l <= n; l++)
    if (memcmp(a.mdiag[l], b.mdiag[l], sizeof a.mdiag[l])) return false;
  return true;
}
// the inertias of links 0..n and joints 0..n-1 agree value by value
bool same_inertia(const abrk_arm_inertia& a, const abrk_arm_inertia& b, int n) {
  for (int l = 0; l <= n; l++)
    if (memcmp(a.mlink[l], b.mlink[l], sizeof a.mlink[l])) return false;
  for (int j = 0; j < n; j++)
    if (memcmp(a.mjoint[j], b.mjoint[j], sizeof a.mjoint[j])) return false;
  return true;
}
}  // namespace

extern "C" const char* abrk_plugin_abi(void) { return ABRK_PLUGIN_ABI; }

extern "C" int abrk_arm_create_compiled(const abrk_arm_desc* d, const char* plugin_path) {
  return abrk_arm_create_compiled_inertia(d, nullptr, plugin_path);
}

extern "C" int abrk_arm_create_compiled_inertia(const abrk_arm_desc* d, const abrk_arm_inertia* inertia,
                                                const char* plugin_path) {
  if (!d || !plugin_path) return fail(ABRK_EINVAL, "abrk_arm_create_compiled: NULL argument");
  if (int rc = check_joints(d->n_joints)) return rc;
  if (d->n_links_dyn < 0 || d->n_links_dyn > d->n_joints + 1)
    return fail(ABRK_EINVAL, "n_links_dyn=%d outside 0..n_joints+1", d->n_links_dyn);
  std::lock_guard<std::mutex> lk(g_mu);
  init_builtins();
  const PluginLib* pl = nullptr;
  for (const auto& p : g_plugins)
    if (p.path == plugin_path) pl = &p;
  if (!pl) {
    void* h = dlopen(plugin_path, RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(ABRK_EINVAL, "cannot load arm plugin: %s", dlerror());
    auto f_abi = reinterpret_cast<abrk_plugin_abi_fn>(dlsym(h, "abrk_plugin_abi_tag"));
    auto f_ops = reinterpret_cast<abrk_plugin_ops_fn>(dlsym(h, "abrk_plugin_ops"));
    auto f_desc = reinterpret_cast<abrk_plugin_desc_fn>(dlsym(h, "abrk_plugin_desc"));
    auto f_inertia = reinterpret_cast<abrk_plugin_inertia_fn>(dlsym(h, "abrk_plugin_inertia"));
    if (!f_abi || !f_ops || !f_desc) {
      dlclose(h);
      return fail(ABRK_EINVAL, "%s is not an arm plugin (entry points missing)", plugin_path);
    }
    if (strcmp(f_abi(), ABRK_PLUGIN_ABI) != 0) {
      int rc = fail(ABRK_EINVAL, "arm plugin %s was built for kernel headers %s, this library is %s: rebuild it",
                    plugin_path, f_abi(), ABRK_PLUGIN_ABI);
      dlclose(h);
      return rc;
    }
    if (!f_inertia) {  // (same headers, so never for a plugin that make built)
      dlclose(h);
      return fail(ABRK_EINVAL, "%s is not an arm plugin (entry points missing)", plugin_path);
    }
    PluginLib p;
    p.path = plugin_path;
    p.ops = static_cast<const ArmOps*>(f_ops());
    f_desc(&p.desc);
    auto in = std::make_shared<abrk_arm_inertia>();
    f_inertia(in.get());
    p.inertia = in;
    g_plugins.push_back(std::move(p));
    pl = &g_plugins.back();
  }
  if (!same_table(pl->desc, *d))
    return fail(ABRK_EINVAL, "arm plugin %s was compiled for a different arm table than the one given", plugin_path);
  abrk_arm_inertia plain;
  inertia_plain(*d, &plain);
  const bool gi = !same_inertia(*pl->inertia, plain, d->n_joints);
  if (!same_inertia(*pl->inertia, inertia ? *inertia : plain, d->n_joints))
    return fail(ABRK_EINVAL, "arm plugin %s was compiled for %s inertias than the ones given", plugin_path,
                gi ? "other (general)" : "other (plain)");
  ArmEntry e;
  e.ops = pl->ops;
  if (gi) e.gi = pl->inertia;
  return install_arm(std::move(e), *d);
}

extern "C" int abrk_arm_get_desc(int arm_id, abrk_arm_desc* out) {
  ArmEntry* a = get_arm(arm_id);
  if (!a || !out) return fail(ABRK_ENOARM, "unknown arm id %d", arm_id);
  *out = a->desc;
  return 0;
}

extern "C" int abrk_arm_get_inertia(int arm_id, abrk_arm_inertia* out) {
  ArmEntry* a = get_arm(arm_id);
  if (!a || !out) return fail(ABRK_ENOARM, "unknown arm id %d", arm_id);
  if (a->gi) *out = *a->gi;
  else inertia_plain(a->desc, out);
  return 0;
}

extern "C" int abrk_arm_destroy(int arm_id) {
  std::lock_guard<std::mutex> lk(g_mu);
  init_builtins();
  const int slot = arm_slot(arm_id);
  if (slot < 5) return fail(ABRK_ENOARM, "arm id %d is not a (live) user arm", arm_id);
  g_arms[slot].live = false;
  g_arms[slot].gen = (g_arms[slot].gen + 1) & kArmGenMask;
  g_arms[slot].rt64 = {};
  g_arms[slot].rt32 = {};
  g_arms[slot].gi = nullptr;
  return 0;
}

// ------------------------------------------------------------------------------- device plumbing
static thread_local int t_current_device = -1;
int& host::current_device() { return t_current_device; }
int host::use_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return fail(ABRK_ENODEV, "no HIP device available (%s); libabrk has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  }
  if (device < 0 || device >= n) return fail(ABRK_EINVAL, "device %d outside 0..%d", device, n - 1);
  HIPCHK(hipSetDevice(device));
  t_current_device = device;
  return 0;
}

// ---- the "M is not positive definite" flag (ABRK_ESINGULAR; the reference raises LinAlgError at osc.py:136).  The OSC
// kernels store 1 through OscP::status where a row's Cholesky factor of M meets a non-positive pivot.  A word lives in
// pinned, device-mapped host memory, so reading it costs the host nothing once the stream is drained:
//   * a call that hands over HOST arrays is synchronous - it uses the calling thread's own word and returns the code;
//   * a call on DEVICE pointers is asynchronous - it uses the word of its (device, stream), which is reported ONCE by
//     whatever drains that stream next: abrk_stream_sync, abrk_memcpy_d2h on it, abrk_device_sync (every stream of the
//     device).  Several control loops on one GPU each hear of their own singular batch and of nobody else's.
// Words come from a pool (64 of them per pinned 4 KiB block; blocks live as long as the process, words are recycled): a
// thread's word goes back when the thread exits, a stream's word when abrk_stream_destroy is called.
enum { kStatusSingular = 1, kStatusPath = 2 };
namespace {
struct StatusPool {
  std::mutex mu;
  std::vector<StatusWord> free_;
  int64_t blocks = 0, handed_out = 0;
  static constexpr size_t kStride = 64, kBlock = 4096;
  StatusWord get() {  // {nullptr, nullptr}: no pinned memory to be had - nobody listens, as before round 5
    std::lock_guard<std::mutex> lk(mu);
    if (free_.empty()) {
      void *h = nullptr, *d = nullptr;
      if (hipHostMalloc(&h, kBlock, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess ||
          hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (h) (void)hipHostFree(h);
        return {};
      }
      memset(h, 0, kBlock);
      blocks++;
      for (size_t o = 0; o < kBlock; o += kStride)
        free_.push_back(StatusWord{(volatile int*)((char*)h + o), (int*)((char*)d + o)});
    }
    StatusWord w = free_.back();
    free_.pop_back();
    w.host[0] = w.host[1] = 0;
    handed_out++;
    return w;
  }
  void put(StatusWord w) {
    if (!w.host) return;
    std::lock_guard<std::mutex> lk(mu);
    free_.push_back(w);
    handed_out--;
  }
};
// (never destroyed: thread_local destructors of late-exiting threads may still hand words back during process exit)
StatusPool& status_pool() {
  static StatusPool* p = new StatusPool;
  return *p;
}
struct ThreadStatus {
  StatusWord w;
  ~ThreadStatus() { status_pool().put(w); }
};
thread_local ThreadStatus t_status;
std::mutex g_status_mu;
std::map<std::pair<int, void*>, StatusWord> g_stream_status;  // (device, stream) -> the word of its asynchronous calls
}  // namespace
StatusWord* host::status_word(bool synchronous, int device, void* stream) {
  if (synchronous) {
    if (!t_status.w.host) t_status.w = status_pool().get();
    return t_status.w.host ? &t_status.w : nullptr;
  }
  std::lock_guard<std::mutex> lk(g_status_mu);
  StatusWord& w = g_stream_status[{device, stream}];  // (node addresses of a std::map are stable)
  if (!w.host) w = status_pool().get();
  return w.host ? &w : nullptr;
}
// which flags of (device, stream) were raised since they were last reported (kStatus* bits)?  all_streams: any stream
// of the device
static int status_take(int device, void* stream, bool all_streams) {
  std::lock_guard<std::mutex> lk(g_status_mu);
  int raised = 0;
  auto take = [&](StatusWord& w) {
    if (w.take()) raised |= kStatusSingular;
    if (w.take_path()) raised |= kStatusPath;
  };
  if (all_streams) {
    for (auto it = g_stream_status.lower_bound({device, nullptr}); it != g_stream_status.end() && it->first.first == device; ++it)
      take(it->second);
  } else {
    auto it = g_stream_status.find({device, stream});
    if (it != g_stream_status.end()) take(it->second);
  }
  return raised;
}
static void status_forget_stream(int device, void* stream) {
  std::lock_guard<std::mutex> lk(g_status_mu);
  auto it = g_stream_status.find({device, stream});
  if (it == g_stream_status.end()) return;
  status_pool().put(it->second);
  g_stream_status.erase(it);
}
void host::status_pool_stats(int64_t* words_out, int64_t* blocks) {
  StatusPool& sp = status_pool();
  std::lock_guard<std::mutex> lk(sp.mu);
  *words_out = sp.handed_out;
  *blocks = sp.blocks;
}
int host::singular_error() {
  return fail(ABRK_ESINGULAR, "Singular matrix: the joint-space inertia matrix M of at least one row is not positive "
                              "definite (numpy.linalg.inv(M) raises LinAlgError there, osc.py:136); the outputs of "
                              "those rows are unspecified");
}
int host::path_error() {
  return fail(ABRK_EPATH, "at least one row has no path: start == target, no max_v candidate whose ramps fit the curve "
                          "(the reference raises ValueError at path_planner.py:245), or fewer than 2 / more than 2e9 "
                          "steps; n_timesteps is 0 for those rows");
}
// what a drained stream reports: a singular batch first, else a row without a path
static int status_error(int raised) { return (raised & kStatusSingular) ? singular_error() : path_error(); }

extern "C" int abrk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}
extern "C" int abrk_device_name(int device, char* buf, size_t len) {
  if (int rc = use_device(device)) return rc;
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, device));
  // the marketing name comes from libdrm's amdgpu.ids, which minimal images lack: fall back to the architecture
  snprintf(buf, len, "%s (%s, %d CUs)", p.name[0] ? p.name : "AMD GPU", p.gcnArchName, p.multiProcessorCount);
  return 0;
}
extern "C" void* abrk_malloc(int device, size_t bytes) {
  if (use_device(device)) return nullptr;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    fail(ABRK_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return nullptr;
  }
  return p;
}
extern "C" int abrk_free(int device, void* p) {
  if (int rc = use_device(device)) return rc;
  HIPCHK(hipFree(p));
  return 0;
}
extern "C" int abrk_memcpy_h2d(int device, void* dst, const void* src, size_t bytes, void* stream) {
  if (int rc = use_device(device)) return rc;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
extern "C" int abrk_memcpy_d2h(int device, void* dst, const void* src, size_t bytes, void* stream) {
  if (int rc = use_device(device)) return rc;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  // the stream is drained: a singular batch enqueued on it earlier is reported here (the bytes ARE copied; the torques of
  // the offending rows are unspecified - a caller that reads results back this way must not get them silently)
  if (const int raised = status_take(device, stream, false)) return status_error(raised);
  return 0;
}
extern "C" int abrk_memset(int device, void* dst, int value, size_t bytes, void* stream) {
  if (int rc = use_device(device)) return rc;
  HIPCHK(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
  return 0;
}
extern "C" void* abrk_stream_create(int device) {
  if (use_device(device)) return nullptr;
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    fail(ABRK_ENODEV, "hipStreamCreate failed");
    return nullptr;
  }
  return s;
}
extern "C" int abrk_stream_destroy(int device, void* stream) {
  if (int rc = use_device(device)) return rc;
  if (stream) wl_forget_stream(device, (hipStream_t)stream);
  HIPCHK(hipStreamDestroy((hipStream_t)stream));  // (waits for the stream's work: nothing writes its word any more)
  if (stream) status_forget_stream(device, stream);
  return 0;
}
extern "C" int abrk_stream_sync(int device, void* stream) {
  if (int rc = use_device(device)) return rc;
  // ABRK_SYNC_SPIN=1 (measurement switch): poll the stream instead of blocking in hipStreamSynchronize - whether the
  // wake-up latency of the blocking wait shows in a 20-step replay (it does not: profiles/round3/launch_latency.txt)
  static const bool spin = measurement_env("ABRK_SYNC_SPIN") != nullptr;
  if (spin) {
    hipError_t e;
    while ((e = hipStreamQuery((hipStream_t)stream)) == hipErrorNotReady) {
    }
    (void)hipGetLastError();
    HIPCHK(e);
  } else {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  }
  // the "M not positive definite" flag of THIS stream's asynchronous (device-pointer) OSC calls: reported once
  if (const int raised = status_take(device, stream, false)) return status_error(raised);
  return 0;
}
extern "C" int abrk_device_sync(int device) {
  if (int rc = use_device(device)) return rc;
  HIPCHK(hipDeviceSynchronize());
  if (const int raised = status_take(device, nullptr, true)) return status_error(raised);  // every stream is drained
  return 0;
}
extern "C" void* abrk_event_create(int device) {
  if (use_device(device)) return nullptr;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) {
    (void)hipGetLastError();
    fail(ABRK_ENODEV, "hipEventCreate failed");
    return nullptr;
  }
  return e;
}
extern "C" int abrk_event_destroy(int device, void* ev) {
  if (int rc = use_device(device)) return rc;
  HIPCHK(hipEventDestroy((hipEvent_t)ev));
  return 0;
}
extern "C" int abrk_event_record(int device, void* ev, void* stream) {
  if (int rc = use_device(device)) return rc;
  HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
  return 0;
}
extern "C" int abrk_event_elapsed_ms(int device, void* start, void* stop, float* ms) {
  if (int rc = use_device(device)) return rc;
  HIPCHK(hipEventSynchronize((hipEvent_t)stop));
  HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return 0;
}

// ------------------------------------------------------------------------------- staging
namespace {
// Per-thread device scratch arena for host-pointer arguments (grown on demand, reused).
struct Arena {
  int device = -1;
  char* base = nullptr;
  size_t cap = 0, used = 0;
};
thread_local Arena t_arena;

// Small host batches (a control loop calling with B = 1 .. a few thousand rows) skip the copy engine: the
// arguments are packed by the CPU into a pinned, device-mapped arena that the kernel reads and writes directly
// over PCIe - one launch and one stream sync instead of 3-4 hipMemcpyAsync calls of a few hundred bytes each.
// Above ABRK_ZEROCOPY_MAX bytes (default 1 MiB) the copy engine + device scratch arena wins.
struct PinArena {
  char* base = nullptr;  // the memory as the host sees it
  char* dev = nullptr;   // the same memory as the device sees it
  size_t cap = 0;
};
thread_local PinArena t_pin;
size_t zero_copy_max() {
  static const size_t v = [] {
    const char* e = getenv("ABRK_ZEROCOPY_MAX");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)1 << 20;
  }();
  return v;
}

}  // namespace

// Pinned host memory (hipHostMalloc / hipHostRegister) is device-visible: it is passed through and read in place.
void* host::device_view(const void* p) {
  hipPointerAttribute_t at;
  hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // plain malloc'ed host memory is "invalid value" to HIP
    return nullptr;
  }
  if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) return const_cast<void*>(p);
  if (at.type == hipMemoryTypeHost && at.devicePointer) return at.devicePointer;
  return nullptr;
}

int Stager::reserve() {
  if (items.empty()) return 0;
  staged = true;
  if (recording()) return fail(ABRK_EINVAL, "plans take device pointers only (got a host pointer)");
  if (need <= zero_copy_max()) {
    PinArena& pa = t_pin;
    if (pa.cap < need) {
      if (pa.base) (void)hipHostFree(pa.base);
      pa.base = pa.dev = nullptr;
      pa.cap = 0;
      size_t cap = need < (64u << 10) ? (64u << 10) : need;
      void* h = nullptr;
      hipError_t e = hipHostMalloc(&h, cap, hipHostMallocMapped | hipHostMallocPortable);
      void* d = nullptr;
      if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        if (h) (void)hipHostFree(h);
        return fail(ABRK_ENOMEM, "pinned staging hipHostMalloc(%zu): %s", cap, hipGetErrorString(e));
      }
      pa.base = (char*)h;
      pa.dev = (char*)d;
      pa.cap = cap;
    }
    pinned = true;
    size_t off = 0;
    for (auto& it : items) {
      it.dev = *it.field = pa.dev + off;
      if (it.in) memcpy(pa.base + off, it.host, it.bytes);
      off += (it.bytes + 255) & ~size_t(255);
    }
    return 0;
  }
  Arena& a = t_arena;
  if (a.device != device || a.cap < need) {
    if (a.base) {
      (void)hipSetDevice(a.device);
      (void)hipFree(a.base);
      (void)hipSetDevice(device);
    }
    a.base = nullptr;
    a.cap = 0;
    size_t cap = need < (1u << 20) ? (1u << 20) : need + need / 4;
    hipError_t e = hipMalloc((void**)&a.base, cap);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(ABRK_ENOMEM, "staging hipMalloc(%zu): %s", cap, hipGetErrorString(e));
    }
    a.cap = cap;
    a.device = device;
  }
  size_t off = 0;
  for (auto& it : items) {
    it.dev = *it.field = a.base + off;
    off += (it.bytes + 255) & ~size_t(255);
    if (it.in) {
      hipError_t e = hipMemcpyAsync(it.dev, it.host, it.bytes, hipMemcpyHostToDevice, stream);
      if (e != hipSuccess) return fail(ABRK_ENODEV, "H2D staging: %s", hipGetErrorString(e));
    }
  }
  return 0;
}
int Stager::finish() {
  if (!staged) return 0;
  if (pinned) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(ABRK_ENODEV, "stream sync: %s", hipGetErrorString(e));
    for (auto& it : items)
      if (it.out) memcpy(it.host, t_pin.base + ((char*)it.dev - t_pin.dev), it.bytes);
    return 0;
  }
  for (auto& it : items)
    if (it.out) {
      hipError_t e = hipMemcpyAsync(it.host, it.dev, it.bytes, hipMemcpyDeviceToHost, stream);
      if (e != hipSuccess) return fail(ABRK_ENODEV, "D2H staging: %s", hipGetErrorString(e));
    }
  hipError_t e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(ABRK_ENODEV, "stream sync: %s", hipGetErrorString(e));
  return 0;
}

// ------------------------------------------------------------------------------- launch plans
static thread_local Recorder* t_rec = nullptr;
Recorder*& host::recorder() { return t_rec; }
// A plan is the list of kernel launches recorded between abrk_plan_begin and abrk_plan_end (one control tick: one
// law, or several secondary controllers accumulating into the buffer the OSC law then filters).  Launching it only
// enqueues those kernels on the plan's stream - no validation, no pointer classification, no locks, no staging.
namespace {
struct Plan {
  int id = -1;
  Recorder rec;  // what was recorded, device scratch included: the plan owns it from abrk_plan_end on
  explicit Plan(Recorder&& r) : rec(std::move(r)) {}
  hipError_t enqueue() const {
    for (const auto& f : rec.steps) {
      hipError_t e = f();
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  int graph_repeat = 0;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  void drop_graph() {
    if (graph_exec || graph) {
      if (hipSetDevice(rec.device) == hipSuccess) {
        t_current_device = rec.device;
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (graph) (void)hipGraphDestroy(graph);
      }
      (void)hipGetLastError();
    }
    graph_exec = nullptr;
    graph = nullptr;
    graph_repeat = 0;
  }
};
// Slot table: abrk_plan_launch reads a slot without taking the lock (hot path of a control loop).  Slots are
// recycled: a plan id is slot | generation << 12, so a stale id of a destroyed plan never matches the slot's new
// tenant; the payload of a destroyed plan is freed.  (Destroying a plan while another thread launches it is a
// caller error, as with any handle.)
constexpr int kSlotBits = 12, kMaxPlans = 1 << kSlotBits, kGenMask = (1 << (31 - kSlotBits)) - 1;
std::mutex g_plan_mu;
Plan* g_plans[kMaxPlans] = {};
int g_plan_gen[kMaxPlans] = {};
std::vector<int> g_plan_free;
int g_plan_hi = 0;  // slots [0, g_plan_hi) have been handed out at least once

Plan* find_plan(int id) {
  if (id < 0) return nullptr;
  Plan* pl = __atomic_load_n(&g_plans[id & (kMaxPlans - 1)], __ATOMIC_ACQUIRE);
  return (pl && pl->id == id) ? pl : nullptr;
}
int register_plan(Plan* pl) {
  std::lock_guard<std::mutex> lk(g_plan_mu);
  int slot;
  if (!g_plan_free.empty()) {
    slot = g_plan_free.back();
    g_plan_free.pop_back();
  } else if (g_plan_hi < kMaxPlans) {
    slot = g_plan_hi++;
  } else {
    delete pl;
    return fail(ABRK_ENOMEM, "too many live plans (max %d)", kMaxPlans);
  }
  pl->id = slot | (g_plan_gen[slot] << kSlotBits);
  __atomic_store_n(&g_plans[slot], pl, __ATOMIC_RELEASE);
  return pl->id;
}
void free_dev_bufs(int device, std::vector<void*>& bufs) {
  if (bufs.empty()) return;
  if (hipSetDevice(device) == hipSuccess) {
    t_current_device = device;
    for (void* p : bufs) (void)hipFree(p);
  }
  (void)hipGetLastError();
  bufs.clear();
}
void abort_recording() {
  if (t_rec) free_dev_bufs(t_rec->device, t_rec->dev_bufs);
  delete t_rec;
  t_rec = nullptr;
}
}  // namespace

extern "C" int abrk_plan_begin(int device, void* stream) {
  if (t_rec) return fail(ABRK_EINVAL, "this thread is already recording a plan");
  if (int rc = use_device(device)) return rc;
  t_rec = new Recorder;
  t_rec->device = device;
  t_rec->stream = (hipStream_t)stream;
  return 0;
}

extern "C" int abrk_plan_abort(void) {
  abort_recording();
  return 0;
}

extern "C" int abrk_plan_end(void) {
  if (!t_rec) return fail(ABRK_EINVAL, "abrk_plan_end without abrk_plan_begin");
  if (t_rec->steps.empty()) {
    abort_recording();
    return fail(ABRK_EINVAL, "nothing was recorded (every call had B == 0 or failed)");
  }
  Plan* pl = new Plan(std::move(*t_rec));  // (a moved-from vector is empty: abort_recording() frees nothing)
  abort_recording();
  return register_plan(pl);
}

// the two original single-law plans: record exactly one call
template <class Call>
static int plan_of_one(int64_t B, int device, void* stream, Call&& call) {
  if (B <= 0) return fail(ABRK_EINVAL, "a plan needs a positive batch");
  if (int rc = abrk_plan_begin(device, stream)) return rc;
  if (int rc = call()) {
    abort_recording();
    return rc;
  }
  return abrk_plan_end();
}
extern "C" int abrk_osc_plan_create(int arm_id, int dtype, const abrk_osc_params* P, int64_t B, const void* q,
                                    const void* dq, const void* target, const void* target_velocity,
                                    void* integrated_error, const void* u_null_ext, void* u,
                                    void* training_signal, int device, void* stream) {
  return plan_of_one(B, device, stream, [&] {
    return abrk_osc_generate_batch(arm_id, dtype, P, B, q, dq, target, target_velocity, integrated_error, u_null_ext, u,
                                   training_signal, device, stream);
  });
}

extern "C" int abrk_sliding_plan_create(int arm_id, int dtype, const abrk_sliding_params* P, int64_t B, const void* q,
                                        const void* dq, const void* target, const void* target_velocity,
                                        const void* target_acc, void* u, void* s_out, int device, void* stream) {
  return plan_of_one(B, device, stream, [&] {
    return abrk_sliding_generate_batch(arm_id, dtype, P, B, q, dq, target, target_velocity, target_acc, u, s_out, device, stream);
  });
}

namespace {
// make the plan's device current (plan launches skip hipSetDevice when this thread is already on it)
int use_plan_device(const Plan* pl) {
  if (t_current_device != pl->rec.device) {
    HIPCHK(hipSetDevice(pl->rec.device));
    t_current_device = pl->rec.device;
  }
  return 0;
}
}  // namespace

extern "C" int abrk_plan_launch(int plan) { return abrk_plan_launch_repeat(plan, 1); }

extern "C" int abrk_plan_launch_repeat(int plan, int repeat) {
  Plan* pl = find_plan(plan);
  if (!pl) return fail(ABRK_EINVAL, "unknown plan %d", plan);
  if (repeat < 1) return fail(ABRK_EINVAL, "repeat must be >= 1");
  if (int rc = use_plan_device(pl)) return rc;
  for (int i = 0; i < repeat; i++) HIPCHK(pl->enqueue());
  return 0;
}

extern "C" int abrk_plan_launch_graph(int plan, int repeat) {
  Plan* pl = find_plan(plan);
  if (!pl) return fail(ABRK_EINVAL, "unknown plan %d", plan);
  if (repeat < 1) return fail(ABRK_EINVAL, "repeat must be >= 1");
  if (int rc = use_plan_device(pl)) return rc;
  if (!pl->rec.stream) return fail(ABRK_EINVAL, "graph launches need a plan created on an explicit stream");
  if (pl->graph_repeat != repeat) {
    pl->drop_graph();
    HIPCHK(hipStreamBeginCapture(pl->rec.stream, hipStreamCaptureModeThreadLocal));
    hipError_t le = hipSuccess;
    for (int i = 0; i < repeat && le == hipSuccess; i++) le = pl->enqueue();
    hipError_t ce = hipStreamEndCapture(pl->rec.stream, &pl->graph);
    if (le != hipSuccess || ce != hipSuccess)
      return fail(ABRK_ENODEV, "graph capture failed: %s", hipGetErrorString(le != hipSuccess ? le : ce));
    HIPCHK(hipGraphInstantiate(&pl->graph_exec, pl->graph, nullptr, nullptr, 0));
    // (hipGraphUpload here was measured in round 3: no change to a 20-step replay - 4.83 us per step of wall clock with
    //  and without, the graph's first launch is an untimed warm-up anyway - and one more call for rocprofv3 to trip over)
    pl->graph_repeat = repeat;
  }
  HIPCHK(hipGraphLaunch(pl->graph_exec, pl->rec.stream));
  return 0;
}

// One tick (or `repeat` of them) of SEVERAL plans from one call - the plans of a sharded control loop, one per shard /
// device: mode 0 = `repeat` plain launches of each plan, 1 = one hipGraph of `repeat` ticks per plan (captured on first use,
// abrk_plan_launch_graph).  Every device has its work before the call returns; nothing is waited for.
extern "C" int abrk_plans_launch(const int* plans, int n_plans, int repeat, int mode) {
  if (!plans || n_plans < 1) return fail(ABRK_EINVAL, "plans / n_plans");
  if (mode != 0 && mode != 1) return fail(ABRK_EINVAL, "mode must be 0 (plain launches) or 1 (graph replay)");
  for (int i = 0; i < n_plans; i++)
    if (int rc = mode ? abrk_plan_launch_graph(plans[i], repeat) : abrk_plan_launch_repeat(plans[i], repeat)) return rc;
  return 0;
}

extern "C" int abrk_plan_destroy(int plan) {
  std::lock_guard<std::mutex> lk(g_plan_mu);
  Plan* pl = find_plan(plan);
  if (!pl) return fail(ABRK_EINVAL, "unknown plan %d", plan);
  const int slot = plan & (kMaxPlans - 1);
  __atomic_store_n(&g_plans[slot], (Plan*)nullptr, __ATOMIC_RELEASE);
  g_plan_gen[slot] = (g_plan_gen[slot] + 1) & kGenMask;
  g_plan_free.push_back(slot);
  pl->drop_graph();
  free_dev_bufs(pl->rec.device, pl->rec.dev_bufs);
  delete pl;
  return 0;
}

extern "C" int abrk_plan_count(void) {
  std::lock_guard<std::mutex> lk(g_plan_mu);
  return g_plan_hi - (int)g_plan_free.size();
}

// abrk_host_shard.cpp - one batch over several devices: the *_sharded and *_resident entry points.
#include <thread>

#include "abrk_host.h"

// ------------------------------------------------------------------------------- host arrays over several devices
// One call, host arrays, all the devices the caller names (BASELINE config 4: 2^20 rows over 8 GPUs; run_sharded below).
// The shards of one DEVICE are one unit of work - staged in, launched and collected by one host thread per device (the
// calling thread takes the first device, short-lived workers the others), under that device's lock only: the staging
// copies (pageable host memory: synchronous on the thread that issues them) of different devices run side by side, and
// calls on disjoint device sets do not wait for each other.  Callers that keep their shards RESIDENT use the
// abrk_*_resident entry points below (device pointer tables, enqueue only) or one process per GPU (bench.py --gpus N).
namespace {
struct ShardCtx {
  hipStream_t stream = nullptr;
  char* base = nullptr;
  size_t cap = 0;
};
constexpr int kMaxShardDevices = 64;
std::mutex g_shard_mu;                       // the registry below (look-ups only)
std::mutex g_shard_dev_mu[kMaxShardDevices];  // the scratch arenas of one device's contexts (held while a call uses them)
// (device, slot on that device) -> context; heap-allocated: the pointers handed out stay valid as the table grows
std::vector<std::pair<std::pair<int, int>, std::unique_ptr<ShardCtx>>> g_shard_ctx;

// the context of (device, slot), its stream created; the calling thread's current device must be `device`
ShardCtx* shard_ctx_find(int device, int slot) {
  std::lock_guard<std::mutex> lk(g_shard_mu);
  ShardCtx* c = nullptr;
  for (auto& e : g_shard_ctx)
    if (e.first.first == device && e.first.second == slot) c = e.second.get();
  if (!c) {
    g_shard_ctx.emplace_back(std::make_pair(device, slot), std::unique_ptr<ShardCtx>(new ShardCtx));
    c = g_shard_ctx.back().second.get();
  }
  if (!c->stream && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
  return c;
}
// ... with at least `need` bytes of device scratch (caller holds g_shard_dev_mu[device])
ShardCtx* shard_ctx(int device, int slot, size_t need) {
  ShardCtx* c = shard_ctx_find(device, slot);
  if (!c) return nullptr;
  if (c->cap < need) {
    if (c->base) {
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(c->base);
    }
    c->base = nullptr;
    c->cap = 0;
    const size_t cap = need + need / 4;
    if (hipMalloc((void**)&c->base, cap) != hipSuccess) return nullptr;
    c->cap = cap;
  }
  return c;
}
}  // namespace

namespace {
// One host batch over several devices: [0, B) is cut into n_shards contiguous row ranges (sizes differing by at most one
// row - abr_control_amd/sharding.py shard_range), the pieces of shard g are staged to devices[g] on a stream of its own,
// `call(dev, rows, device, stream)` enqueues the shard through the family's single-device call (dev[k]: device address
// of array k of the table, null for an absent one; -> an ABRK_* code), and only when every shard of a device is in
// flight are that device's results collected.  No collective: rows are independent.
// Lock order: g_shard_dev_mu[device] is held while a shard's launch takes the six-row law's worklist slot mutex of its
// (device, stream) (worklist_for); the *_resident calls take slot mutexes without a device lock, and nothing takes a
// device lock while holding a slot mutex - keep it one-way.
// table(): the family's arrays, asked for once `call` has accepted the arguments (B = 0 returns right after its
// checks); host[k]: the caller's array k.
template <class Table, class Call>
int run_sharded(int dtype, int64_t B, int n_shards, const int* devices, void* const* host, Table&& table, Call&& call) {
  if (n_shards < 1 || !devices) return fail(ABRK_EINVAL, "n_shards must be >= 1 and devices non-NULL");
  if (int rc = call(host, 0, devices[0], nullptr)) return rc;
  const ArrayTable t = table();
  struct Piece {
    char* host;      // null: absent (not given, or not used by this call)
    size_t per_row;  // bytes
  } pieces[kMaxArrays];
  const int n_pieces = t.n;
  for (int k = 0; k < n_pieces; k++) pieces[k] = {t.a[k].used ? (char*)host[k] : nullptr, t.a[k].per_row * esz(dtype)};
  if (recording()) return fail(ABRK_EINVAL, "a sharded entry point cannot be recorded into a plan");
  if (B < 0) return fail(ABRK_EINVAL, "negative batch %lld", (long long)B);
  if (B == 0) return 0;
  for (int k = 0; k < n_pieces; k++) {
    hipPointerAttribute_t at;
    if (pieces[k].host && hipPointerGetAttributes(&at, pieces[k].host) == hipSuccess && at.type == hipMemoryTypeDevice)
      return fail(ABRK_EINVAL, "the *_sharded entry points take host arrays (a device pointer lives on one device); "
                               "shards that live on the devices go through the *_resident entry points");
    (void)hipGetLastError();  // plain malloc'ed memory is "invalid value" to HIP
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(ABRK_ENODEV, "no HIP device available; libabrk has no CPU fallback");
  }
  for (int g = 0; g < n_shards; g++)
    if (devices[g] < 0 || devices[g] >= ndev || devices[g] >= kMaxShardDevices)
      return fail(ABRK_EINVAL, "device %d outside 0..%d", devices[g], ndev - 1);
  struct Shard {
    ShardCtx* c;
    int device, slot, index;
    int64_t r0, rows;
    void* dev[kMaxArrays];
  };
  std::vector<Shard> shards;
  std::vector<int> per_dev(ndev, 0), order;  // order: the distinct devices, as first named
  for (int g = 0; g < n_shards; g++) {
    const int64_t base = B / n_shards, extra = B % n_shards;
    const int64_t r0 = g * base + (g < extra ? g : extra), r1 = r0 + base + (g < extra ? 1 : 0);
    if (r1 == r0) continue;
    Shard sh{};
    sh.device = devices[g];
    sh.index = g;
    sh.r0 = r0;
    sh.rows = r1 - r0;
    if (per_dev[sh.device] == 0) order.push_back(sh.device);
    sh.slot = per_dev[sh.device]++;
    shards.push_back(sh);
  }
  // everything one device has to do (its lock held throughout: the contexts' scratch arenas are per (device, slot))
  auto device_work = [&](int device) -> int {
    std::lock_guard<std::mutex> lk(g_shard_dev_mu[device]);
    HIPCHK(hipSetDevice(device));
    current_device() = device;
    for (Shard& sh : shards) {
      if (sh.device != device) continue;
      size_t need = 0;
      for (int k = 0; k < n_pieces; k++)
        if (pieces[k].host) need += (sh.rows * pieces[k].per_row + 255) & ~size_t(255);
      sh.c = shard_ctx(device, sh.slot, need);
      if (!sh.c) {
        (void)hipGetLastError();
        return fail(ABRK_ENOMEM, "shard %d: stream / %zu bytes of scratch on device %d", sh.index, need, device);
      }
      size_t off = 0;
      for (int k = 0; k < n_pieces; k++) {
        const Piece& pc = pieces[k];
        sh.dev[k] = nullptr;
        if (!pc.host) continue;
        sh.dev[k] = sh.c->base + off;
        off += (sh.rows * pc.per_row + 255) & ~size_t(255);
        if (t.a[k].in)
          HIPCHK(hipMemcpyAsync(sh.dev[k], pc.host + sh.r0 * pc.per_row, sh.rows * pc.per_row, hipMemcpyHostToDevice,
                                sh.c->stream));
      }
      if (int rc = call(sh.dev, sh.rows, device, sh.c->stream)) return rc;
    }
    // every kernel of this device is enqueued; now collect (a device-to-host copy into pageable memory waits for its shard)
    for (Shard& sh : shards) {
      if (sh.device != device) continue;
      for (int k = 0; k < n_pieces; k++)
        if (t.a[k].out && sh.dev[k])
          HIPCHK(hipMemcpyAsync(pieces[k].host + sh.r0 * pieces[k].per_row, sh.dev[k], sh.rows * pieces[k].per_row,
                                hipMemcpyDeviceToHost, sh.c->stream));
      HIPCHK(hipStreamSynchronize(sh.c->stream));
    }
    return 0;
  };
  if (order.size() == 1) return device_work(order[0]);
  // several devices: one host thread each (the caller's own for the first); a worker's error text travels back with its code
  std::vector<int> rcs(order.size(), 0);
  std::vector<std::string> msgs(order.size());
  std::vector<std::thread> workers;
  for (size_t i = 1; i < order.size(); i++)
    workers.emplace_back([&, i] {
      rcs[i] = device_work(order[i]);
      if (rcs[i]) msgs[i] = err_text();
    });
  rcs[0] = device_work(order[0]);
  if (rcs[0]) msgs[0] = err_text();
  for (auto& w : workers) w.join();
  (void)hipSetDevice(order[0]);
  current_device() = order[0];
  for (size_t i = 0; i < order.size(); i++)
    if (rcs[i]) {
      err_text() = msgs[i];
      return rcs[i];
    }
  return 0;
}
}  // namespace

extern "C" int abrk_osc_generate_sharded(int arm_id, int dtype, const abrk_osc_params* P, int64_t B, const void* q,
                                         const void* dq, const void* target, const void* target_velocity,
                                         void* integrated_error, const void* u_null_ext, void* u,
                                         void* training_signal, int n_shards, const int* devices) {
  void* const host[] = {(void*)q, (void*)dq, (void*)target, (void*)target_velocity, integrated_error, (void*)u_null_ext,
                        u, training_signal};
  // a synchronous call: the calling thread's word, shared by every shard (portable pinned host memory), reports this
  // batch alone - the words of the shard streams (left there by *_resident calls) are neither cleared nor taken.  It
  // is taken once the arguments are accepted: `table` runs right after the validation pass, on the calling thread
  StatusWord none, *sw = nullptr;
  const auto table = [&] {
    if ((sw = status_word(true, 0))) *sw->host = 0;
    return osc_arrays(get_arm(arm_id)->desc.n_joints, P->ki != 0, 0);
  };
  const int rc = run_sharded(dtype, B, n_shards, devices, host, table, [&](void* const* arr, int64_t rows, int device, void* st) {
    return osc_call(arm_id, dtype, P, rows, arr, 0, device, st, sw ? sw : &none);
  });
  return rc == 0 && sw && sw->take() ? singular_error() : rc;
}

extern "C" int abrk_sliding_generate_sharded(int arm_id, int dtype, const abrk_sliding_params* P, int64_t B,
                                             const void* q, const void* dq, const void* target,
                                             const void* target_velocity, const void* target_acc, void* u, void* s_out,
                                             int n_shards, const int* devices) {
  void* const host[] = {(void*)q, (void*)dq, (void*)target, (void*)target_velocity, (void*)target_acc, u, s_out};
  const auto table = [&] { return sliding_arrays(get_arm(arm_id)->desc.n_joints, P->cartesian != 0); };
  return run_sharded(dtype, B, n_shards, devices, host, table, [&](void* const* arr, int64_t rows, int device, void* st) {
    return sliding_call(arm_id, dtype, P, rows, arr, device, st);
  });
}

extern "C" int abrk_joint_generate_sharded(int arm_id, int dtype, const abrk_null_ctrl* ctrl, int account_for_gravity,
                                           int64_t B, const void* q, const void* dq, const void* target,
                                           const void* target_velocity, void* u, int n_shards, const int* devices) {
  void* const host[] = {(void*)q, (void*)dq, (void*)target, (void*)target_velocity, u};
  const auto table = [&] { return joint_arrays(get_arm(arm_id)->desc.n_joints); };
  return run_sharded(dtype, B, n_shards, devices, host, table, [&](void* const* arr, int64_t rows, int device, void* st) {
    return joint_call(arm_id, dtype, ctrl, account_for_gravity, rows, arr, device, st);
  });
}

extern "C" int abrk_dynamics_sharded(int arm_id, int dtype, int64_t B, const void* q, const void* dq, int frame,
                                     const double* x_off, uint32_t want, const abrk_dyn_out* out, int n_shards,
                                     const int* devices) {
  void* host[12] = {(void*)q, (void*)dq};
  if (out) memcpy(host + 2, out, sizeof *out);
  const auto table = [&] { return dynamics_arrays(get_arm(arm_id)->desc.n_joints, want); };
  return run_sharded(dtype, B, n_shards, devices, host, table, [&](void* const* arr, int64_t rows, int device, void* st) {
    return dynamics_call(arm_id, dtype, rows, arr, frame, x_off, want, device, st);
  });
}

// ------------------------------------------------------------------------------- resident shards
// "Results remain in per-device buffers unless the caller asks for host arrays": a batch whose shards LIVE on the
// devices.  Every array argument is a table of n_shards device pointers (shard g: rows[g] rows on devices[g]); a call
// only ENQUEUES - shard g's kernels on shard g's stream, nothing is staged, nothing is waited for - by going through the
// single-device entry point of the same name once per shard (so everything that holds there holds here: the six-row
// law's (device, stream) scratch, the per-(device, stream) ABRK_ESINGULAR word, per-row state staying with its shard).
// abrk_shards_sync drains the shards' streams.  One host thread, N GPUs, no collective.
namespace {
int check_cut(const abrk_shard_cut* cut) {
  if (!cut || cut->n_shards < 1 || !cut->devices || !cut->rows)
    return fail(ABRK_EINVAL, "shard cut: n_shards >= 1, devices and rows are required");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(ABRK_ENODEV, "no HIP device available; libabrk has no CPU fallback");
  }
  for (int g = 0; g < cut->n_shards; g++) {
    if (cut->devices[g] < 0 || cut->devices[g] >= ndev || cut->devices[g] >= kMaxShardDevices)
      return fail(ABRK_EINVAL, "shard %d: device %d outside 0..%d", g, cut->devices[g], ndev - 1);
    if (cut->rows[g] < 0) return fail(ABRK_EINVAL, "shard %d: negative row count", g);
  }
  return 0;
}
// the stream shard g runs on: the caller's, or the library's stream of (device, k) for the k-th shard named on that device
int cut_stream(const abrk_shard_cut* cut, int g, void** out) {
  if (cut->streams) {
    *out = cut->streams[g];
    return 0;
  }
  int slot = 0;
  for (int h = 0; h < g; h++) slot += cut->devices[h] == cut->devices[g] ? 1 : 0;
  if (int rc = use_device(cut->devices[g])) return rc;
  ShardCtx* c = shard_ctx_find(cut->devices[g], slot);
  if (!c) {
    (void)hipGetLastError();
    return fail(ABRK_ENODEV, "shard %d: no stream on device %d", g, cut->devices[g]);
  }
  *out = c->stream;
  return 0;
}
// a resident array must be memory the device reads in place: device memory or pinned host memory
int check_resident(int g, const char* name, const void* p) {
  if (!p) return 0;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ABRK_EINVAL, "shard %d: %s is a pageable host pointer - the *_resident entry points take device "
                             "pointers (host arrays go through the *_sharded entry points)", g, name);
  }
  return 0;
}
template <class Call>
int for_each_shard(const abrk_shard_cut* cut, Call&& call) {
  if (int rc = check_cut(cut)) return rc;
  for (int g = 0; g < cut->n_shards; g++) {
    if (cut->rows[g] == 0) continue;
    void* stream = nullptr;
    if (int rc = cut_stream(cut, g, &stream)) return rc;
    if (int rc = call(g, cut->devices[g], cut->rows[g], stream)) return rc;
  }
  return 0;
}
// The shards of a resident batch through the family's call, one after the other.  tabs[k]: the pointer table of array
// k of `t` (NULL: absent in every shard); the arrays past n_tabs are the pointers of out[g], of which a call uses (and
// this checks) only the ones asked for.
template <class Call>
int run_resident(const abrk_shard_cut* cut, const ArrayTable& t, const void* const* const* tabs, int n_tabs,
                 const abrk_dyn_out* out, Call&& call) {
  return for_each_shard(cut, [&](int g, int device, int64_t rows, void* stream) -> int {
    void* arr[kMaxArrays];
    for (int k = 0; k < t.n; k++) {
      if (k < n_tabs) arr[k] = tabs[k] ? (void*)tabs[k][g] : nullptr;
      else arr[k] = ((void* const*)&out[g])[k - n_tabs];
      if (k < n_tabs || t.a[k].used)
        if (int rc = check_resident(g, t.a[k].name, arr[k])) return rc;
    }
    return call(arr, rows, device, stream);
  });
}
}  // namespace

extern "C" void* abrk_shard_stream(int device, int slot) {
  if (slot < 0 || device >= kMaxShardDevices || use_device(device)) return nullptr;
  ShardCtx* c = shard_ctx_find(device, slot);
  if (!c) {
    (void)hipGetLastError();
    fail(ABRK_ENODEV, "no stream for (device %d, slot %d)", device, slot);
    return nullptr;
  }
  return c->stream;
}

extern "C" int abrk_osc_generate_resident(int arm_id, int dtype, const abrk_osc_params* P, const abrk_shard_cut* cut,
                                          const void* const* q, const void* const* dq, const void* const* target,
                                          const void* const* target_velocity, void* const* integrated_error,
                                          const void* const* u_null_ext, void* const* u, void* const* training_signal) {
  if (!q || !dq || !target || !u) return fail(ABRK_EINVAL, "q, dq, target and u are required");
  const void* const* const tabs[] = {q, dq, target, target_velocity, (const void* const*)integrated_error, u_null_ext,
                                     (const void* const*)u, (const void* const*)training_signal};
  return run_resident(cut, osc_arrays(0, false, 0), tabs, 8, nullptr, [&](void* const* arr, int64_t rows, int device, void* st) {
    return osc_call(arm_id, dtype, P, rows, arr, 0, device, st, nullptr);
  });
}

extern "C" int abrk_sliding_generate_resident(int arm_id, int dtype, const abrk_sliding_params* P,
                                              const abrk_shard_cut* cut, const void* const* q, const void* const* dq,
                                              const void* const* target, const void* const* target_velocity,
                                              const void* const* target_acc, void* const* u, void* const* s_out) {
  if (!q || !dq || !target || !u) return fail(ABRK_EINVAL, "q, dq, target and u are required");
  const void* const* const tabs[] = {q, dq, target, target_velocity, target_acc, (const void* const*)u,
                                     (const void* const*)s_out};
  return run_resident(cut, sliding_arrays(0, false), tabs, 7, nullptr, [&](void* const* arr, int64_t rows, int device, void* st) {
    return sliding_call(arm_id, dtype, P, rows, arr, device, st);
  });
}

extern "C" int abrk_joint_generate_resident(int arm_id, int dtype, const abrk_null_ctrl* ctrl, int account_for_gravity,
                                            const abrk_shard_cut* cut, const void* const* q, const void* const* dq,
                                            const void* const* target, const void* const* target_velocity,
                                            void* const* u) {
  if (!q || !dq || !u) return fail(ABRK_EINVAL, "q, dq and u are required");
  const void* const* const tabs[] = {q, dq, target, target_velocity, (const void* const*)u};
  return run_resident(cut, joint_arrays(0), tabs, 5, nullptr, [&](void* const* arr, int64_t rows, int device, void* st) {
    return joint_call(arm_id, dtype, ctrl, account_for_gravity, rows, arr, device, st);
  });
}

extern "C" int abrk_dynamics_resident(int arm_id, int dtype, const abrk_shard_cut* cut, const void* const* q,
                                      const void* const* dq, int frame, const double* x_off, uint32_t want,
                                      const abrk_dyn_out* out) {
  if (!q || !out) return fail(ABRK_EINVAL, "q and out (one abrk_dyn_out per shard) are required");
  const void* const* const tabs[] = {q, dq};
  return run_resident(cut, dynamics_arrays(0, want), tabs, 2, out, [&](void* const* arr, int64_t rows, int device, void* st) {
    return dynamics_call(arm_id, dtype, rows, arr, frame, x_off, want, device, st);
  });
}

extern "C" int abrk_shards_sync(const abrk_shard_cut* cut) {
  // every stream is drained before anything is reported: a singular shard does not leave its neighbours running
  bool singular = false;
  int first_rc = 0;
  std::string first_msg;
  const int rc = for_each_shard(cut, [&](int, int device, int64_t, void* stream) -> int {
    const int r = abrk_stream_sync(device, stream);
    if (r == ABRK_ESINGULAR) singular = true;
    else if (r && !first_rc) {
      first_rc = r;
      first_msg = err_text();
    }
    return 0;
  });
  if (rc) return rc;
  if (first_rc) {
    err_text() = first_msg;
    return first_rc;
  }
  return singular ? singular_error() : 0;
}

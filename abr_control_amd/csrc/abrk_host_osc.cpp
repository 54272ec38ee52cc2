// abrk_host_osc.cpp - operational space control: the six-row kernels' scratch cache, the law and its helper methods.
#include <atomic>

#include "abrk_host.h"
#include "abrk_coop.h"
#include "abrk_params.h"

// ------------------------------------------------------------------------------- scratch of the six-row kernels
// Scratch of the six-row OSC kernels (rows whose law needs the truncating pseudo-inverse are deferred to a second pass;
// which form a batch takes: abrk_osc6_plan.h): wl_ints(B) ~ B + 20 k ints of device memory and - hand-over forms - a
// record of rec_len(n) values per row.  Immediate calls take both from a cache keyed by
// (device, stream) - calls on one stream are ordered, so the buffers can be reused - PROVIDED the launches that use
// them (counters' memset, pass 1, pass 2) enter the stream as a unit: several host threads may share a stream (every
// Python call without an explicit stream is on the NULL stream, and ctypes releases the GIL), and memset A, pass-1 A,
// memset B, pass-2 A would lose A's deferred rows (or overrun a list sized for one call).  So the caller keeps `hold` -
// the SLOT's mutex: calls on other streams and other devices do not wait for it - from here until its launches are
// enqueued (dispatch() releases it before any stream sync).  A grow frees the old buffers only after draining the
// slot's own stream, which - every earlier user having enqueued under the same lock - covers all of them; only callers
// of that one stream wait meanwhile.  The registry lock (g_wl_mu) is held for the look-up alone.  abrk_stream_destroy
// hands a stream's slot back; streams the caller destroyed behind the library's back are evicted once the cache is
// full (least recently used slot whose stream is idle or gone).  A recorded plan owns its worklist.
struct host::WorklistSlot {
  int device = 0;
  hipStream_t stream = nullptr;
  int* buf = nullptr;      // counters + row indices
  size_t cap = 0;          // bytes
  void* rec = nullptr;     // hand-over records
  size_t rec_cap = 0;      // bytes
  uint64_t last_use = 0;
  bool retired = false;    // left the cache (evicted / its stream destroyed): buffers released, never handed out again
  std::mutex mu;
};
namespace {
std::mutex g_wl_mu;
// shared ownership: a caller copies the pointer under g_wl_mu and locks the slot afterwards - an eviction or
// abrk_stream_destroy in that window removes the slot from the cache but cannot free the mutex under the caller
std::vector<std::shared_ptr<WorklistSlot>> g_wl_cache;
uint64_t g_wl_clock = 0;
std::atomic<int64_t> g_wl_inline_fallbacks{0}, g_wl_evictions{0};
constexpr size_t kWlCacheSlots = 64;

void wl_release(WorklistSlot& s) {  // caller holds s.mu; the slot's stream is drained
  (void)hipSetDevice(s.device);
  if (s.buf) (void)hipFree(s.buf);
  if (s.rec) (void)hipFree(s.rec);
  s.buf = nullptr;
  s.rec = nullptr;
  s.cap = s.rec_cap = 0;
}
// a slot that left the cache: wait for whoever is enqueueing on it, drain its stream if that still exists, free
void wl_retire(const std::shared_ptr<WorklistSlot>& s, bool stream_alive) {
  std::lock_guard<std::mutex> sl(s->mu);
  s->retired = true;
  if (stream_alive) {
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    (void)hipGetLastError();
  }
  wl_release(*s);
}
}  // namespace
// abrk_stream_destroy: the stream's slot leaves the cache (its launches are drained by the caller's hipStreamDestroy,
// which waits for the stream's work; the buffers are freed after an explicit drain here)
void host::wl_forget_stream(int device, hipStream_t stream) {
  std::shared_ptr<WorklistSlot> mine;
  {
    std::lock_guard<std::mutex> lk(g_wl_mu);
    for (size_t i = 0; i < g_wl_cache.size(); i++)
      if (g_wl_cache[i]->device == device && g_wl_cache[i]->stream == stream) {
        mine = std::move(g_wl_cache[i]);
        g_wl_cache.erase(g_wl_cache.begin() + i);
        break;
      }
  }
  if (mine) wl_retire(mine, true);  // (a caller that found the slot just before may still be enqueueing: s->mu)
}
namespace {
// the six-row law's measurement switches (abrk_osc6_plan.h), read once
const Osc6Switches& osc6_switches() {
  static const Osc6Switches sw = [] {
    Osc6Switches s;
    s.no_defer = measurement_env("ABRK_NO_DEFER") != nullptr;
    s.no_handover = measurement_env("ABRK_NO_HANDOVER") != nullptr;
    if (const char* e = measurement_env("ABRK_HANDOVER_MAX")) s.handover_max = atoll(e);
    if (const char* e = measurement_env("ABRK_DENSE_MAX")) s.dense_max = atoll(e);
    if (const char* e = measurement_env("ABRK_FINISH_SLOTS")) s.finish_slots = atoi(e);
    if (const char* e = measurement_env("ABRK_FINISH_ROUNDS")) s.finish_rounds = atoi(e);
    if (const char* e = measurement_env("ABRK_FINISH_GROUP")) s.finish_group = atoi(e);
    return s;
  }();
  return sw;
}
// one of the slot's two buffers grown to `need` bytes (+ 25 %); the other one is left alone.  The slot's stream is
// drained first if the old buffer may still be in use (every earlier user enqueued under s->mu).  false: no memory
bool wl_grow(hipStream_t stream, void** buf, size_t* cap, size_t need, bool* drained) {
  if (*cap >= need) return true;
  if (*buf) {
    if (!*drained) (void)hipStreamSynchronize(stream);
    *drained = true;
    (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
  }
  void* p = nullptr;
  if (hipMalloc(&p, need + need / 4) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  *buf = p;
  *cap = need + need / 4;
  return true;
}
// The scratch a plan other than OnePass needs, of (device, stream) or owned by the plan being recorded: -> 0 and *wl =
// the worklist / the chunks' masks, *rec = the record store (hand-over forms), or an error code.  An immediate call that
// finds no scratch runs the sweeps inline (same results): `plan` is then OnePass, *wl and *rec stay null.
// n / dtype: the arm's joint count and the arithmetic type (record size).
int worklist_for(int device, hipStream_t stream, int64_t B, int n, int dtype, Osc6Plan& plan, int** wl, void** rec,
                 WlHold& hold) {
  const bool handover = plan.uses_records();
  const auto inline_fallback = [&] {
    g_wl_inline_fallbacks++;
    plan = Osc6Plan{};
    return 0;
  };
  const size_t need = (size_t)wl_ints(B) * sizeof(int);
  // (hand-over forms keep one 64-bit mask per 64-row chunk in `wl` - far less than the recompute form's lists)
  // (whole chunks: the finish kernel asks for a chunk's slot before it knows whether a record is there)
  const size_t need_rec = handover ? (size_t)((B + kBlock - 1) / kBlock * kBlock) * rec_len(n) * esz(dtype) : 0;
  if (Recorder* r = recorder()) {
    void *p = nullptr, *q = nullptr;
    hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess && need_rec) e = hipMalloc(&q, need_rec);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      if (p) (void)hipFree(p);
      return fail(ABRK_ENOMEM, "worklist of the recorded six-row OSC call, hipMalloc(%zu + %zu): %s", need, need_rec,
                  hipGetErrorString(e));
    }
    r->dev_bufs.push_back(p);
    if (q) r->dev_bufs.push_back(q);
    *wl = (int*)p;
    *rec = q;
    return 0;
  }
  for (int attempt = 0;; attempt++) {
    std::shared_ptr<WorklistSlot> s, evicted;
    bool evicted_stream_alive = false;
    {
      std::lock_guard<std::mutex> lk(g_wl_mu);
      for (auto& e : g_wl_cache)
        if (e->device == device && e->stream == stream) s = e;
      if (!s) {
        if (g_wl_cache.size() >= kWlCacheSlots) {
          // full: the least recently used slot whose stream has nothing in flight (or no longer exists) makes room
          size_t pick = g_wl_cache.size();
          bool pick_alive = false;
          for (size_t i = 0; i < g_wl_cache.size(); i++) {
            WorklistSlot& c = *g_wl_cache[i];
            if (pick < g_wl_cache.size() && c.last_use >= g_wl_cache[pick]->last_use) continue;
            if (g_wl_cache[i].use_count() > 1) continue;  // a caller holds (or is about to lock) it
            if (!c.mu.try_lock()) continue;               // somebody is enqueueing on it
            (void)hipSetDevice(c.device);
            const hipError_t q = c.stream ? hipStreamQuery(c.stream) : hipErrorNotReady;  // the NULL stream stays
            (void)hipGetLastError();
            c.mu.unlock();
            if (q != hipErrorNotReady) {
              pick = i;
              pick_alive = q == hipSuccess;
            }
          }
          (void)hipSetDevice(device);
          if (pick == g_wl_cache.size()) return inline_fallback();  // every cached stream is busy
          g_wl_evictions++;
          evicted = std::move(g_wl_cache[pick]);
          evicted_stream_alive = pick_alive;
          g_wl_cache.erase(g_wl_cache.begin() + pick);
        }
        s = std::make_shared<WorklistSlot>();
        s->device = device;
        s->stream = stream;
        g_wl_cache.push_back(s);
      }
      s->last_use = ++g_wl_clock;
    }
    if (evicted) {
      wl_retire(evicted, evicted_stream_alive);
      (void)hipSetDevice(device);
    }
    hold.slot = s;
    hold.lk = std::unique_lock<std::mutex>(s->mu);
    if (s->retired) {  // evicted / forgotten between the look-up and the lock: look again (a fresh slot)
      hold.release();
      if (attempt < 4) continue;
      return inline_fallback();
    }
    bool drained = false;
    void* b = s->buf;
    // the two buffers grow independently, and a recompute-form call (need_rec = 0) leaves the record store alone: a
    // stream alternating hand-over batches with large ones keeps both
    const bool ok = wl_grow(stream, &b, &s->cap, need, &drained) &&
                    (!need_rec || wl_grow(stream, &s->rec, &s->rec_cap, need_rec, &drained));
    s->buf = (int*)b;
    if (!ok) {
      hold.release();
      return inline_fallback();  // no memory
    }
    *wl = s->buf;
    if (handover) *rec = s->rec;
    return 0;
  }
}

}  // namespace

extern "C" int abrk_scratch_stats(int device, abrk_scratch_info* out) {
  if (!out) return fail(ABRK_EINVAL, "out is NULL");
  memset(out, 0, sizeof *out);
  {
    std::lock_guard<std::mutex> lk(g_wl_mu);
    out->worklist_slots = (int64_t)g_wl_cache.size();
    for (auto& e : g_wl_cache) out->worklist_bytes += (int64_t)(e->cap + e->rec_cap);  // (racy read of sizes: diagnostics)
  }
  out->inline_fallbacks = g_wl_inline_fallbacks.load();
  out->evictions = g_wl_evictions.load();
  status_pool_stats(&out->status_words_out, &out->status_blocks);
  if (int rc = use_device(device)) return rc;
  size_t fr = 0, tot = 0;
  HIPCHK(hipMemGetInfo(&fr, &tot));
  out->device_free_bytes = (int64_t)fr;
  out->device_total_bytes = (int64_t)tot;
  return 0;
}

// ------------------------------------------------------------------------------- OSC
ArrayTable host::osc_arrays(int n, bool ki, uint32_t want) {
  ArrayTable t;
  t.add("q", n, kRead);
  t.add("dq", n, kRead);
  t.add("target", 6, kRead);
  t.add("target_velocity", 6, kRead);
  t.add("integrated_error", 6, kRead | kWritten, ki);
  t.add("u_null_ext", n, kRead);
  t.add("u", n, kWritten);
  t.add("training_signal", n, kWritten);
  if (want) add_dyn_outputs(t, n, want, 6);  // the fused outputs: Tx, J, M, g, C, dJ
  return t;
}

extern "C" int abrk_osc_generate_batch(int arm_id, int dtype, const abrk_osc_params* P, int64_t B, const void* q,
                                       const void* dq, const void* target, const void* target_velocity,
                                       void* integrated_error, const void* u_null_ext, void* u,
                                       void* training_signal, int device, void* stream) {
  void* const arr[] = {(void*)q, (void*)dq, (void*)target, (void*)target_velocity, integrated_error, (void*)u_null_ext,
                       u, training_signal};
  return osc_call(arm_id, dtype, P, B, arr, 0, device, stream, nullptr);
}

extern "C" int abrk_osc_generate_full_batch(int arm_id, int dtype, const abrk_osc_params* P, int64_t B, const void* q,
                                            const void* dq, const void* target, const void* target_velocity,
                                            void* integrated_error, const void* u_null_ext, void* u,
                                            void* training_signal, uint32_t want, const abrk_dyn_out* out, int device,
                                            void* stream) {
  const uint32_t ok = ABRK_WANT_TX | ABRK_WANT_J | ABRK_WANT_M | ABRK_WANT_G | ABRK_WANT_C | ABRK_WANT_DJ;
  if (!want || (want & ~ok))
    return fail(ABRK_EINVAL, "want must be a non-empty subset of Tx | J | M | g | C | dJ (0x%x)", want);
  if (!out) return fail(ABRK_EINVAL, "out is NULL");
  void* const arr[] = {(void*)q, (void*)dq, (void*)target, (void*)target_velocity, integrated_error, (void*)u_null_ext,
                       u, training_signal, out->Tx, out->J, out->M, out->g, out->C, out->dJ};
  return osc_call(arm_id, dtype, P, B, arr, want, device, stream, nullptr);
}

// want == 0: arr may hold the law's eight arrays alone (the pointer of an array the call does not use is never read)
int host::osc_call(int arm_id, int dtype, const abrk_osc_params* P, int64_t B, void* const* arr, uint32_t want,
                   int device, void* stream, StatusWord* word) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  const int n = a->desc.n_joints;
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  if (P->ref_frame < 0 || P->ref_frame > 2 * n + 1)
    return fail(ABRK_EFRAME, "Invalid transformation name: frame id %d", P->ref_frame);
  if (P->n_null < 0 || P->n_null > ABRK_MAX_NULL) return fail(ABRK_EINVAL, "n_null=%d outside 0..%d", P->n_null, ABRK_MAX_NULL);
  for (int c = 0; c < P->n_null; c++)
    if (P->null_ctrl[c].kind != ABRK_NULL_DAMPING && P->null_ctrl[c].kind != ABRK_NULL_RESTING)
      return fail(ABRK_EINVAL, "null controller %d has unknown kind %d", c, P->null_ctrl[c].kind);
  if (P->orientation_algorithm != 0 && P->orientation_algorithm != 1)
    return fail(ABRK_EINVAL, "Invalid algorithm number %d for calculating orientation error", P->orientation_algorithm);
  int k = 0;
  for (int r = 0; r < 6; r++) k += P->ctrlr_dof[r] ? 1 : 0;
  if (k == 0) return fail(ABRK_EINVAL, "ctrlr_dof selects no task-space dimension");
  if (!arr[0] || !arr[1] || !arr[2] || !arr[6]) return fail(ABRK_EINVAL, "q, dq, target and u are required");
  if (P->ki != 0 && !arr[4]) return fail(ABRK_EINVAL, "ki != 0 needs the integrated_error state array");
  for (int i = 0; i < 6; i++)
    if ((want >> i & 1) && !arr[8 + i]) return fail(ABRK_EINVAL, "output %d requested but its pointer is NULL", i);
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  Stager st{device, (hipStream_t)stream};
  OscArgs oa;
  void** fields[14] = {(void**)&oa.q, (void**)&oa.dq, (void**)&oa.target, (void**)&oa.tv, &oa.ierr, (void**)&oa.une, &oa.u, &oa.ts};
  for (int i = 0; i < 6; i++) fields[8 + i] = &oa.out[i];
  st.bind_table(osc_arrays(n, P->ki != 0, want), arr, fields, B, esz(dtype));
  if (int rc = st.reserve()) return rc;
  const bool u_null_ext = arr[5] != nullptr;
  oa.want = want;
  oa.use_C = P->use_C ? 1 : 0;
  oa.fast = osc_fast_rows(*P, n, u_null_ext);
  WlHold wl_hold;  // the (device, stream) worklist stays ours until the launches are enqueued
  Osc6Plan plan;
  if (oa.fast == 0 && !want) {
    plan = osc6_plan((long)B, osc6_switches());
    if (plan.form != Osc6Form::OnePass)
      if (int rc = worklist_for(device, (hipStream_t)stream, B, n, dtype, plan, &oa.wl, &oa.rec, wl_hold)) return rc;
  }
  oa.form = plan.form;
  auto pb = blocks([&](auto t) { return make_oscp<decltype(t)>(*P, n); });
  const ArmOps* ops = a->ops;
  const hipStream_t hs = (hipStream_t)stream;
  // hand-over forms: the arm's first pass, then the arm-independent finish kernel on the records it left
  const FinishArgs fa{plan, oa.wl, oa.rec, (P->n_null > 0 || u_null_ext) ? 1 : 0, oa.u, oa.ts};
  return with_status_word(st, pb, word, [&] {
    return dispatch(st, a, dtype, [=](const void* rt) {
      OscArgs o = oa;
      o.P = pb.of(dtype);
      const LaunchArgs la{rt, (long)B, hs};
      const hipError_t e = ops->osc(dtype, la, o);
      if (e != hipSuccess || !fa.plan.uses_records()) return e;
      return launch_osc6_finish(n, dtype, la, fa);
    }, &wl_hold);
  });
}

// ------------------------------------------------------------------------------- OSC, wave-cooperative mapping
namespace abrk {
hipError_t launch_osc_coop_ur5(const LaunchArgs& la, const CoopArgs& a);
}
extern "C" int abrk_osc_generate_coop_batch(int arm_id, int dtype, const abrk_osc_params* P, int64_t B, const void* q,
                                            const void* dq, const void* target, void* u, void* training_signal,
                                            int lanes_per_arm, int device, void* stream) {
  ArmEntry* a;
  if (int rc = check_common(arm_id, dtype, B, &a)) return rc;
  const int n = a->desc.n_joints;
  if (!(a->builtin && strcmp(a->desc.name, "ur5") == 0) || dtype != ABRK_F64)
    return fail(ABRK_EINVAL, "the wave-cooperative kernels are built for the built-in ur5 arm in fp64 (measurement variant)");
  if (lanes_per_arm != 4 && lanes_per_arm != 8 && lanes_per_arm != 16)
    return fail(ABRK_EINVAL, "lanes_per_arm must be 4, 8 or 16");
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  if (osc_fast_rows(*P, n, false) != 3 || P->n_null != 0 || P->use_C || P->ki != 0 || P->xyz_offset[0] != 0 ||
      P->xyz_offset[1] != 0 || P->xyz_offset[2] != 0)
    return fail(ABRK_EINVAL, "the wave-cooperative kernels cover the plain law: x,y,z of the EE, no offset, no null "
                             "controllers, no Coriolis term, ki = 0");
  if (!q || !dq || !target || !u) return fail(ABRK_EINVAL, "q, dq, target and u are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  CoopArgs ca;
  ca.P = nullptr;
  ca.lanes = lanes_per_arm;
  st.in(&ca.q, q, B * n * s);
  st.in(&ca.dq, dq, B * n * s);
  st.in(&ca.target, target, B * 6 * s);
  st.out(&ca.u, u, B * n * s);
  st.out(&ca.ts, training_signal, B * n * s);
  if (int rc = st.reserve()) return rc;
  const OscP<double> p64 = make_oscp<double>(*P, n);
  const hipStream_t hs = (hipStream_t)stream;
  return dispatch(st, a, dtype, [=](const void*) {
    CoopArgs o = ca;
    o.P = &p64;
    return launch_osc_coop_ur5(LaunchArgs{nullptr, (long)B, hs}, o);
  });
}

// ------------------------------------------------------------------------------- OSC law on supplied dynamics
extern "C" int abrk_osc_law_batch(int n_joints, int dtype, const abrk_osc_params* P, int64_t B, const void* J,
                                  const void* M, const void* g, const void* Cdq, const void* xyz, const void* R,
                                  const void* q, const void* dq, const void* target, const void* target_velocity,
                                  void* integrated_error, const void* u_null_ext, void* u, void* training_signal,
                                  int device, void* stream) {
  const int n = n_joints;
  if (int rc = check_joints(n)) return rc;
  if (int rc = check_batch(dtype, B)) return rc;
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  if (P->n_null < 0 || P->n_null > ABRK_MAX_NULL) return fail(ABRK_EINVAL, "n_null=%d outside 0..%d", P->n_null, ABRK_MAX_NULL);
  if (P->orientation_algorithm != 0 && P->orientation_algorithm != 1)
    return fail(ABRK_EINVAL, "Invalid algorithm number %d for calculating orientation error", P->orientation_algorithm);
  int k = 0, pos = 0, ori = 0;
  for (int r = 0; r < 6; r++) {
    k += P->ctrlr_dof[r] ? 1 : 0;
    (r < 3 ? pos : ori) += P->ctrlr_dof[r] ? 1 : 0;
  }
  if (k == 0) return fail(ABRK_EINVAL, "ctrlr_dof selects no task-space dimension");
  if (!J || !M || !dq || !target || !u) return fail(ABRK_EINVAL, "J, M, dq, target and u are required");
  if (pos && !xyz) return fail(ABRK_EINVAL, "position control needs xyz (robot_config.Tx)");
  if (ori && !R) return fail(ABRK_EINVAL, "orientation control needs R (robot_config.R)");
  if (P->use_g && !g) return fail(ABRK_EINVAL, "use_g needs g (robot_config.g)");
  if (P->use_C && !Cdq) return fail(ABRK_EINVAL, "use_C needs Cdq (robot_config.C(q,dq) @ dq)");
  if (P->ki != 0 && !integrated_error) return fail(ABRK_EINVAL, "ki != 0 needs the integrated_error state array");
  for (int c = 0; c < P->n_null; c++)
    if (P->null_ctrl[c].kind == ABRK_NULL_RESTING && !q) return fail(ABRK_EINVAL, "RestingConfig needs q");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  LawArgs a{};
  st.in(&a.J, J, B * 6 * n * s);
  st.in(&a.M, M, B * n * n * s);
  st.in(&a.g, P->use_g ? g : nullptr, B * n * s);
  st.in(&a.c, P->use_C ? Cdq : nullptr, B * n * s);
  st.in(&a.xyz, xyz, B * 3 * s);
  st.in(&a.R, R, B * 9 * s);
  st.in(&a.q, q, B * n * s);
  st.in(&a.dq, dq, B * n * s);
  st.in(&a.target, target, B * 6 * s);
  st.in(&a.tv, target_velocity, B * 6 * s);
  st.inout(&a.ierr, P->ki != 0 ? integrated_error : nullptr, B * 6 * s);
  st.in(&a.une, u_null_ext, B * n * s);
  st.out(&a.u, u, B * n * s);
  st.out(&a.ts, training_signal, B * n * s);
  if (int rc = st.reserve()) return rc;
  auto pb = blocks([&](auto t) { return make_oscp<decltype(t)>(*P, n); });
  const hipStream_t hs = (hipStream_t)stream;
  return with_status_word(st, pb, nullptr, [&] {
    return dispatch(st, nullptr, dtype, [=](const void*) {
      LawArgs o = a;
      o.P = pb.of(dtype);
      return launch_osc_law(n, dtype, LaunchArgs{nullptr, (long)B, hs}, o);
    });
  });
}

// ------------------------------------------------------------------------------- helper methods of OSC
extern "C" int abrk_osc_mx_batch(int n_joints, int k, int dtype, int64_t B, const void* M, const void* J,
                                 double threshold, void* Mx, void* M_inv, int device, void* stream) {
  const int n = n_joints;
  if (int rc = check_joints(n)) return rc;
  if (k < 1 || k > 6) return fail(ABRK_EINVAL, "k=%d task rows outside 1..6", k);
  if (int rc = check_helper(dtype, B)) return rc;
  if (!M || !J || !Mx) return fail(ABRK_EINVAL, "M, J and Mx are required");
  if (!(threshold >= 0)) return fail(ABRK_EINVAL, "threshold must be >= 0");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  const void *Md, *Jd;
  void *Xd, *Id;
  st.in(&Md, M, B * n * n * s);
  st.in(&Jd, J, B * k * n * s);
  st.out(&Xd, Mx, B * k * k * s);
  st.out(&Id, M_inv, B * n * n * s);
  if (int rc = st.reserve()) return rc;
  LaunchArgs la{nullptr, (long)B, (hipStream_t)stream};
  HIPCHK(launch_osc_mx(n, dtype, la, k, threshold, Md, Jd, Xd, Id));
  return st.finish();
}

extern "C" int abrk_osc_velocity_limiting_batch(int dtype, const abrk_osc_params* P, int64_t B, const void* u_task,
                                                void* out, int device, void* stream) {
  if (int rc = check_helper(dtype, B)) return rc;
  if (!P) return fail(ABRK_EINVAL, "params is NULL");
  if (!P->use_vmax) return fail(ABRK_EINVAL, "velocity limiting needs vmax (OSC(vmax=[xyz, abg]))");
  if (!u_task || !out) return fail(ABRK_EINVAL, "u_task and out are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  const void* id;
  void* od;
  st.in(&id, u_task, B * 6 * s);
  st.out(&od, out, B * 6 * s);
  if (int rc = st.reserve()) return rc;
  LaunchArgs la{nullptr, (long)B, (hipStream_t)stream};
  const double g[5] = {P->kp, P->ko, P->kv, P->vmax[0], P->vmax[1]};
  HIPCHK(launch_velocity_limiting(dtype, la, g, id, od));
  return st.finish();
}

extern "C" int abrk_osc_orientation_forces_batch(int algorithm, int dtype, int64_t B, const void* R,
                                                 const void* target_abg, void* u_task_orientation, int device,
                                                 void* stream) {
  if (int rc = check_helper(dtype, B)) return rc;
  if (algorithm != 0 && algorithm != 1)
    return fail(ABRK_EINVAL, "Invalid algorithm number %d for calculating orientation error", algorithm);
  if (!R || !target_abg || !u_task_orientation) return fail(ABRK_EINVAL, "R, target_abg and the output are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  const void *Rd, *ad;
  void* od;
  st.in(&Rd, R, B * 9 * s);
  st.in(&ad, target_abg, B * 3 * s);
  st.out(&od, u_task_orientation, B * 3 * s);
  if (int rc = st.reserve()) return rc;
  LaunchArgs la{nullptr, (long)B, (hipStream_t)stream};
  HIPCHK(launch_orientation_forces(dtype, la, algorithm, Rd, ad, od));
  return st.finish();
}

extern "C" int abrk_transformations_batch(int op, int dtype, int64_t B, const void* a, const void* b, void* out,
                                          int device, void* stream) {
  // elements per row of (a, b, out) for each ABRK_TF_* operation
  static const int kIn[8] = {3, 3, 9, 4, 4, 4, 3, 3}, kIn2[8] = {0, 0, 0, 4, 0, 0, 0, 0}, kOut[8] = {4, 4, 4, 4, 4, 4, 3, 9};
  if (op < 0 || op > 7) return fail(ABRK_EINVAL, "unknown transformations op %d", op);
  if (int rc = check_helper(dtype, B)) return rc;
  if (!a || !out || (kIn2[op] && !b)) return fail(ABRK_EINVAL, "input and output arrays are required");
  if (B == 0) return 0;
  if (int rc = use_device(device)) return rc;
  const size_t s = esz(dtype);
  Stager st{device, (hipStream_t)stream};
  const void *ad, *bd;
  void* od;
  st.in(&ad, a, B * kIn[op] * s);
  st.in(&bd, kIn2[op] ? b : nullptr, B * kIn2[op] * s);
  st.out(&od, out, B * kOut[op] * s);
  if (int rc = st.reserve()) return rc;
  LaunchArgs la{nullptr, (long)B, (hipStream_t)stream};
  HIPCHK(launch_transformations(dtype, la, op, ad, bd, od));
  return st.finish();
}

// ellgpu -- the extern "C" surface of include/ellgpu.h, written once over
// Engine<ELL_BACKEND>.  Included by capi.hip (ELL_BACKEND = HipBackend, the
// product) and by tests/hostsim/hostsim.cpp (ELL_BACKEND = LoopBackend, CPU
// unit-test build of the same code).  The including file must define
//   ELL_BACKEND            backend type
//   ell_backend_create(int device, ELL_BACKEND* out, std::string* err) -> int
//   ell_backend_destroy(ELL_BACKEND*)
//   ell_device_count() -> int
// before including this header.
#pragma once

#include "../include/ellgpu_edsum.h"
#include "engine.h"

#include <mutex>
#include <thread>
#include <vector>

// A context owns one engine on one device.  A GROUP (ellgpu_group_create) is a context whose
// `members` are ordinary contexts, one per listed device: the host-buffer scalar-multiplication
// and verify entry points cut a batch into contiguous shards, one host thread per member drives
// its device (its own streams, scratch arena and replicated tables), and every member copies its
// results straight into the caller's buffers -- no device-to-device traffic at all (SURVEY.md 8e:
// "a direct per-device D2H is the zero-collective alternative").  Any other entry point called on
// a group runs on member 0.
// `mu` serialises the entry points of ONE context: the staging buffers, the scratch arenas, the
// stream bookkeeping and `err` belong to the context, so two host threads inside it at once -- the
// N-API addon's libuv worker running a Promise-form batch while the JS thread makes a synchronous
// call -- would overwrite each other's staged inputs.  The second caller waits (host-buffer calls
// hold the lock until their results are back; *_dev calls only while they enqueue).  Recursive:
// an entry point may call another on the same context.  A group call locks the group, then every
// member from its worker thread.
struct ellgpu_ctx {
  ell::Engine<ELL_BACKEND>* eng;
  std::vector<ellgpu_ctx*> members;
  std::recursive_mutex mu;
  int deferred_rc = 0;             // status of a deferred call that something else completed
  std::string deferred_msg;
};

// (entering a context also completes a call that ellgpu_ctx_defer left in flight: its results sit
// in the context's one pinned buffer, which the next small call would overwrite)
static void ell_complete_deferred(ellgpu_ctx* ctx) {
  if (!ctx->members.empty() || !ctx->eng || !ctx->eng->defer_pending()) return;
  const int rc = ctx->eng->defer_collect();
  if (rc && !ctx->deferred_rc) { ctx->deferred_rc = rc; ctx->deferred_msg = ctx->eng->err; }
  ctx->eng->bk.end_call(false);
}
// the context's lock for the rest of the scope, taken with the pending call completed
struct EllLock {
  std::lock_guard<std::recursive_mutex> g;
  explicit EllLock(ellgpu_ctx* ctx) : g(ctx->mu) { ell_complete_deferred(ctx); }
};
#define ELL_LOCK(ctx) EllLock ell_ctx_lock_(ctx)

static thread_local std::string g_last_error;

static int set_err(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
// end of every entry point.  `stream_call` = a *_dev entry point: it returns without
// synchronising, so the backend records where its work ends (see HipBackend::use_stream).
static int finish(ellgpu_ctx* ctx, int rc, bool stream_call = false) {
  ctx->eng->bk.end_call(stream_call);
  if (rc) g_last_error = ctx->eng->err.empty() ? "ellgpu error" : ctx->eng->err;
  return rc;
}

extern "C" {

int ellgpu_version(void) { return ELLGPU_VERSION; }
#ifndef ELLGPU_SOURCE_DIGEST
#define ELLGPU_SOURCE_DIGEST "unstamped"
#endif
const char* ellgpu_source_digest(void) { return ELLGPU_SOURCE_DIGEST; }
const char* ellgpu_last_error(void) { return g_last_error.c_str(); }

int ellgpu_curve_id(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < ell::CURVE_COUNT; i++)
    if (strcmp(name, ell::curve_info(i)->name) == 0) return i;
  return -1;
}
int ellgpu_curve_field_bytes(int curve) {
  const ell::CurveInfo* ci = ell::curve_info(curve);
  return ci ? ci->field_bytes : ELLGPU_E_ARG;
}
int ellgpu_curve_order_bytes(int curve) {
  const ell::CurveInfo* ci = ell::curve_info(curve);
  return ci ? ci->order_bytes : ELLGPU_E_ARG;
}
int ellgpu_device_count(void) { return ell_device_count(); }

int ellgpu_ctx_create(int device, ellgpu_ctx** out) {
  if (!out) return set_err(ELLGPU_E_ARG, "null out pointer");
  *out = nullptr;
  ELL_BACKEND bk;
  std::string err;
  int rc = ell_backend_create(device, &bk, &err);
  if (rc) return set_err(rc, err);
  ellgpu_ctx* c = new ellgpu_ctx;
  c->eng = new ell::Engine<ELL_BACKEND>(bk);
  *out = c;
  return ELLGPU_OK;
}
int ellgpu_group_create(const int* devices, int ndev, ellgpu_ctx** out) {
  if (!out) return set_err(ELLGPU_E_ARG, "null out pointer");
  *out = nullptr;
  if (!devices || ndev < 1 || ndev > 64) return set_err(ELLGPU_E_ARG, "ellgpu_group_create: 1..64 devices");
  ellgpu_ctx* g = new ellgpu_ctx;
  g->eng = nullptr;
  for (int i = 0; i < ndev; i++) {
    ellgpu_ctx* m = nullptr;
    int rc = ellgpu_ctx_create(devices[i], &m);
    if (rc) {
      for (ellgpu_ctx* x : g->members) ellgpu_ctx_destroy(x);
      delete g;
      return rc;                                    // message already set by ellgpu_ctx_create
    }
    g->members.push_back(m);
  }
  g->eng = g->members[0]->eng;                      // borrowed: entry points without a sharded form
  *out = g;
  return ELLGPU_OK;
}
int ellgpu_group_size(const ellgpu_ctx* ctx) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  return ctx->members.empty() ? 1 : (int)ctx->members.size();
}
}  // extern "C"
// run f(member, lo, hi) for the contiguous shard of every member on its own host thread
template <class Fn>
static int group_shard(ellgpu_ctx* g, size_t n, Fn f) {
  const size_t m = g->members.size();
  std::vector<int> rc(m, 0);
  std::vector<std::string> msg(m);
  std::vector<std::thread> th;
  for (size_t i = 0; i < m; i++) {
    const size_t lo = n * i / m, hi = n * (i + 1) / m;
    th.emplace_back([&, i, lo, hi]() {
      rc[i] = lo < hi ? f(g->members[i], lo, hi) : 0;
      if (rc[i]) msg[i] = g_last_error;             // the worker's thread-local message
    });
  }
  for (auto& t : th) t.join();
  for (size_t i = 0; i < m; i++)
    if (rc[i]) return set_err(rc[i], "device shard " + std::to_string(i) + ": " + msg[i]);
  return ELLGPU_OK;
}
extern "C" {

void ellgpu_ctx_destroy(ellgpu_ctx* ctx) {
  if (!ctx) return;
  if (!ctx->members.empty()) {
    for (ellgpu_ctx* m : ctx->members) ellgpu_ctx_destroy(m);
    delete ctx;
    return;
  }
  ctx->eng->bk.sync();
  ELL_BACKEND bk = ctx->eng->bk;
  delete ctx->eng;
  ell_backend_destroy(&bk);
  delete ctx;
}
int ellgpu_ctx_synchronize(ellgpu_ctx* ctx) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  ELL_LOCK(ctx);
  if (!ctx->members.empty()) {                       // a group: every member's device
    for (ellgpu_ctx* m : ctx->members) {
      int rc = ellgpu_ctx_synchronize(m);
      if (rc) return rc;
    }
    return ELLGPU_OK;
  }
  return finish(ctx, ctx->eng->bk.sync());
}
void* ellgpu_ctx_stream(ellgpu_ctx* ctx) {
  if (!ctx) return nullptr;
  ELL_LOCK(ctx);
  return ctx->eng->bk.own_stream();
}
int ellgpu_ctx_defer(ellgpu_ctx* ctx) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  ELL_LOCK(ctx);
  if (ctx->members.empty()) ctx->eng->defer_arm();          // (a group's calls are never deferred)
  return ELLGPU_OK;
}
int ellgpu_ctx_collect(ellgpu_ctx* ctx) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  ELL_LOCK(ctx);                                             // completes the pending call, if any
  if (ctx->members.empty()) ctx->eng->defer_collect();       // disarms
  const int rc = ctx->deferred_rc;
  ctx->deferred_rc = 0;
  if (rc) return set_err(rc, ctx->deferred_msg.empty() ? "device error in a deferred call" : ctx->deferred_msg);
  return ELLGPU_OK;
}
int ellgpu_ctx_reserve(ellgpu_ctx* ctx, int curve, size_t n) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  ELL_LOCK(ctx);
  if (!ctx->members.empty()) {
    // a group: every member gets its shard's worth (tables and scratch are per device), so that
    // the first sharded call does not allocate and build tables inside its worker threads
    const size_t m = ctx->members.size();
    return group_shard(ctx, m, [=](ellgpu_ctx* mem, size_t lo, size_t) {
      return ellgpu_ctx_reserve(mem, curve, (n * (lo + 1) / m) - (n * lo / m));
    });
  }
  ctx->eng->bk.use_stream(nullptr);
  return finish(ctx, ctx->eng->reserve(curve, n));
}

int ellgpu_ctx_comb_bits(ellgpu_ctx* ctx, int curve) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  if (curve < 0 || curve >= ell::CURVE_COUNT) return set_err(ELLGPU_E_ARG, "unknown curve id");
  ELL_LOCK(ctx);
  return ctx->eng->comb_bits(curve);
}

// edwards: 0 short, 1 Edwards, 2 Montgomery (b unused); dom: n, gx, gy of an ECDSA domain (edwards = 0 or 1), else null
static int define_custom(ellgpu_ctx* ctx, int edwards, const uint8_t* p, const uint8_t* a, const uint8_t* b,
                         int* out_curve, const uint8_t* const* dom = nullptr) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  ELL_LOCK(ctx);
  if (!ctx->members.empty()) {
    // all or nothing: a member that cannot take the curve (table full), or would give it another
    // id than member 0 (curves were defined on a member directly), is found BEFORE anything is
    // registered -- the engine dedups identical parameters, so the probe is the definition's own
    // first half (Engine::custom_slot_for)
    int id = -1;
    for (size_t i = 0; i < ctx->members.size(); i++) {
      int mid = ctx->members[i]->eng->custom_slot_for(edwards, p, a, b, dom);
      if (mid < 0) return set_err(ELLGPU_E_UNSUPPORTED, "user-defined curve table of a group member is full");
      if (i && mid != id) return set_err(ELLGPU_E_ARG, "group members disagree on the curve id (curves were defined on a member directly)");
      id = mid;
    }
    for (size_t i = 0; i < ctx->members.size(); i++) {
      int mid = -1;
      int rc = define_custom(ctx->members[i], edwards, p, a, b, &mid, dom);
      if (rc) return rc;                             // (parameter errors are the same on every member: member 0 fails first)
    }
    if (out_curve) *out_curve = id;
    return ELLGPU_OK;
  }
  ctx->eng->err.clear();
  int rc = dom ? (edwards ? ctx->eng->define_edwards_domain(p, a, b, dom[0], dom[1], dom[2], out_curve)
                          : ctx->eng->define_short_domain(p, a, b, dom[0], dom[1], dom[2], out_curve))
               : edwards == 2 ? ctx->eng->define_mont(p, a, out_curve)
               : edwards ? ctx->eng->define_edwards(p, a, b, out_curve) : ctx->eng->define_short(p, a, b, out_curve);
  if (rc) g_last_error = ctx->eng->err.empty() ? "ellgpu error" : ctx->eng->err;
  return rc;
}
int ellgpu_curve_define_short(ellgpu_ctx* ctx, const uint8_t* p, const uint8_t* a, const uint8_t* b,
                              int* out_curve) {
  return define_custom(ctx, 0, p, a, b, out_curve);
}
int ellgpu_curve_define_edwards(ellgpu_ctx* ctx, const uint8_t* p, const uint8_t* a, const uint8_t* d,
                                int* out_curve) {
  return define_custom(ctx, 1, p, a, d, out_curve);
}
int ellgpu_curve_define_mont(ellgpu_ctx* ctx, const uint8_t* p, const uint8_t* a, int* out_curve) {
  return define_custom(ctx, 2, p, a, nullptr, out_curve);
}
int ellgpu_curve_define_short_domain(ellgpu_ctx* ctx, const uint8_t* p, const uint8_t* a, const uint8_t* b,
                                     const uint8_t* n, const uint8_t* gx, const uint8_t* gy, int* out_curve) {
  const uint8_t* dom[3] = {n, gx, gy};
  if (!n || !gx || !gy) return set_err(ELLGPU_E_ARG, "null pointer");
  return define_custom(ctx, 0, p, a, b, out_curve, dom);
}
int ellgpu_curve_define_edwards_domain(ellgpu_ctx* ctx, const uint8_t* p, const uint8_t* a, const uint8_t* d,
                                       const uint8_t* n, const uint8_t* gx, const uint8_t* gy, int* out_curve) {
  const uint8_t* dom[3] = {n, gx, gy};
  if (!n || !gx || !gy) return set_err(ELLGPU_E_ARG, "null pointer");
  return define_custom(ctx, 1, p, a, d, out_curve, dom);
}

}  // extern "C"

// Every batch entry point is ell_call() around one Engine operation: ellgpu_X passes Mem::host (the
// operands are host buffers; the call returns with its results back), ellgpu_X_dev Mem::device and
// the caller's stream (device pointers; the call returns as soon as its work is enqueued, and works
// in the scratch arena of its stream, HipBackend::use_stream_dev).  `op` gets the engine and `where`.
typedef ell::Engine<ELL_BACKEND> Eng;
using ell::Mem;
// (the start of a call, under the context's lock: the white-box probes of capi.hip use it alone)
static void ell_enter(Eng& e, void* stream, Mem where) {
  e.err.clear();
  if (where == Mem::host) {
    e.bk.use_stream(stream);
    e.set_lane(0);
  } else {
    e.set_lane(e.bk.use_stream_dev(stream));
  }
}
template <class Op>
static int ell_call(ellgpu_ctx* ctx, void* stream, Mem where, Op op) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  ELL_LOCK(ctx);
  ell_enter(*ctx->eng, stream, where);
  return finish(ctx, op(*ctx->eng, where), where == Mem::device);
}

extern "C" {

// byte widths of a curve's field elements and scalars (for slicing the flat buffers of a group call)
static int curve_widths(int curve, size_t& B, size_t& NB) {
  const ell::CurveInfo* ci = ell::curve_info(curve);
  if (!ci) return set_err(ELLGPU_E_ARG, "unknown curve id");
  B = (size_t)ci->field_bytes;
  NB = (size_t)ci->order_bytes;
  return 0;
}

int ellgpu_mul_fixed(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* k, uint8_t* out_xy,
                     uint8_t* out_inf) {
  if (ctx && !ctx->members.empty()) {
    ELL_LOCK(ctx);
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    if (n && (!k || !out_xy)) return set_err(ELLGPU_E_ARG, "null buffer");
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_mul_fixed(m, curve, hi - lo, k + lo * B, out_xy + lo * 2 * B, out_inf ? out_inf + lo : nullptr);
    });
  }
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.mul_fixed(w, curve, n, k, out_xy, out_inf); });
}
int ellgpu_mul_fixed_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* k, uint8_t* out_xy,
                         uint8_t* out_inf, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.mul_fixed(w, curve, n, k, out_xy, out_inf); });
}

// ---- fixed-base tables of caller-chosen points (Engine::define_base) ----
// (ed: ellgpu_ed_base_define, the Edwards curves' entry point -- the same handles, the same path)
static int base_define(ellgpu_ctx* ctx, int curve, const uint8_t* xy, int window_bits, int* out_base, bool ed) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  ELL_LOCK(ctx);
  if (!ctx->members.empty()) {
    // all or nothing, with one handle: what the members built before one of them refused is
    // released again (never a base that existed before this call)
    if (!out_base) return set_err(ELLGPU_E_ARG, "null pointer");
    std::vector<int> made(ctx->members.size(), -1);
    int id = -1, rc = ELLGPU_OK;
    std::string msg;
    for (size_t i = 0; i < ctx->members.size() && rc == ELLGPU_OK; i++) {
      ellgpu_ctx* m = ctx->members[i];
      std::lock_guard<std::recursive_mutex> g(m->mu);
      ell_enter(*m->eng, nullptr, Mem::host);
      int h = -1;
      bool created = false;
      rc = finish(m, m->eng->define_base(curve, xy, window_bits, &h, &created, ed));
      if (rc) { msg = g_last_error; break; }
      if (created) made[i] = h;
      if (i && h != id) { rc = ELLGPU_E_ARG; msg = "group members disagree on the base handle (bases were defined on a member directly)"; }
      id = h;
    }
    if (rc) {
      for (size_t i = 0; i < ctx->members.size(); i++)
        if (made[i] >= 0) {
          ellgpu_ctx* m = ctx->members[i];
          std::lock_guard<std::recursive_mutex> g(m->mu);
          ell_enter(*m->eng, nullptr, Mem::host);
          finish(m, m->eng->release_base(made[i], true));     // never issued: the member's counter goes back
        }
      return set_err(rc, msg);
    }
    *out_base = id;
    return ELLGPU_OK;
  }
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem) { return e.define_base(curve, xy, window_bits, out_base, nullptr, ed); });
}
int ellgpu_base_define(ellgpu_ctx* ctx, int curve, const uint8_t* xy, int window_bits, int* out_base) {
  return base_define(ctx, curve, xy, window_bits, out_base, false);
}
int ellgpu_ed_base_define(ellgpu_ctx* ctx, int curve, const uint8_t* xy, int window_bits, int* out_base) {
  return base_define(ctx, curve, xy, window_bits, out_base, true);
}
int ellgpu_base_release(ellgpu_ctx* ctx, int base) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  if (!ctx->members.empty()) {
    ELL_LOCK(ctx);
    int rc = ELLGPU_OK;
    for (ellgpu_ctx* m : ctx->members) {
      const int r = ellgpu_base_release(m, base);
      if (r && !rc) rc = r;
    }
    return rc;
  }
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem) { return e.release_base(base); });
}
int ellgpu_base_info(ellgpu_ctx* ctx, int base, int* out_curve, int* out_window_bits, uint64_t* out_table_bytes) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem) {
    ell::u64 bytes = 0;
    const int rc = e.base_info(base, out_curve, out_window_bits, &bytes);
    if (rc == ELLGPU_OK && out_table_bytes) *out_table_bytes = (uint64_t)bytes;
    return rc;
  });
}
// `mem` / `stream` of the calls that have one form: -> where the operands live, or a refusal
static int mem_of(int mem, void* stream, Mem& where) {
  if (mem != ELLGPU_MEM_HOST && mem != ELLGPU_MEM_DEVICE) return set_err(ELLGPU_E_ARG, "mem: ELLGPU_MEM_HOST or ELLGPU_MEM_DEVICE");
  if (mem == ELLGPU_MEM_HOST && stream) return set_err(ELLGPU_E_ARG, "a stream goes with ELLGPU_MEM_DEVICE: host memory takes NULL");
  where = mem == ELLGPU_MEM_HOST ? Mem::host : Mem::device;
  return ELLGPU_OK;
}
int ellgpu_mul_base(ellgpu_ctx* ctx, int base, size_t n, const uint8_t* k, uint8_t* out_xy, uint8_t* out_inf,
                    int mem, void* stream) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  Mem where;
  if (int rc = mem_of(mem, stream, where)) return rc;
  if (!ctx->members.empty() && where == Mem::host) {
    ELL_LOCK(ctx);
    int curve = -1;
    if (int rc = ellgpu_base_info(ctx, base, &curve, nullptr, nullptr)) return rc;
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    if (n && (!k || !out_xy || !out_inf)) return set_err(ELLGPU_E_ARG, "null pointer");
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_mul_base(m, base, hi - lo, k + lo * B, out_xy + lo * 2 * B, out_inf + lo, mem, nullptr);
    });
  }
  return ell_call(ctx, stream, where, [=](Eng& e, Mem w) { return e.mul_base(w, base, n, k, out_xy, out_inf); });
}
int ellgpu_mul_base2(ellgpu_ctx* ctx, int base1, int base2, size_t n, const uint8_t* k1, const uint8_t* k2,
                     uint8_t* out_xy, uint8_t* out_inf, int mem, void* stream) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  Mem where;
  if (int rc = mem_of(mem, stream, where)) return rc;
  if (!ctx->members.empty() && where == Mem::host) {
    ELL_LOCK(ctx);
    int c1 = -1, c2 = -1;
    if (int rc = ellgpu_base_info(ctx, base1, &c1, nullptr, nullptr)) return rc;
    if (int rc = ellgpu_base_info(ctx, base2, &c2, nullptr, nullptr)) return rc;
    if (c1 != c2) return set_err(ELLGPU_E_ARG, "the two bases are on different curves");
    size_t B, NB;
    if (curve_widths(c1, B, NB)) return ELLGPU_E_ARG;
    if (n && (!k1 || !k2 || !out_xy || !out_inf)) return set_err(ELLGPU_E_ARG, "null pointer");
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_mul_base2(m, base1, base2, hi - lo, k1 + lo * B, k2 + lo * B, out_xy + lo * 2 * B, out_inf + lo,
                              mem, nullptr);
    });
  }
  return ell_call(ctx, stream, where, [=](Eng& e, Mem w) { return e.mul_base2(w, base1, base2, n, k1, k2, out_xy, out_inf); });
}
int ellgpu_mul_var(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* k, const uint8_t* in_xy,
                   uint8_t* out_xy, uint8_t* out_inf) {
  if (ctx && !ctx->members.empty()) {
    ELL_LOCK(ctx);
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    if (n && (!k || !in_xy || !out_xy)) return set_err(ELLGPU_E_ARG, "null buffer");
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_mul_var(m, curve, hi - lo, k + lo * B, in_xy + lo * 2 * B, out_xy + lo * 2 * B,
                            out_inf ? out_inf + lo : nullptr);
    });
  }
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.mul_var(w, curve, n, k, in_xy, out_xy, out_inf); });
}
int ellgpu_mul_var_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* k,
                       const uint8_t* in_xy, uint8_t* out_xy, uint8_t* out_inf, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.mul_var(w, curve, n, k, in_xy, out_xy, out_inf); });
}
int ellgpu_mul_add2(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* k1, const uint8_t* p1_xy,
                    const uint8_t* k2, const uint8_t* p2_xy, uint8_t* out_xy, uint8_t* out_inf) {
  if (ctx && !ctx->members.empty()) {
    ELL_LOCK(ctx);
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    if (n && (!k1 || !k2 || !p2_xy || !out_xy)) return set_err(ELLGPU_E_ARG, "null buffer");
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_mul_add2(m, curve, hi - lo, k1 + lo * B, p1_xy ? p1_xy + lo * 2 * B : nullptr, k2 + lo * B,
                             p2_xy + lo * 2 * B, out_xy + lo * 2 * B, out_inf ? out_inf + lo : nullptr);
    });
  }
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.mul_add2(w, curve, n, k1, p1_xy, k2, p2_xy, out_xy, out_inf); });
}
int ellgpu_mul_add2_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* k1,
                        const uint8_t* p1_xy, const uint8_t* k2, const uint8_t* p2_xy,
                        uint8_t* out_xy, uint8_t* out_inf, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.mul_add2(w, curve, n, k1, p1_xy, k2, p2_xy, out_xy, out_inf); });
}
int ellgpu_ecdsa_verify(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                        int msg_bits, const uint8_t* r, const uint8_t* s, const uint8_t* pub_xy,
                        uint8_t* out_ok, uint8_t* out_status) {
  if (ctx && !ctx->members.empty()) {
    ELL_LOCK(ctx);
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    if (n && (!hash || !r || !s || !pub_xy || !out_ok)) return set_err(ELLGPU_E_ARG, "null buffer");
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_ecdsa_verify(m, curve, hi - lo, hash + lo * (size_t)hash_len, hash_len, msg_bits, r + lo * NB,
                                 s + lo * NB, pub_xy + lo * 2 * B, out_ok + lo,
                                 out_status ? out_status + lo : nullptr);
    });
  }
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.ecdsa_verify(w, curve, n, hash, hash_len, msg_bits, r, s, pub_xy, out_ok, out_status); });
}
int ellgpu_ecdsa_verify_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash,
                            int hash_len, int msg_bits, const uint8_t* r, const uint8_t* s,
                            const uint8_t* pub_xy, uint8_t* out_ok, uint8_t* out_status,
                            void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.ecdsa_verify(w, curve, n, hash, hash_len, msg_bits, r, s, pub_xy, out_ok, out_status); });
}
// EC#verify against the table of the signer's key (include/ellgpu_ext2.h): one form, `mem` says
// where the operands live; a group shards a host batch as ellgpu_mul_base2's
int ellgpu_ecdsa_verify_base(ellgpu_ctx* ctx, int base, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                             const uint8_t* r, const uint8_t* s, uint8_t* out_ok, int mem, void* stream) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  Mem where;
  if (int rc = mem_of(mem, stream, where)) return rc;
  if (!ctx->members.empty() && where == Mem::host) {
    ELL_LOCK(ctx);
    int curve = -1;
    if (int rc = ellgpu_base_info(ctx, base, &curve, nullptr, nullptr)) return rc;
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    if (n && (!hash || !r || !s || !out_ok)) return set_err(ELLGPU_E_ARG, "null pointer");
    if (n && hash_len <= 0) return set_err(ELLGPU_E_ARG, "bad hash_len");
    if (!n) return ellgpu_ecdsa_verify_base(ctx->members[0], base, 0, hash, hash_len, msg_bits, r, s, out_ok, mem, nullptr);
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_ecdsa_verify_base(m, base, hi - lo, hash + lo * (size_t)hash_len, hash_len, msg_bits, r + lo * NB,
                                      s + lo * NB, out_ok + lo, mem, nullptr);
    });
  }
  return ell_call(ctx, stream, where, [=](Eng& e, Mem w) { return e.ecdsa_verify_base(w, base, n, hash, hash_len, msg_bits, r, s, out_ok); });
}
int ellgpu_x25519_ladder(ellgpu_ctx* ctx, size_t n, const uint8_t* k, const uint8_t* in_x,
                         uint8_t* out_x, uint8_t* out_inf) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.x25519(w, n, k, in_x, out_x, out_inf); });
}
int ellgpu_x25519_ladder_dev(ellgpu_ctx* ctx, size_t n, const uint8_t* k, const uint8_t* in_x,
                             uint8_t* out_x, uint8_t* out_inf, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.x25519(w, n, k, in_x, out_x, out_inf); });
}

int ellgpu_x25519_derive(ellgpu_ctx* ctx, size_t n, const uint8_t* k, const uint8_t* in_x,
                         uint8_t* out_x, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    if (n && !out_status) return e.fail(ELLGPU_E_ARG, "null buffer");
    // (never deferred: the status bytes are put together on the host)
    e.defer_collect();
    std::vector<uint8_t> inf(n ? n : 1);
    const int rc = e.x25519(w, n, k, in_x, out_x, inf.data(), out_status);
    if (!rc)
      for (size_t i = 0; i < n; i++) out_status[i] = out_status[i] ? 1 : (inf[i] ? 2 : 0);
    return rc;
  });
}

int ellgpu_decompress(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* v, const uint8_t* odd,
                      uint8_t* out_xy, uint8_t* out_ok) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.decompress(w, curve, n, v, odd, out_xy, out_ok); });
}
int ellgpu_decompress_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* v, const uint8_t* odd,
                          uint8_t* out_xy, uint8_t* out_ok, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.decompress(w, curve, n, v, odd, out_xy, out_ok); });
}

// point codecs and key validation (decodePoint / encode / KeyPair#validate)
int ellgpu_decode_points(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* enc, size_t enc_len,
                         uint8_t* out_xy, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.decode_points(w, curve, n, enc, enc_len, out_xy, out_status); });
}
int ellgpu_decode_points_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* enc, size_t enc_len,
                             uint8_t* out_xy, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.decode_points(w, curve, n, enc, enc_len, out_xy, out_status); });
}
int ellgpu_encode_points(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, int compact,
                         uint8_t* out_enc) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.encode_points(w, curve, n, xy, compact, out_enc); });
}
int ellgpu_encode_points_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, int compact,
                             uint8_t* out_enc, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.encode_points(w, curve, n, xy, compact, out_enc); });
}
int ellgpu_validate(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, const uint8_t* inf,
                    int check_order, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.validate(w, curve, n, xy, inf, check_order, out_status); });
}
int ellgpu_validate_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, const uint8_t* inf,
                        int check_order, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.validate(w, curve, n, xy, inf, check_order, out_status); });
}

// Point#add on affine points
int ellgpu_point_add(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy1, const uint8_t* inf1,
                     const uint8_t* xy2, const uint8_t* inf2, uint8_t* out_xy, uint8_t* out_inf) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.point_add(w, curve, n, xy1, inf1, xy2, inf2, out_xy, out_inf); });
}
int ellgpu_point_add_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy1, const uint8_t* inf1,
                         const uint8_t* xy2, const uint8_t* inf2, uint8_t* out_xy, uint8_t* out_inf,
                         void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.point_add(w, curve, n, xy1, inf1, xy2, inf2, out_xy, out_inf); });
}

// signature DER codec and EC#verify on wire formats
int ellgpu_sig_from_der(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* der, size_t stride,
                        const uint32_t* der_len, uint8_t* out_r, uint8_t* out_s, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.sig_from_der(w, curve, n, der, stride, der_len, out_r, out_s, out_status); });
}
int ellgpu_sig_from_der_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* der, size_t stride,
                            const uint32_t* der_len, uint8_t* out_r, uint8_t* out_s, uint8_t* out_status,
                            void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.sig_from_der(w, curve, n, der, stride, der_len, out_r, out_s, out_status); });
}
int ellgpu_sig_to_der(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* r, const uint8_t* s,
                      uint8_t* out_der, size_t stride, uint32_t* out_len) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.sig_to_der(w, curve, n, r, s, out_der, stride, out_len); });
}
int ellgpu_sig_to_der_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* r, const uint8_t* s,
                          uint8_t* out_der, size_t stride, uint32_t* out_len, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.sig_to_der(w, curve, n, r, s, out_der, stride, out_len); });
}
int ellgpu_ecdsa_verify_wire(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                             int msg_bits, const uint8_t* der, size_t der_stride, const uint32_t* der_len,
                             const uint8_t* pub_enc, size_t pub_len, uint8_t* out_ok, uint8_t* out_err) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    return e.ecdsa_verify_wire(w, curve, n, hash, hash_len, msg_bits, der, der_stride, der_len, pub_enc, pub_len, out_ok, out_err);
  });
}
int ellgpu_ecdsa_verify_wire_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                                 int msg_bits, const uint8_t* der, size_t der_stride,
                                 const uint32_t* der_len, const uint8_t* pub_enc, size_t pub_len,
                                 uint8_t* out_ok, uint8_t* out_err, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) {
    return e.ecdsa_verify_wire(w, curve, n, hash, hash_len, msg_bits, der, der_stride, der_len, pub_enc, pub_len, out_ok, out_err);
  });
}

// wire formats on user-defined short curves (a group: member 0, like the presets' wire verify)
int ellgpu_custom_decompress(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* x, const uint8_t* odd,
                             uint8_t* out_xy, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_decompress(w, curve, n, x, odd, out_xy, out_status); });
}
int ellgpu_custom_decompress_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* x, const uint8_t* odd,
                                 uint8_t* out_xy, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_decompress(w, curve, n, x, odd, out_xy, out_status); });
}
int ellgpu_custom_decode_points(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* enc, size_t enc_len,
                                uint8_t* out_xy, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_decode_points(w, curve, n, enc, enc_len, out_xy, out_status); });
}
int ellgpu_custom_decode_points_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* enc, size_t enc_len,
                                    uint8_t* out_xy, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_decode_points(w, curve, n, enc, enc_len, out_xy, out_status); });
}
int ellgpu_custom_verify_wire(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                              int msg_bits, const uint8_t* der, size_t der_stride, const uint32_t* der_len,
                              const uint8_t* pub_enc, size_t pub_len, uint8_t* out_ok, uint8_t* out_err) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    return e.custom_verify_wire(w, curve, n, hash, hash_len, msg_bits, der, der_stride, der_len, pub_enc, pub_len, out_ok, out_err);
  });
}
int ellgpu_custom_verify_wire_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                                  int msg_bits, const uint8_t* der, size_t der_stride,
                                  const uint32_t* der_len, const uint8_t* pub_enc, size_t pub_len,
                                  uint8_t* out_ok, uint8_t* out_err, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) {
    return e.custom_verify_wire(w, curve, n, hash, hash_len, msg_bits, der, der_stride, der_len, pub_enc, pub_len, out_ok, out_err);
  });
}

// EC#recoverPubKey on a user-defined ECDSA domain (a group: member 0)
int ellgpu_custom_recover(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                          const uint8_t* r, const uint8_t* s, const uint8_t* recid, uint8_t* out_xy,
                          uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_recover(w, curve, n, hash, hash_len, r, s, recid, out_xy, out_status); });
}
int ellgpu_custom_recover_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                              const uint8_t* r, const uint8_t* s, const uint8_t* recid, uint8_t* out_xy,
                              uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_recover(w, curve, n, hash, hash_len, r, s, recid, out_xy, out_status); });
}

// EC#sign on a user-defined ECDSA domain (a group: member 0): supplied nonces, or HmacDRBG over drbg_hash
static_assert(ELLGPU_CUSTOM_SIGN_MAX_DRAWS == ell::CUSTOM_SIGN_MAX_DRAWS, "the header's draw cap is the engine's");
int ellgpu_custom_sign(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                       const uint8_t* priv, const uint8_t* nonces, int canonical, uint8_t* out_r,
                       uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    return e.custom_sign(w, curve, n, hash, hash_len, msg_bits, priv, nonces, false, 0, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_custom_sign_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                           const uint8_t* priv, const uint8_t* nonces, int canonical, uint8_t* out_r,
                           uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) {
    return e.custom_sign(w, curve, n, hash, hash_len, msg_bits, priv, nonces, false, 0, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_custom_sign_det(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                           const uint8_t* priv, int drbg_hash, int canonical, uint8_t* out_r, uint8_t* out_s,
                           uint8_t* out_recid, uint8_t* out_ok) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    return e.custom_sign(w, curve, n, hash, hash_len, msg_bits, priv, nullptr, true, drbg_hash, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_custom_sign_det_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                               int msg_bits, const uint8_t* priv, int drbg_hash, int canonical, uint8_t* out_r,
                               uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) {
    return e.custom_sign(w, curve, n, hash, hash_len, msg_bits, priv, nullptr, true, drbg_hash, canonical, out_r, out_s, out_recid, out_ok);
  });
}

// KeyPair#derive, KeyPair#validate and BasePoint#encode on a user-defined short curve (a group: member 0)
int ellgpu_custom_derive(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_xy,
                         uint8_t* out_x, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_derive(w, curve, n, priv, pub_xy, false, 0, out_x, out_status, nullptr); });
}
int ellgpu_custom_derive_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_xy,
                             uint8_t* out_x, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_derive(w, curve, n, priv, pub_xy, false, 0, out_x, out_status, nullptr); });
}
int ellgpu_custom_derive_wire(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_enc,
                              size_t pub_len, uint8_t* out_x, uint8_t* out_status, uint8_t* out_err) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_derive(w, curve, n, priv, pub_enc, true, pub_len, out_x, out_status, out_err); });
}
int ellgpu_custom_derive_wire_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_enc,
                                  size_t pub_len, uint8_t* out_x, uint8_t* out_status, uint8_t* out_err,
                                  void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_derive(w, curve, n, priv, pub_enc, true, pub_len, out_x, out_status, out_err); });
}
int ellgpu_custom_validate(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, const uint8_t* inf,
                           int check_order, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_validate(w, curve, n, xy, inf, check_order, out_status); });
}
int ellgpu_custom_validate_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, const uint8_t* inf,
                               int check_order, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_validate(w, curve, n, xy, inf, check_order, out_status); });
}
int ellgpu_custom_encode_points(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, int compact,
                                uint8_t* out_enc) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_encode_points(w, curve, n, xy, compact, out_enc); });
}
int ellgpu_custom_encode_points_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, int compact,
                                    uint8_t* out_enc, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_encode_points(w, curve, n, xy, compact, out_enc); });
}

// pointFromX / pointFromY, decodePoint, KeyPair#validate, KeyPair#derive and BasePoint#encode on a
// user-defined Edwards curve (a group: member 0)
int ellgpu_custom_ed_decompress(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* v, const uint8_t* odd,
                                int from_y, uint8_t* out_xy, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_ed_decompress(w, curve, n, v, odd, from_y, out_xy, out_status); });
}
int ellgpu_custom_ed_decompress_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* v, const uint8_t* odd,
                                    int from_y, uint8_t* out_xy, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_ed_decompress(w, curve, n, v, odd, from_y, out_xy, out_status); });
}
int ellgpu_custom_ed_decode_points(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* enc, size_t enc_len,
                                   uint8_t* out_xy, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_ed_decode_points(w, curve, n, enc, enc_len, out_xy, out_status); });
}
int ellgpu_custom_ed_decode_points_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* enc, size_t enc_len,
                                       uint8_t* out_xy, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_ed_decode_points(w, curve, n, enc, enc_len, out_xy, out_status); });
}
int ellgpu_custom_ed_validate(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, const uint8_t* order_host,
                              uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_ed_validate(w, curve, n, xy, order_host, out_status); });
}
int ellgpu_custom_ed_validate_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, const uint8_t* order_host,
                                  uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_ed_validate(w, curve, n, xy, order_host, out_status); });
}
int ellgpu_custom_ed_derive(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_xy,
                            uint8_t* out_x, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_ed_derive(w, curve, n, priv, pub_xy, false, 0, out_x, out_status, nullptr); });
}
int ellgpu_custom_ed_derive_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_xy,
                                uint8_t* out_x, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_ed_derive(w, curve, n, priv, pub_xy, false, 0, out_x, out_status, nullptr); });
}
int ellgpu_custom_ed_derive_wire(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_enc,
                                 size_t pub_len, uint8_t* out_x, uint8_t* out_status, uint8_t* out_err) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_ed_derive(w, curve, n, priv, pub_enc, true, pub_len, out_x, out_status, out_err); });
}
int ellgpu_custom_ed_derive_wire_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_enc,
                                     size_t pub_len, uint8_t* out_x, uint8_t* out_status, uint8_t* out_err,
                                     void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_ed_derive(w, curve, n, priv, pub_enc, true, pub_len, out_x, out_status, out_err); });
}
int ellgpu_custom_ed_encode_points(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, int compact,
                                   uint8_t* out_enc) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_ed_encode_points(w, curve, n, xy, compact, out_enc); });
}
int ellgpu_custom_ed_encode_points_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* xy, int compact,
                                       uint8_t* out_enc, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_ed_encode_points(w, curve, n, xy, compact, out_enc); });
}

// EC#verify and EC#sign on a user-defined Edwards domain (a group: member 0)
int ellgpu_custom_ed_verify(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                            const uint8_t* r, const uint8_t* s, const uint8_t* pub_xy, uint8_t* out_ok,
                            uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_ed_verify(w, curve, n, hash, hash_len, msg_bits, r, s, pub_xy, out_ok, out_status); });
}
int ellgpu_custom_ed_verify_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                                const uint8_t* r, const uint8_t* s, const uint8_t* pub_xy, uint8_t* out_ok,
                                uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_ed_verify(w, curve, n, hash, hash_len, msg_bits, r, s, pub_xy, out_ok, out_status); });
}
int ellgpu_custom_ed_sign(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                          const uint8_t* priv, const uint8_t* nonces, int canonical, uint8_t* out_r,
                          uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    return e.custom_ed_sign(w, curve, n, hash, hash_len, msg_bits, priv, nonces, false, 0, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_custom_ed_sign_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                              const uint8_t* priv, const uint8_t* nonces, int canonical, uint8_t* out_r,
                              uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) {
    return e.custom_ed_sign(w, curve, n, hash, hash_len, msg_bits, priv, nonces, false, 0, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_custom_ed_sign_det(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                              const uint8_t* priv, int drbg_hash, int canonical, uint8_t* out_r, uint8_t* out_s,
                              uint8_t* out_recid, uint8_t* out_ok) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    return e.custom_ed_sign(w, curve, n, hash, hash_len, msg_bits, priv, nullptr, true, drbg_hash, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_custom_ed_sign_det_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                                  int msg_bits, const uint8_t* priv, int drbg_hash, int canonical, uint8_t* out_r,
                                  uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) {
    return e.custom_ed_sign(w, curve, n, hash, hash_len, msg_bits, priv, nullptr, true, drbg_hash, canonical, out_r, out_s, out_recid, out_ok);
  });
}

// Point#mul + getX, MontCurve#validate and KeyPair#derive on a user-defined Montgomery curve (a group: member 0)
int ellgpu_custom_mont_ladder(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* k, const uint8_t* in_x,
                              uint8_t* out_x, uint8_t* out_inf) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_mont(w, curve, Eng::OP_MONTC_LADDER, n, k, in_x, out_x, out_inf); });
}
int ellgpu_custom_mont_ladder_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* k, const uint8_t* in_x,
                                  uint8_t* out_x, uint8_t* out_inf, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_mont(w, curve, Eng::OP_MONTC_LADDER, n, k, in_x, out_x, out_inf); });
}
int ellgpu_custom_mont_validate(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* in_x, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_mont(w, curve, Eng::OP_MONTC_VALIDATE, n, nullptr, in_x, nullptr, out_status); });
}
int ellgpu_custom_mont_validate_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* in_x, uint8_t* out_status,
                                    void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_mont(w, curve, Eng::OP_MONTC_VALIDATE, n, nullptr, in_x, nullptr, out_status); });
}
int ellgpu_custom_mont_derive(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_x,
                              uint8_t* out_x, uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.custom_mont(w, curve, Eng::OP_MONTC_DERIVE, n, priv, pub_x, out_x, out_status); });
}
int ellgpu_custom_mont_derive_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* priv, const uint8_t* pub_x,
                                  uint8_t* out_x, uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.custom_mont(w, curve, Eng::OP_MONTC_DERIVE, n, priv, pub_x, out_x, out_status); });
}

// ECDSA sign and recover on the presets, EdDSA
int ellgpu_ecdsa_sign(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, int msg_bits,
                      const uint8_t* priv, const uint8_t* nonces, int canonical, uint8_t* out_r,
                      uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    return e.ecdsa_sign(w, curve, n, hash, hash_len, msg_bits, priv, nonces, false, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_ecdsa_sign_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                          int msg_bits, const uint8_t* priv, const uint8_t* nonces, int canonical,
                          uint8_t* out_r, uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok,
                          void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) {
    return e.ecdsa_sign(w, curve, n, hash, hash_len, msg_bits, priv, nonces, false, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_ecdsa_sign_det(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                          int msg_bits, const uint8_t* priv, int canonical, uint8_t* out_r, uint8_t* out_s,
                          uint8_t* out_recid, uint8_t* out_ok) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) {
    return e.ecdsa_sign(w, curve, n, hash, hash_len, msg_bits, priv, nullptr, true, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_ecdsa_sign_det_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                              int msg_bits, const uint8_t* priv, int canonical, uint8_t* out_r,
                              uint8_t* out_s, uint8_t* out_recid, uint8_t* out_ok, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) {
    return e.ecdsa_sign(w, curve, n, hash, hash_len, msg_bits, priv, nullptr, true, canonical, out_r, out_s, out_recid, out_ok);
  });
}
int ellgpu_ecdsa_recover(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                         const uint8_t* r, const uint8_t* s, const uint8_t* recid, uint8_t* out_xy,
                         uint8_t* out_status) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.ecdsa_recover(w, curve, n, hash, hash_len, r, s, recid, out_xy, out_status); });
}
int ellgpu_ecdsa_recover_dev(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len,
                             const uint8_t* r, const uint8_t* s, const uint8_t* recid, uint8_t* out_xy,
                             uint8_t* out_status, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.ecdsa_recover(w, curve, n, hash, hash_len, r, s, recid, out_xy, out_status); });
}
int ellgpu_eddsa_verify(ellgpu_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* msg_off,
                        size_t msg_len, const uint8_t* sigs, const uint8_t* pubs, uint8_t* out_ok,
                        uint8_t* out_err) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.eddsa_verify(w, n, msgs, (const ell::u64*)msg_off, msg_len, sigs, pubs, out_ok, out_err); });
}
int ellgpu_eddsa_verify_dev(ellgpu_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* msg_off,
                            size_t msg_len, const uint8_t* sigs, const uint8_t* pubs,
                            uint8_t* out_ok, uint8_t* out_err, void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.eddsa_verify(w, n, msgs, (const ell::u64*)msg_off, msg_len, sigs, pubs, out_ok, out_err); });
}
// EDDSA#verify against the table of the signer's key (include/ellgpu_ext3.h): one form, `mem` says
// where the operands live.  A group shards a host batch of uniform stride as ellgpu_ecdsa_verify_base
// shards its batch (handles are defined on every member); with offsets the call runs on the first member
int ellgpu_eddsa_verify_base(ellgpu_ctx* ctx, int base, size_t n, const uint8_t* msgs, const uint64_t* msg_off,
                             size_t msg_len, const uint8_t* sigs, uint8_t* out_ok, uint8_t* out_err, int mem,
                             void* stream) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  Mem where;
  if (int rc = mem_of(mem, stream, where)) return rc;
  if (!ctx->members.empty() && where == Mem::host && !msg_off && n) {
    ELL_LOCK(ctx);
    if (int rc = ellgpu_base_info(ctx, base, nullptr, nullptr, nullptr)) return rc;
    if (!sigs || !out_ok || (!msgs && msg_len)) return set_err(ELLGPU_E_ARG, "null pointer");
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_eddsa_verify_base(m, base, hi - lo, msgs ? msgs + lo * msg_len : nullptr, nullptr, msg_len,
                                      sigs + lo * 64, out_ok + lo, out_err ? out_err + lo : nullptr, mem, nullptr);
    });
  }
  return ell_call(ctx, stream, where, [=](Eng& e, Mem w) {
    return e.eddsa_verify_base(w, base, n, msgs, (const ell::u64*)msg_off, msg_len, sigs, out_ok, out_err);
  });
}
// include/ellgpu_ext4.h: EC#getKeyRecoveryParam in one pass.  One form, like ellgpu_mul_base; a group
// shards a host batch (the engine's refusals come from the first member that has items)
int ellgpu_ecdsa_recid(ellgpu_ctx* ctx, int curve, size_t n, const uint8_t* hash, int hash_len, const uint8_t* r,
                       const uint8_t* s, const uint8_t* pub_xy, uint8_t* out_recid, uint8_t* out_status, int mem,
                       void* stream) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  Mem where;
  if (int rc = mem_of(mem, stream, where)) return rc;
  if (!ctx->members.empty() && where == Mem::host && n && hash_len > 0 && hash && r && s && pub_xy && out_recid &&
      out_status) {
    ELL_LOCK(ctx);
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    return group_shard(ctx, n, [=](ellgpu_ctx* m, size_t lo, size_t hi) {
      return ellgpu_ecdsa_recid(m, curve, hi - lo, hash + lo * (size_t)hash_len, hash_len, r + lo * NB, s + lo * NB,
                                pub_xy + lo * 2 * B, out_recid + lo, out_status + lo, mem, nullptr);
    });
  }
  return ell_call(ctx, stream, where, [=](Eng& e, Mem w) {
    return e.ecdsa_recid(w, curve, n, hash, hash_len, r, s, pub_xy, out_recid, out_status);
  });
}
// include/ellgpu_addn.h: n sums of m terms k * P each.  One form, like ellgpu_mul_base; a group shards
// a host batch by whole sums (fewer sums than members, or operands that the engine refuses anyway:
// the first member)
int ellgpu_mul_sum(ellgpu_ctx* ctx, int curve, size_t n, size_t m, const uint8_t* k, const uint8_t* xy,
                   uint8_t* out_xy, uint8_t* out_inf, int mem, void* stream) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  Mem where;
  if (int rc = mem_of(mem, stream, where)) return rc;
  if (where == Mem::host && ctx->members.size() > 1 && n >= ctx->members.size() && m && k && xy && out_xy &&
      out_inf && m <= SIZE_MAX / n / 256) {
    ELL_LOCK(ctx);
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    return group_shard(ctx, n, [=](ellgpu_ctx* mb, size_t lo, size_t hi) {
      return ellgpu_mul_sum(mb, curve, hi - lo, m, k + lo * m * B, xy + lo * m * 2 * B, out_xy + lo * 2 * B,
                            out_inf + lo, mem, nullptr);
    });
  }
  return ell_call(ctx, stream, where, [=](Eng& e, Mem w) { return e.mul_sum(w, curve, n, m, k, xy, out_xy, out_inf); });
}
// elliptic_amd/include/ellgpu_edsum.h: the same on ed25519 and user-defined Edwards ids (B = 32); one
// form, sharded like ellgpu_mul_sum
int ellgpu_ed_mul_sum(ellgpu_ctx* ctx, int curve, size_t n, size_t m, const uint8_t* k, const uint8_t* xy,
                      uint8_t* out_xy, uint8_t* out_inf, int mem, void* stream) {
  if (!ctx) return set_err(ELLGPU_E_ARG, "null context");
  Mem where;
  if (int rc = mem_of(mem, stream, where)) return rc;
  if (where == Mem::host && ctx->members.size() > 1 && n >= ctx->members.size() && m && k && xy && out_xy &&
      out_inf && m <= SIZE_MAX / n / 256) {
    ELL_LOCK(ctx);
    size_t B, NB;
    if (curve_widths(curve, B, NB)) return ELLGPU_E_ARG;
    B = 32;                                             // (whatever the id: the engine refuses the others)
    return group_shard(ctx, n, [=](ellgpu_ctx* mb, size_t lo, size_t hi) {
      return ellgpu_ed_mul_sum(mb, curve, hi - lo, m, k + lo * m * B, xy + lo * m * 2 * B, out_xy + lo * 2 * B,
                               out_inf + lo, mem, nullptr);
    });
  }
  return ell_call(ctx, stream, where, [=](Eng& e, Mem w) { return e.ed_mul_sum(w, curve, n, m, k, xy, out_xy, out_inf); });
}
int ellgpu_eddsa_sign(ellgpu_ctx* ctx, size_t n, const uint8_t* secrets, const uint8_t* msgs,
                      const uint64_t* msg_off, size_t msg_len, uint8_t* out_sig, uint8_t* out_pub) {
  return ell_call(ctx, nullptr, Mem::host, [=](Eng& e, Mem w) { return e.eddsa_sign(w, n, secrets, msgs, (const ell::u64*)msg_off, msg_len, out_sig, out_pub); });
}
int ellgpu_eddsa_sign_dev(ellgpu_ctx* ctx, size_t n, const uint8_t* secrets, const uint8_t* msgs,
                          const uint64_t* msg_off, size_t msg_len, uint8_t* out_sig, uint8_t* out_pub,
                          void* stream) {
  return ell_call(ctx, stream, Mem::device, [=](Eng& e, Mem w) { return e.eddsa_sign(w, n, secrets, msgs, (const ell::u64*)msg_off, msg_len, out_sig, out_pub); });
}

}  // extern "C"

/*
 * ellgpu_napi.c -- Node N-API addon: the JavaScript-side binding of the C ABI
 * in include/ellgpu.h.  It marshals flat Buffers (fixed-width big-endian
 * integers, exactly BN#toArray('be', len)) into libellgpu.so and back; no curve
 * arithmetic lives here.  The library is dlopen()ed from an explicit path
 * (default ../lib/libellgpu.so next to this addon), so the same addon can be
 * pointed at the CPU unit-test build of the device code in a GPU-less
 * container (tests only, see tests/test_js_install.py).
 *
 *   gcc -shared -fPIC -I/usr/include/node -o ellgpu.node ellgpu_napi.c -ldl
 *
 * Conventions:
 *   - open(path) first; createContext(device | [devices]) -> the external every other call takes first;
 *     destroyContext(ctx) releases it.  The context, curve-definition and base-table calls have a
 *     comment each where they stand.
 *   - Every batch operation is one row of the table ops[] (its signature stands on its row): operands
 *     and results are flat Buffers of n fixed-width big-endian rows; an operand written `x|null` may
 *     be null or undefined; counts (lens) are little-endian uint32, offsets little-endian uint64.
 *   - A batch operation returns an object of result Buffers named as its row says (two return the
 *     bare Buffer).  callAsync(op, ...) is its Promise form, op = ops.<name>.
 *   - Errors -- a refused argument, or the library's own message -- are thrown as plain
 *     `Error(message)`, the reference's convention (minimalistic-assert, dist/elliptic.js:8832-8835);
 *     a Promise-form call that fails in the library rejects with that Error.
 *   - One call per context at a time: index.js serialises the Promise forms.
 */
#include <dlfcn.h>
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

typedef struct ellgpu_ctx ellgpu_ctx;
/* ELLGPU_VERSION of the include/ellgpu.h this file was written against: open() refuses a library
 * that reports another one (a prototype changed; dlsym would still find the name) */
#define ELLGPU_ABI_VERSION 0x000200
static struct {
  void* h;
  int (*version)(void);
  int (*ctx_defer)(ellgpu_ctx*);
  int (*ctx_comb_bits)(ellgpu_ctx*, int);
  int (*ctx_collect)(ellgpu_ctx*);
  const char* (*last_error)(void);
  int (*curve_id)(const char*);
  int (*field_bytes)(int);
  int (*order_bytes)(int);
  int (*device_count)(void);
  int (*ctx_create)(int, ellgpu_ctx**);
  int (*group_create)(const int*, int, ellgpu_ctx**);
  int (*group_size)(const ellgpu_ctx*);
  int (*define_short)(ellgpu_ctx*, const uint8_t*, const uint8_t*, const uint8_t*, int*);
  int (*define_edwards)(ellgpu_ctx*, const uint8_t*, const uint8_t*, const uint8_t*, int*);
  int (*define_mont)(ellgpu_ctx*, const uint8_t*, const uint8_t*, int*);
  int (*custom_mont_ladder)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*custom_mont_validate)(ellgpu_ctx*, int, size_t, const uint8_t*, uint8_t*);
  int (*custom_mont_derive)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*custom_ed_decompress)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, int, uint8_t*, uint8_t*);
  int (*custom_ed_decode_points)(ellgpu_ctx*, int, size_t, const uint8_t*, size_t, uint8_t*, uint8_t*);
  int (*custom_ed_validate)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*);
  int (*custom_ed_derive)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*custom_ed_derive_wire)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, size_t, uint8_t*, uint8_t*,
                               uint8_t*);
  int (*custom_ed_encode_points)(ellgpu_ctx*, int, size_t, const uint8_t*, int, uint8_t*);
  int (*define_short_domain)(ellgpu_ctx*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*,
                             const uint8_t*, const uint8_t*, int*);
  void (*ctx_destroy)(ellgpu_ctx*);
  int (*mul_fixed)(ellgpu_ctx*, int, size_t, const uint8_t*, uint8_t*, uint8_t*);
  int (*base_define)(ellgpu_ctx*, int, const uint8_t*, int, int*);
  int (*ed_base_define)(ellgpu_ctx*, int, const uint8_t*, int, int*);      /* include/ellgpu_ext.h */
  int (*base_release)(ellgpu_ctx*, int);
  int (*base_info)(ellgpu_ctx*, int, int*, int*, uint64_t*);
  int (*mul_base)(ellgpu_ctx*, int, size_t, const uint8_t*, uint8_t*, uint8_t*, int, void*);
  int (*mul_base2)(ellgpu_ctx*, int, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, int, void*);
  int (*ecdsa_verify_base)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, const uint8_t*, uint8_t*, int, void*);
  int (*eddsa_verify_base)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint64_t*, size_t, const uint8_t*, uint8_t*,
                           uint8_t*, int, void*);
  int (*mul_var)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*mul_add2)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, const uint8_t*,
                  const uint8_t*, uint8_t*, uint8_t*);
  int (*ecdsa_verify)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*,
                      const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*x25519)(ellgpu_ctx*, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*x25519_derive)(ellgpu_ctx*, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*decompress)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*ecdsa_sign)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, const uint8_t*,
                    int, uint8_t*, uint8_t*, uint8_t*, uint8_t*);
  int (*eddsa_verify)(ellgpu_ctx*, size_t, const uint8_t*, const uint64_t*, size_t, const uint8_t*,
                      const uint8_t*, uint8_t*, uint8_t*);
  int (*eddsa_sign)(ellgpu_ctx*, size_t, const uint8_t*, const uint8_t*, const uint64_t*, size_t,
                    uint8_t*, uint8_t*);
  int (*ecdsa_recover)(ellgpu_ctx*, int, size_t, const uint8_t*, int, const uint8_t*, const uint8_t*,
                       const uint8_t*, uint8_t*, uint8_t*);
  int (*ecdsa_sign_det)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, int,
                        uint8_t*, uint8_t*, uint8_t*, uint8_t*);
  int (*decode_points)(ellgpu_ctx*, int, size_t, const uint8_t*, size_t, uint8_t*, uint8_t*);
  int (*encode_points)(ellgpu_ctx*, int, size_t, const uint8_t*, int, uint8_t*);
  int (*validate)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, int, uint8_t*);
  int (*point_add)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*,
                   uint8_t*, uint8_t*);
  int (*sig_from_der)(ellgpu_ctx*, int, size_t, const uint8_t*, size_t, const uint32_t*, uint8_t*, uint8_t*,
                      uint8_t*);
  int (*sig_to_der)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, size_t, uint32_t*);
  int (*verify_wire)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, size_t,
                     const uint32_t*, const uint8_t*, size_t, uint8_t*, uint8_t*);
  int (*custom_decompress)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*custom_decode_points)(ellgpu_ctx*, int, size_t, const uint8_t*, size_t, uint8_t*, uint8_t*);
  int (*custom_recover)(ellgpu_ctx*, int, size_t, const uint8_t*, int, const uint8_t*, const uint8_t*,
                        const uint8_t*, uint8_t*, uint8_t*);
  int (*custom_derive)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
  int (*custom_derive_wire)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, size_t, uint8_t*, uint8_t*,
                            uint8_t*);
  int (*custom_validate)(ellgpu_ctx*, int, size_t, const uint8_t*, const uint8_t*, int, uint8_t*);
  int (*custom_encode_points)(ellgpu_ctx*, int, size_t, const uint8_t*, int, uint8_t*);
  int (*custom_sign)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, const uint8_t*, int,
                     uint8_t*, uint8_t*, uint8_t*, uint8_t*);
  int (*define_edwards_domain)(ellgpu_ctx*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*,
                               const uint8_t*, const uint8_t*, int*);
  int (*custom_ed_verify)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, const uint8_t*,
                          const uint8_t*, uint8_t*, uint8_t*);
  int (*custom_ed_sign)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, const uint8_t*, int,
                        uint8_t*, uint8_t*, uint8_t*, uint8_t*);
  int (*custom_ed_sign_det)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, int, int,
                            uint8_t*, uint8_t*, uint8_t*, uint8_t*);
  int (*custom_sign_det)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, int, int,
                         uint8_t*, uint8_t*, uint8_t*, uint8_t*);
  int (*custom_verify_wire)(ellgpu_ctx*, int, size_t, const uint8_t*, int, int, const uint8_t*, size_t,
                            const uint32_t*, const uint8_t*, size_t, uint8_t*, uint8_t*);
} L;

#define THROW(env, msg) do { napi_throw_error((env), NULL, (msg)); return NULL; } while (0)
#define CHECK(env, call) do { if ((call) != napi_ok) THROW(env, "N-API call failed"); } while (0)

static napi_value lib_error(napi_env env) {
  const char* m = L.last_error ? L.last_error() : "ellgpu error";
  napi_throw_error(env, NULL, m && *m ? m : "ellgpu error");
  return NULL;
}
static int need_lib(napi_env env) {
  if (!L.h) { napi_throw_error(env, NULL, "ellgpu: library not opened (call open(path) first)"); return 0; }
  return 1;
}

static napi_value fn_open(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  char path[4096]; size_t len = 0;
  if (argc < 1 || napi_get_value_string_utf8(env, argv[0], path, sizeof path, &len) != napi_ok)
    THROW(env, "open(path): path string required");
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) { char msg[4400]; snprintf(msg, sizeof msg, "ellgpu: cannot load %s: %s", path, dlerror()); THROW(env, msg); }
#define SYM(field, name) do { *(void**)(&L.field) = dlsym(h, name); if (!L.field) { char m_[256]; \
    snprintf(m_, sizeof m_, "ellgpu: %s missing from library", name); dlclose(h); THROW(env, m_); } } while (0)
  SYM(version, "ellgpu_version");
  if (L.version() != ELLGPU_ABI_VERSION) {
    char m_[256];
    snprintf(m_, sizeof m_, "ellgpu: library reports ABI version 0x%06x, this addon was built for 0x%06x (include/ellgpu.h)",
             L.version(), ELLGPU_ABI_VERSION);
    dlclose(h); THROW(env, m_);
  }
  SYM(ctx_defer, "ellgpu_ctx_defer"); SYM(ctx_collect, "ellgpu_ctx_collect");
  SYM(ctx_comb_bits, "ellgpu_ctx_comb_bits");
  SYM(last_error, "ellgpu_last_error"); SYM(curve_id, "ellgpu_curve_id");
  SYM(field_bytes, "ellgpu_curve_field_bytes"); SYM(order_bytes, "ellgpu_curve_order_bytes");
  SYM(device_count, "ellgpu_device_count"); SYM(ctx_create, "ellgpu_ctx_create");
  SYM(group_create, "ellgpu_group_create"); SYM(group_size, "ellgpu_group_size");
  SYM(define_short, "ellgpu_curve_define_short");
  SYM(define_edwards, "ellgpu_curve_define_edwards");
  SYM(define_mont, "ellgpu_curve_define_mont");
  SYM(ed_base_define, "ellgpu_ed_base_define");
  SYM(base_define, "ellgpu_base_define"); SYM(base_release, "ellgpu_base_release"); SYM(base_info, "ellgpu_base_info");
  SYM(mul_base, "ellgpu_mul_base"); SYM(mul_base2, "ellgpu_mul_base2");
  SYM(ecdsa_verify_base, "ellgpu_ecdsa_verify_base");
  SYM(eddsa_verify_base, "ellgpu_eddsa_verify_base");
  SYM(custom_mont_ladder, "ellgpu_custom_mont_ladder");
  SYM(custom_mont_validate, "ellgpu_custom_mont_validate");
  SYM(custom_mont_derive, "ellgpu_custom_mont_derive");
  SYM(custom_ed_decompress, "ellgpu_custom_ed_decompress");
  SYM(custom_ed_decode_points, "ellgpu_custom_ed_decode_points");
  SYM(custom_ed_validate, "ellgpu_custom_ed_validate");
  SYM(custom_ed_derive, "ellgpu_custom_ed_derive");
  SYM(custom_ed_derive_wire, "ellgpu_custom_ed_derive_wire");
  SYM(custom_ed_encode_points, "ellgpu_custom_ed_encode_points");
  SYM(define_short_domain, "ellgpu_curve_define_short_domain");
  SYM(ctx_destroy, "ellgpu_ctx_destroy"); SYM(mul_fixed, "ellgpu_mul_fixed"); SYM(mul_var, "ellgpu_mul_var");
  SYM(mul_add2, "ellgpu_mul_add2"); SYM(ecdsa_verify, "ellgpu_ecdsa_verify"); SYM(x25519, "ellgpu_x25519_ladder");
  SYM(x25519_derive, "ellgpu_x25519_derive");
  SYM(decompress, "ellgpu_decompress");
  SYM(eddsa_verify, "ellgpu_eddsa_verify");
  SYM(eddsa_sign, "ellgpu_eddsa_sign");
  SYM(ecdsa_recover, "ellgpu_ecdsa_recover");
  SYM(ecdsa_sign_det, "ellgpu_ecdsa_sign_det");
  SYM(ecdsa_sign, "ellgpu_ecdsa_sign");
  SYM(decode_points, "ellgpu_decode_points");
  SYM(encode_points, "ellgpu_encode_points");
  SYM(validate, "ellgpu_validate");
  SYM(point_add, "ellgpu_point_add");
  SYM(sig_from_der, "ellgpu_sig_from_der");
  SYM(sig_to_der, "ellgpu_sig_to_der");
  SYM(verify_wire, "ellgpu_ecdsa_verify_wire");
  SYM(custom_decompress, "ellgpu_custom_decompress");
  SYM(custom_decode_points, "ellgpu_custom_decode_points");
  SYM(custom_verify_wire, "ellgpu_custom_verify_wire");
  SYM(custom_recover, "ellgpu_custom_recover");
  SYM(custom_derive, "ellgpu_custom_derive");
  SYM(custom_derive_wire, "ellgpu_custom_derive_wire");
  SYM(custom_validate, "ellgpu_custom_validate");
  SYM(custom_encode_points, "ellgpu_custom_encode_points");
  SYM(custom_sign, "ellgpu_custom_sign");
  SYM(custom_sign_det, "ellgpu_custom_sign_det");
  SYM(define_edwards_domain, "ellgpu_curve_define_edwards_domain");
  SYM(custom_ed_verify, "ellgpu_custom_ed_verify");
  SYM(custom_ed_sign, "ellgpu_custom_ed_sign");
  SYM(custom_ed_sign_det, "ellgpu_custom_ed_sign_det");
  L.h = h;
  napi_value t; CHECK(env, napi_get_boolean(env, 1, &t));
  return t;
}

/* Environment teardown (the script has ended, node is about to exit): finalizers still run then
 * (node >= 12.17), in no useful order with respect to the HIP runtime's own exit handlers and its
 * helper threads.  A context that is still alive at that point is not torn down piece by piece --
 * the process ends, the driver reclaims its device memory -- and the result-buffer pool stops
 * telling V8 about memory V8 no longer tracks.  (One of ~ 40 fuzz processes on a loaded GPU box
 * ended with SIGSEGV AFTER its last line of output; nothing but teardown was left to run.)
 * g_closing is set by an environment cleanup hook, which node runs before the finalizers. */
static int g_closing = 0;
static void on_env_cleanup(void* arg) { (void)arg; g_closing = 1; }
/* Contexts are PINNED: the addon holds a strong reference to every context external until
 * destroyContext(ctx) is called (Engine#close in index.js).  Left to the garbage collector, the
 * external of a script that has just run off its end is garbage a moment before node frees the
 * environment; when a collection falls into that moment, the reference's first-pass weak callback
 * has run and its second pass is a pending task while napi_env's teardown finalizes and deletes
 * the same reference -- and node 12.22 then runs the pending second pass on freed memory (caught
 * under rocgdb: FreeEnvironment -> RunCleanup -> CleanupHandles -> uv_run ->
 * InvokeSecondPassPhantomCallbacks -> N-API's reference helpers; fixed in node >= 14.17).  A strong
 * reference has no weak callback.  A context owns gigabytes of device memory anyway: its lifetime
 * is explicit, like that of the stream it wraps. */
#define MAX_CTX 64
static struct { ellgpu_ctx* c; napi_ref pin; } g_ctx[MAX_CTX];
static int g_jobs_in_flight = 0;
static int ctx_slot(ellgpu_ctx* c) {
  for (int i = 0; i < MAX_CTX; i++) if (g_ctx[i].c == c) return i;
  return -1;
}
static void ctx_finalize(napi_env env, void* data, void* hint) {
  (void)env; (void)hint;
  if (getenv("ELLGPU_NAPI_TRACE")) fprintf(stderr, "ellgpu_napi: ctx_finalize closing=%d\n", g_closing);
  /* (reached for the external of a context that destroyContext has released -- only then is it
   * unpinned and collectable -- and for every external at environment teardown: nothing is left to do) */
  (void)data;
}
static napi_value fn_create(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 1; napi_value argv[1]; int32_t dev = 0;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ellgpu_ctx* c = NULL;
  bool is_arr = false;
  if (argc >= 1) napi_is_array(env, argv[0], &is_arr);
  if (is_arr) {
    /* createContext([d0, d1, ...]): a device group (ellgpu_group_create) -- the batch entry
     * points shard over the devices, every other call runs on the first one */
    uint32_t nd = 0; int devs[64];
    CHECK(env, napi_get_array_length(env, argv[0], &nd));
    if (nd < 1 || nd > 64) THROW(env, "createContext([devices]): 1..64 devices");
    for (uint32_t i = 0; i < nd; i++) {
      napi_value e; int32_t d = 0;
      CHECK(env, napi_get_element(env, argv[0], i, &e));
      if (napi_get_value_int32(env, e, &d) != napi_ok) THROW(env, "createContext([devices]): integers expected");
      devs[i] = d;
    }
    if (L.group_create(devs, (int)nd, &c) != 0) return lib_error(env);
  } else {
    if (argc >= 1) napi_get_value_int32(env, argv[0], &dev);
    if (L.ctx_create(dev, &c) != 0) return lib_error(env);
  }
  int slot = ctx_slot(NULL);
  if (slot < 0) { L.ctx_destroy(c); THROW(env, "ellgpu: too many live contexts (destroyContext / Engine#close releases one)"); }
  napi_value ext;
  if (napi_create_external(env, c, ctx_finalize, NULL, &ext) != napi_ok ||
      napi_create_reference(env, ext, 1, &g_ctx[slot].pin) != napi_ok) { L.ctx_destroy(c); THROW(env, "ellgpu: could not wrap the context"); }
  g_ctx[slot].c = c;
  return ext;
}
static ellgpu_ctx* get_ctx(napi_env env, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) { napi_throw_error(env, NULL, "ellgpu: bad context"); return NULL; }
  if (ctx_slot((ellgpu_ctx*)p) < 0) { napi_throw_error(env, NULL, "ellgpu: the context has been destroyed"); return NULL; }
  return (ellgpu_ctx*)p;
}
static int get_buf(napi_env env, napi_value v, const uint8_t** p, size_t* len, int allow_null) {
  napi_valuetype t; napi_typeof(env, v, &t);
  if (allow_null && (t == napi_null || t == napi_undefined)) { *p = NULL; *len = 0; return 1; }
  bool isbuf = 0; napi_is_buffer(env, v, &isbuf);
  if (!isbuf) { napi_throw_error(env, NULL, "ellgpu: Buffer expected"); return 0; }
  void* d; if (napi_get_buffer_info(env, v, &d, len) != napi_ok) { napi_throw_error(env, NULL, "ellgpu: bad Buffer"); return 0; }
  *p = (const uint8_t*)d; return 1;
}
/* ---- result buffers -------------------------------------------------------------------
 * A fresh n x 64-byte Buffer costs more to fault in (first touch, ~6 ms per 64 MB, whoever
 * touches it) than the GPU needs to fill it.  Large result Buffers are therefore external
 * Buffers over blocks that return to a free list when V8 collects them: after the first call of
 * a given size the memory has been touched already.  The blocks are 2 MiB-aligned and advised
 * as huge pages (the copy engine moves device data into huge-page-backed memory ~3x faster
 * than into 4 KiB pages here; numpy does the same for its large arrays).  Callers that keep
 * their own result Buffers pass them in (mulFixed / mulVar / mulAdd2: trailing xy, inf
 * arguments) and skip all of this.  Everything here runs on the JS thread. */
typedef struct pool_blk { void* p; size_t cap; struct pool_blk* next; } pool_blk;
static pool_blk* g_pool = NULL;
static size_t g_pool_bytes = 0;
#define POOL_MIN_BYTES ((size_t)256 * 1024)
#define POOL_MAX_BYTES ((size_t)1 << 31)
static void pool_release(napi_env env, void* data, void* hint) {
  (void)data;
  pool_blk* b = (pool_blk*)hint;
  int64_t adj;
  if (g_closing) { free(b->p); free(b); return; }
  napi_adjust_external_memory(env, -(int64_t)b->cap, &adj);
  if (g_pool_bytes + b->cap > POOL_MAX_BYTES) { free(b->p); free(b); return; }
  b->next = g_pool; g_pool = b; g_pool_bytes += b->cap;
}
static napi_status result_buffer(napi_env env, size_t size, void** data, napi_value* out) {
  if (size < POOL_MIN_BYTES) return napi_create_buffer(env, size, data, out);
  if (getenv("ELLGPU_NAPI_TRACE")) fprintf(stderr, "ellgpu_napi: pooled result buffer of %zu bytes\n", size);
  pool_blk **pp = &g_pool, **best = NULL;
  for (; *pp; pp = &(*pp)->next)                         /* best fit, at most 2x the request */
    if ((*pp)->cap >= size && (*pp)->cap <= 2 * size && (!best || (*pp)->cap < (*best)->cap)) best = pp;
  pool_blk* b;
  if (best) {
    b = *best; *best = b->next; g_pool_bytes -= b->cap;
  } else {
    b = (pool_blk*)malloc(sizeof *b);
    if (!b) return napi_generic_failure;
    b->cap = (size + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
    if (posix_memalign(&b->p, (size_t)2 << 20, b->cap) != 0) { free(b); return napi_generic_failure; }
    madvise(b->p, b->cap, MADV_HUGEPAGE);                /* as numpy does for large arrays */
    memset(b->p, 0, b->cap);                             /* first touch here, once per block */
  }
  b->next = NULL;
  *data = b->p;
  napi_status st = napi_create_external_buffer(env, size, b->p, pool_release, b, out);
  if (st != napi_ok) { free(b->p); free(b); return st; }
  int64_t adj;                                           /* let V8 see the memory behind the Buffer */
  napi_adjust_external_memory(env, (int64_t)b->cap, &adj);
  return st;
}

static int curve_id_of(const char* name) { return L.curve_id(name); }
static napi_value fn_curve_id(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 1; napi_value argv[1]; char name[64]; size_t len;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (napi_get_value_string_utf8(env, argv[0], name, sizeof name, &len) != napi_ok) THROW(env, "curveId(name)");
  napi_value r; CHECK(env, napi_create_int32(env, curve_id_of(name), &r)); return r;
}
static napi_value int_fn(napi_env env, napi_callback_info info, int which) {
  if (!need_lib(env)) return NULL;
  size_t argc = 1; napi_value argv[1]; int32_t id = 0;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc >= 1) napi_get_value_int32(env, argv[0], &id);
  int v = which == 0 ? L.field_bytes(id) : which == 1 ? L.order_bytes(id) : L.device_count();
  napi_value r; CHECK(env, napi_create_int32(env, v, &r)); return r;
}
static napi_value fn_field_bytes(napi_env e, napi_callback_info i) { return int_fn(e, i, 0); }
static napi_value fn_order_bytes(napi_env e, napi_callback_info i) { return int_fn(e, i, 1); }
static napi_value fn_device_count(napi_env e, napi_callback_info i) { return int_fn(e, i, 2); }

static napi_value fn_group_size(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 1; napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  napi_value v; CHECK(env, napi_create_int32(env, L.group_size(c), &v));
  return v;
}
/* defineShort(ctx, p, a, b) / defineEdwards(ctx, p, a, d) -> curve id: 32-byte big-endian Buffers
 * (ellgpu_curve_define_short / ellgpu_curve_define_edwards) */
static napi_value define_common(napi_env env, napi_callback_info info, int edwards) {
  if (!need_lib(env)) return NULL;
  size_t argc = 4; napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 4) THROW(env, "defineShort(ctx, p, a, b)");
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  const uint8_t* b[3]; size_t l[3];
  for (int i = 0; i < 3; i++) {
    if (!get_buf(env, argv[1 + i], &b[i], &l[i], 0)) return NULL;
    if (l[i] != 32) THROW(env, "defineShort: p, a, b are 32-byte big-endian Buffers");
  }
  int id = -1;
  if ((edwards ? L.define_edwards : L.define_short)(c, b[0], b[1], b[2], &id) != 0) THROW(env, L.last_error());
  napi_value v; CHECK(env, napi_create_int32(env, id, &v));
  return v;
}
static napi_value fn_define_short(napi_env e, napi_callback_info i) { return define_common(e, i, 0); }
static napi_value fn_define_edwards(napi_env e, napi_callback_info i) { return define_common(e, i, 1); }
/* defineMont(ctx, p, a) -> curve id: 32-byte big-endian Buffers (ellgpu_curve_define_mont; no b) */
static napi_value fn_define_mont(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 3; napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) THROW(env, "defineMont(ctx, p, a)");
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  const uint8_t* b[2]; size_t l[2];
  for (int i = 0; i < 2; i++) {
    if (!get_buf(env, argv[1 + i], &b[i], &l[i], 0)) return NULL;
    if (l[i] != 32) THROW(env, "defineMont: p, a are 32-byte big-endian Buffers");
  }
  int id = -1;
  if (L.define_mont(c, b[0], b[1], &id) != 0) THROW(env, L.last_error());
  napi_value v; CHECK(env, napi_create_int32(env, id, &v));
  return v;
}
/* defineShortDomain(ctx, p, a, b, n, gx, gy) -> curve id: 32-byte big-endian Buffers
 * (ellgpu_curve_define_short_domain) */
static napi_value define_domain_with(napi_env env, napi_callback_info info, int edwards) {
  if (!need_lib(env)) return NULL;
  size_t argc = 7; napi_value argv[7];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 7) THROW(env, edwards ? "defineEdwardsDomain(ctx, p, a, d, n, gx, gy)" : "defineShortDomain(ctx, p, a, b, n, gx, gy)");
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  const uint8_t* b[6]; size_t l[6];
  for (int i = 0; i < 6; i++) {
    if (!get_buf(env, argv[1 + i], &b[i], &l[i], 0)) return NULL;
    if (l[i] != 32) THROW(env, "defineShortDomain / defineEdwardsDomain: the six parameters are 32-byte big-endian Buffers");
  }
  int id = -1;
  if ((edwards ? L.define_edwards_domain : L.define_short_domain)(c, b[0], b[1], b[2], b[3], b[4], b[5], &id) != 0)
    THROW(env, L.last_error());
  napi_value v; CHECK(env, napi_create_int32(env, id, &v));
  return v;
}
static napi_value fn_define_short_domain(napi_env env, napi_callback_info info) { return define_domain_with(env, info, 0); }
/* defineEdwardsDomain(ctx, p, a, d, n, gx, gy) -> curve id (ellgpu_curve_define_edwards_domain) */
static napi_value fn_define_edwards_domain(napi_env env, napi_callback_info info) { return define_domain_with(env, info, 1); }
/* destroyContext(ctx): releases the context's device memory and streams (ellgpu_ctx_destroy) and the
 * addon's pin on the external; any later call with that external throws.  Refused while Promise-form
 * batches are in flight (a worker thread is inside the context). */
static napi_value fn_destroy(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 1; napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void* p = NULL;
  napi_value u; napi_get_undefined(env, &u);
  if (argc < 1 || napi_get_value_external(env, argv[0], &p) != napi_ok || !p) THROW(env, "destroyContext(ctx)");
  int i = ctx_slot((ellgpu_ctx*)p);
  if (i < 0) return u;                                  /* destroyed already */
  if (g_jobs_in_flight > 0) THROW(env, "ellgpu: batches are in flight on a worker thread; destroy the context when their Promises have settled");
  L.ctx_destroy(g_ctx[i].c);
  napi_delete_reference(env, g_ctx[i].pin);
  g_ctx[i].c = NULL; g_ctx[i].pin = NULL;
  return u;
}

/* defer(ctx) / collect(ctx): the split form of a few-item call (ellgpu_ctx_defer / _collect) */
static napi_value defer_common(napi_env env, napi_callback_info info, int collect) {
  if (!need_lib(env)) return NULL;
  size_t argc = 1; napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  if ((collect ? L.ctx_collect : L.ctx_defer)(c) != 0) return lib_error(env);
  napi_value u; napi_get_undefined(env, &u); return u;
}
static napi_value fn_defer(napi_env e, napi_callback_info i) { return defer_common(e, i, 0); }
static napi_value fn_collect(napi_env e, napi_callback_info i) { return defer_common(e, i, 1); }

/* combBits(ctx, curve) -> window width of the curve's fixed-base table on this context (0: not
 * built yet; narrower than the default when the device could not hold it: ellgpu_ctx_comb_bits) */
static napi_value fn_comb_bits(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 2; napi_value argv[2]; int32_t curve = 0;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  if (argc < 2 || napi_get_value_int32(env, argv[1], &curve) != napi_ok) THROW(env, "combBits(ctx, curve)");
  int v = L.ctx_comb_bits(c, curve);
  if (v < 0) return lib_error(env);
  napi_value r; CHECK(env, napi_create_int32(env, v, &r)); return r;
}

/* ---- fixed-base tables of caller-chosen points (ellgpu_base_*): host memory throughout ----
 * defineBase(ctx, curve, xy|null, windowBits) -> handle; releaseBase(ctx, base);
 * baseInfo(ctx, base) -> {curve, windowBits, tableBytes}; mulBase(ctx, base, k) -> {xy, inf};
 * mulBase2(ctx, base1, base2, k1, k2) -> {xy, inf}.  The rows' width is the width of the base's
 * curve, asked of the library (ellgpu_base_info).
 * defineEdBase(ctx, curve, xy|null, windowBits) -> handle: the same for ed25519 and user-defined
 * Edwards ids (ellgpu_ed_base_define); its handles go to the calls above unchanged. */
static napi_value define_base_of(napi_env env, napi_callback_info info, int ed) {
  if (!need_lib(env)) return NULL;
  size_t argc = 4; napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 4) THROW(env, "defineBase(ctx, curve, xy|null, windowBits)");
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  int32_t curve, wb;
  if (napi_get_value_int32(env, argv[1], &curve) != napi_ok || napi_get_value_int32(env, argv[3], &wb) != napi_ok)
    THROW(env, "defineBase(ctx, curve, xy|null, windowBits)");
  const uint8_t* xy; size_t l;
  if (!get_buf(env, argv[2], &xy, &l, 1)) return NULL;
  int B = L.field_bytes(curve);
  if (xy && B > 0 && l != 2 * (size_t)B) THROW(env, "defineBase: xy is x || y in the curve's coordinate width");
  int h = -1;
  if ((ed ? L.ed_base_define : L.base_define)(c, curve, xy, wb, &h) != 0) return lib_error(env);
  napi_value v; CHECK(env, napi_create_int32(env, h, &v));
  return v;
}
static napi_value fn_define_base(napi_env env, napi_callback_info info) { return define_base_of(env, info, 0); }
static napi_value fn_define_ed_base(napi_env env, napi_callback_info info) { return define_base_of(env, info, 1); }
static napi_value fn_release_base(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 2; napi_value argv[2]; int32_t base;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  if (argc < 2 || napi_get_value_int32(env, argv[1], &base) != napi_ok) THROW(env, "releaseBase(ctx, base)");
  if (L.base_release(c, base) != 0) return lib_error(env);
  return NULL;
}
static napi_value fn_base_info(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 2; napi_value argv[2]; int32_t base;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ellgpu_ctx* c = get_ctx(env, argv[0]); if (!c) return NULL;
  if (argc < 2 || napi_get_value_int32(env, argv[1], &base) != napi_ok) THROW(env, "baseInfo(ctx, base)");
  int curve = -1, bits = 0; uint64_t bytes = 0;
  if (L.base_info(c, base, &curve, &bits, &bytes) != 0) return lib_error(env);
  napi_value o, v;
  CHECK(env, napi_create_object(env, &o));
  CHECK(env, napi_create_int32(env, curve, &v)); CHECK(env, napi_set_named_property(env, o, "curve", v));
  CHECK(env, napi_create_int32(env, bits, &v)); CHECK(env, napi_set_named_property(env, o, "windowBits", v));
  CHECK(env, napi_create_double(env, (double)bytes, &v)); CHECK(env, napi_set_named_property(env, o, "tableBytes", v));
  return o;
}
/* ---- batch operations: one descriptor each ---------------------------------------------
 * An operation is stated once: a row of ops[] below -- its names, the argument list of its
 * synchronous export, its result properties -- with a `shape` (item count and result lengths from
 * the operands, or the refusal) and a `call` (the one place that names its C ABI entry).  The
 * synchronous exports are one callback, op_sync, which gets the row through napi_create_function's
 * data pointer; callAsync(op, ...) looks the row up by id and runs the same shape and call, the
 * call on a worker thread. */
typedef struct op_desc op_desc;
typedef struct {
  const op_desc* d;
  ellgpu_ctx* ctx;
  int curve, B, NB;            /* the curve id, its coordinate and scalar widths in bytes */
  int hl, mb, i0, i1;          /* hashLen, msgBits and the operation's two integers */
  int promise;                 /* 1 in callAsync: the few places where the two forms differ ask */
  const uint8_t* in[4]; size_t len[4];
  size_t n, ol[4];             /* set by shape: the item count, the result lengths */
  uint8_t* out[4];
} op_call;
enum {
  F_OWN_OUT = 1,      /* the synchronous form takes trailing (xy, inf) result Buffers of the caller's */
  F_BARE = 2,         /* the synchronous form returns its one Buffer, not an object */
  F_BASE_CURVE = 4,   /* the synchronous form has no curve argument: the curve is the base handle's (i0) */
  F_X25519 = 8,       /* callAsync ignores its curve argument: curve25519 */
  F_WIDE_ENC = 16,    /* result rows at the curve's own width: written through rows of ECDH_ENC_MAX bytes */
  F_ECDH = 32,        /* reachable through customEcdh(ctx, op, ...) */
  F_BY_OP = 64,       /* customEcdh itself: the row is chosen by its op argument */
  F_NONCES = 128,     /* a signing call with supplied nonces (operand 2) */
  F_WIRE = 256,       /* a derive call whose peer keys are encodings of i0 bytes */
};
struct op_desc {
  const char* name;               /* key of addon.ops and, where `args` is set, the synchronous export */
  int id;                         /* callAsync's op; -1: no Promise form */
  const char* args;               /* the synchronous export's arguments after ctx, one letter each:
                                   *   c curve  h hashLen  m msgBits  i, j the integers i0, i1  b a boolean into i0
                                   *   k, l base handles into i0, i1  o customEcdh's op  0..3 the operand Buffers
                                   * a '?' after a letter: null / undefined allowed (Buffers), or read leniently
                                   * (a value of another type leaves 0).  NULL: no export of its own. */
  const char* names[5];           /* the result properties, in output order */
  const char* (*shape)(op_call*); /* NULL, or the refusal's message */
  int (*call)(const op_call*);
  int flags;
  int min_argc;                   /* fewer arguments than this throw `usage` */
  const char* usage;              /* thrown too for an integer argument that is none, unless `badint` is set */
  const char* badint;
};

#define MISMATCH "buffer length mismatch"
#define XY(c) ((c)->n * 2 * (size_t)(c)->B)
static const char* outs(op_call* c, size_t l0, size_t l1, size_t l2, size_t l3) {
  c->ol[0] = l0; c->ol[1] = l1; c->ol[2] = l2; c->ol[3] = l3;
  return NULL;
}
/* n from operand 0: hashes of hashLen bytes (hashLen > 0 is the caller's check) */
static const char* per_hash(op_call* c) {
  if (!c->in[0] || c->len[0] % (size_t)c->hl) return "hash buffer length is not a multiple of hashLen";
  c->n = c->len[0] / (size_t)c->hl;
  return NULL;
}
/* n from operand 0: scalars of B bytes */
static const char* per_scalar(op_call* c) {
  if (c->B <= 0) return "unknown curve id";
  if (!c->in[0] || c->len[0] % (size_t)c->B) return "scalar buffer length is not a multiple of the field width";
  c->n = c->len[0] / (size_t)c->B;
  return NULL;
}
/* n from operand 0: points of 2 * w bytes */
static const char* per_point(op_call* c, size_t w, const char* msg) {
  if (!c->in[0] || c->len[0] % (2 * w)) return msg;
  c->n = c->len[0] / (2 * w);
  return NULL;
}
/* offsets of n messages in a buffer of lm bytes: an aligned Buffer of n + 1 non-decreasing uint64 (NULL if fine) */
static const char* bad_offsets(const uint8_t* off, size_t loff, size_t n, size_t lm) {
  if (loff != (n + 1) * 8 || ((uintptr_t)off & 7)) return "offsets must be an aligned Buffer of n+1 uint64";
  if (((const uint64_t*)off)[n] > lm) return "offsets exceed the message buffer";
  for (size_t i = 0; i < n; i++)        /* the kernels take len = off[i+1] - off[i]: must not wrap */
    if (((const uint64_t*)off)[i] > ((const uint64_t*)off)[i + 1]) return "offsets must be non-decreasing";
  return NULL;
}
/* the n messages of an EdDSA call: operand 0 cut by the offsets in operand 1, or into rows of i1 bytes */
static const char* messages(const op_call* c) {
  if (c->in[1]) return bad_offsets(c->in[1], c->len[1], c->n, c->len[0]);
  return (size_t)c->i1 * c->n > c->len[0] ? "message buffer too short" : NULL;
}

static const char* shape_mul_fixed(op_call* c) {
  const char* bad = per_scalar(c);
  return bad ? bad : outs(c, XY(c), c->n, 0, 0);
}
static const char* shape_mul_var(op_call* c) {
  const char* bad = per_scalar(c); if (bad) return bad;
  if (!c->in[1] || c->len[1] != XY(c)) return "point buffer length mismatch";
  return outs(c, XY(c), c->n, 0, 0);
}
static const char* shape_mul_add2(op_call* c) {
  const char* bad = per_scalar(c); if (bad) return bad;
  if ((c->in[1] && c->len[1] != XY(c)) || !c->in[2] || c->len[2] != c->len[0] || !c->in[3] || c->len[3] != XY(c)) return MISMATCH;
  return outs(c, XY(c), c->n, 0, 0);
}
static const char* shape_mul_base(op_call* c) {
  if (c->B <= 0) return "unknown curve id";
  if (!c->in[0] || c->len[0] % (size_t)c->B) return MISMATCH;
  c->n = c->len[0] / (size_t)c->B;
  return outs(c, XY(c), c->n, 0, 0);
}
static const char* shape_mul_base2(op_call* c) {
  const char* bad = shape_mul_base(c); if (bad) return bad;
  return c->in[1] && c->len[1] == c->len[0] ? NULL : MISMATCH;
}
static const char* shape_verify(op_call* c) {
  if (c->B <= 0 || c->hl <= 0) return "bad curve / hashLen";
  const char* bad = per_hash(c); if (bad) return bad;
  if (!c->in[1] || !c->in[2] || !c->in[3] || c->len[1] != c->n * (size_t)c->NB || c->len[2] != c->len[1] || c->len[3] != XY(c))
    return MISMATCH;
  return outs(c, c->n, c->n, 0, 0);
}
static const char* shape_verify_base(op_call* c) {
  if (c->NB <= 0) return "unknown curve id";
  if (c->hl <= 0 || per_hash(c)) return MISMATCH;
  if (!c->in[1] || !c->in[2] || c->in[3] || c->len[1] != c->n * (size_t)c->NB || c->len[2] != c->len[1]) return MISMATCH;
  return outs(c, c->n, 0, 0, 0);
}
static const char* shape_x25519(op_call* c) {
  if (!c->in[0] || !c->in[1] || c->len[0] % 32 || c->len[1] != c->len[0]) return MISMATCH;
  c->n = c->len[0] / 32;
  return outs(c, c->n * 32, c->n, 0, 0);
}
static const char* shape_decompress(op_call* c) {
  if (c->B <= 0) return "unknown curve id";
  if (!c->in[0] || !c->in[1] || c->len[0] % (size_t)c->B || c->len[1] != c->len[0] / (size_t)c->B) return MISMATCH;
  c->n = c->len[1];
  return outs(c, XY(c), c->n, 0, 0);
}
/* private keys (and, with F_NONCES, nonces) of w bytes per hash -> r, s, recid, ok */
static const char* sign_rows(op_call* c, size_t w) {
  const char* bad = per_hash(c); if (bad) return bad;
  if (!c->in[1] || c->len[1] != c->n * w) return MISMATCH;
  if ((c->d->flags & F_NONCES) && (!c->in[2] || c->len[2] != c->len[1])) return MISMATCH;
  return outs(c, c->n * w, c->n * w, c->n, c->n);
}
static const char* shape_sign(op_call* c) {
  if (c->NB <= 0 || c->hl <= 0) return "bad curve / hashLen";
  return sign_rows(c, (size_t)c->NB);
}
static const char* shape_custom_sign(op_call* c) {      /* 32-byte rows; callAsync asks the library for the width */
  if (c->hl <= 0) return "bad hashLen";
  return sign_rows(c, c->promise ? (size_t)c->NB : 32);
}
static const char* shape_recover(op_call* c) {
  if (c->B <= 0 || c->NB <= 0 || c->hl <= 0) return "bad curve / hashLen";
  const char* bad = per_hash(c); if (bad) return bad;
  if (!c->in[1] || !c->in[2] || !c->in[3] || c->len[1] != c->n * (size_t)c->NB || c->len[2] != c->len[1] || c->len[3] != c->n)
    return MISMATCH;
  return outs(c, XY(c), c->n, 0, 0);
}
static const char* shape_decode(op_call* c) {
  if (c->B <= 0 || c->i0 <= 0) return "bad curve / encLen";
  if (!c->in[0] || c->len[0] % (size_t)c->i0) return "enc buffer length is not a multiple of encLen";
  c->n = c->len[0] / (size_t)c->i0;
  return outs(c, XY(c), c->n, 0, 0);
}
static const char* shape_encode(op_call* c) {
  if (c->B <= 0) return "unknown curve id";
  const char* bad = per_point(c, (size_t)c->B, "xy buffer length is not a multiple of 2 * fieldBytes"); if (bad) return bad;
  /* the library's rule for the encoded length: SEC1 for the short curves, 32 bytes for ed25519 */
  size_t el = 1 + (c->i0 ? 1 : 2) * (size_t)c->B;
  if (curve_id_of("ed25519") == c->curve) el = 32;
  return outs(c, c->n * el, 0, 0, 0);
}
static const char* shape_validate(op_call* c) {
  if (c->B <= 0) return "unknown curve id";
  const char* bad = per_point(c, (size_t)c->B, "xy buffer length is not a multiple of 2 * fieldBytes"); if (bad) return bad;
  if (c->in[1] && c->len[1] != c->n) return MISMATCH;
  return outs(c, c->n, 0, 0, 0);
}
static const char* shape_point_add(op_call* c) {
  if (c->B <= 0) return "unknown curve id";
  if (per_point(c, (size_t)c->B, MISMATCH) || !c->in[2] || c->len[2] != c->len[0]) return MISMATCH;
  if ((c->in[1] && c->len[1] != c->n) || (c->in[3] && c->len[3] != c->n)) return MISMATCH;
  return outs(c, XY(c), c->n, 0, 0);
}
static const char* shape_sig_from_der(op_call* c) {
  if (c->NB <= 0 || c->i0 <= 0) return "bad curve / stride";
  if (!c->in[1] || c->len[1] % 4 || ((uintptr_t)c->in[1] & 3)) return "lens must be an aligned Buffer of uint32";
  c->n = c->len[1] / 4;
  if (!c->in[0] || c->len[0] != c->n * (size_t)c->i0) return MISMATCH;
  return outs(c, c->n * (size_t)c->NB, c->n * (size_t)c->NB, c->n, 0);
}
static const char* shape_sig_to_der(op_call* c) {
  if (c->NB <= 0) return "unknown curve id";
  if (!c->in[0] || !c->in[1] || c->len[0] % (size_t)c->NB || c->len[1] != c->len[0]) return MISMATCH;
  c->n = c->len[0] / (size_t)c->NB;
  return outs(c, c->n * (2 * (size_t)c->NB + 9), c->n * 4, 0, 0);
}
static const char* shape_verify_wire(op_call* c) {
  if (c->hl <= 0 || c->i0 <= 0 || c->i1 <= 0) return "bad hashLen / stride / keyLen";
  const char* bad = per_hash(c); if (bad) return bad;
  if (!c->in[2] || c->len[2] != c->n * 4 || ((uintptr_t)c->in[2] & 3)) return "lens must be an aligned Buffer of n uint32";
  if (!c->in[1] || !c->in[3] || c->len[1] != c->n * (size_t)c->i0 || c->len[3] != c->n * (size_t)c->i1) return MISMATCH;
  return outs(c, c->n, c->n, 0, 0);
}
static const char* shape_eddsa_verify(op_call* c) {
  if (!c->in[2] || !c->in[3] || c->len[2] % 64 || c->len[3] != c->len[2] / 2) return MISMATCH;
  c->n = c->len[2] / 64;
  const char* bad = messages(c);
  return bad ? bad : outs(c, c->n, c->n, 0, 0);
}
static const char* shape_eddsa_sign(op_call* c) {
  if (!c->in[2] || c->len[2] % 32) return "secrets must be n x 32 bytes";
  c->n = c->len[2] / 32;
  const char* bad = messages(c);
  return bad ? bad : outs(c, c->n * 64, c->n * 32, 0, 0);
}
static const char* shape_eddsa_verify_base(op_call* c) {
  if (!c->in[2] || c->in[3] || c->len[2] % 64 || (c->promise && !c->in[1])) return MISMATCH;
  c->n = c->len[2] / 64;
  if (!c->in[1] && c->i1 < 0) return "message buffer too short";
  const char* bad = messages(c);
  return bad ? bad : outs(c, c->n, c->n, 0, 0);
}
/* The key side on user-defined short, Montgomery and Edwards curves (reached synchronously through
 * customEcdh): scalars and coordinates are 32 bytes. */
static const char* shape_derive(op_call* c) {
  const int wire = c->d->flags & F_WIRE;
  if (!c->in[0] || !c->in[1] || c->len[0] % 32 || (wire && c->i0 <= 0)) return MISMATCH;
  c->n = c->len[0] / 32;
  if (c->len[1] != c->n * (wire ? (size_t)c->i0 : 64)) return MISMATCH;
  return outs(c, c->n * 32, c->n, wire ? c->n : 0, 0);
}
static const char* shape_custom_validate(op_call* c) {
  if (per_point(c, 32, MISMATCH) || (c->in[1] && c->len[1] != c->n)) return MISMATCH;
  return outs(c, c->n, 0, 0, 0);
}
static const char* shape_ed_validate(op_call* c) {      /* operand 1: the order, 32 bytes, or null */
  if (per_point(c, 32, MISMATCH) || (c->in[1] && c->len[1] != 32)) return MISMATCH;
  return outs(c, c->n, 0, 0, 0);
}
/* The library writes the encoders' rows at the CURVE's width, which this addon cannot ask it for
 * (index.js records it when the curve is defined and refuses another): so the call never gets the
 * caller-sized result buffer.  It writes into n rows of ECDH_ENC_MAX bytes -- the widest a curve
 * below 2^256 has -- and the result is cut from those (F_WIDE_ENC): a wrong i1 gives wrong bytes,
 * never a write past the end. */
#define ECDH_ENC_MAX 65
static const char* shape_custom_encode(op_call* c) {
  /* the row width is the curve's: not a caller's choice to get wrong silently */
  if (c->i1 <= 0 || c->i1 > 32) return "customEncodePoints: coordBytes must be 1..32";
  if (per_point(c, 32, MISMATCH)) return MISMATCH;
  return outs(c, c->n * (1 + (c->i0 ? 1 : 2) * (size_t)c->i1), 0, 0, 0);
}
static const char* shape_ed_decompress(op_call* c) {
  if (!c->in[0] || !c->in[1] || c->len[0] % 32 || c->len[1] != c->len[0] / 32) return MISMATCH;
  c->n = c->len[1];
  return outs(c, c->n * 64, c->n, 0, 0);
}
static const char* shape_ed_decode(op_call* c) {
  if (!c->in[0] || c->in[1] || c->i0 <= 0 || c->len[0] % (size_t)c->i0) return MISMATCH;
  c->n = c->len[0] / (size_t)c->i0;
  return outs(c, c->n * 64, c->n, 0, 0);
}
static const char* shape_mont_pair(op_call* c) {
  if (!c->in[0] || !c->in[1] || c->len[0] % 32 || c->len[1] != c->len[0]) return MISMATCH;
  c->n = c->len[0] / 32;
  return outs(c, c->n * 32, c->n, 0, 0);
}
static const char* shape_mont_validate(op_call* c) {
  if (!c->in[0] || c->in[1] || c->len[0] % 32) return MISMATCH;
  c->n = c->len[0] / 32;
  return outs(c, c->n, 0, 0, 0);
}

static int call_mul_fixed(const op_call* c) { return L.mul_fixed(c->ctx, c->curve, c->n, c->in[0], c->out[0], c->out[1]); }
static int call_mul_var(const op_call* c) { return L.mul_var(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0], c->out[1]); }
static int call_mul_add2(const op_call* c) {
  return L.mul_add2(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->in[2], c->in[3], c->out[0], c->out[1]);
}
static int call_mul_base(const op_call* c) { return L.mul_base(c->ctx, c->i0, c->n, c->in[0], c->out[0], c->out[1], 0, NULL); }
static int call_mul_base2(const op_call* c) {
  return L.mul_base2(c->ctx, c->i0, c->i1, c->n, c->in[0], c->in[1], c->out[0], c->out[1], 0, NULL);
}
static int call_verify(const op_call* c) {
  return L.ecdsa_verify(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], c->in[2], c->in[3], c->out[0], c->out[1]);
}
static int call_custom_ed_verify(const op_call* c) {
  return L.custom_ed_verify(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], c->in[2], c->in[3], c->out[0], c->out[1]);
}
static int call_verify_base(const op_call* c) {
  return L.ecdsa_verify_base(c->ctx, c->i0, c->n, c->in[0], c->hl, c->mb, c->in[1], c->in[2], c->out[0], 0, NULL);
}
static int call_x25519(const op_call* c) { return L.x25519(c->ctx, c->n, c->in[0], c->in[1], c->out[0], c->out[1]); }
static int call_x25519_derive(const op_call* c) { return L.x25519_derive(c->ctx, c->n, c->in[0], c->in[1], c->out[0], c->out[1]); }
static int call_decompress(const op_call* c) { return L.decompress(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0], c->out[1]); }
static int call_custom_decompress(const op_call* c) {
  return L.custom_decompress(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0], c->out[1]);
}
static int call_sign(const op_call* c) {
  return L.ecdsa_sign(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], c->in[2], c->i0, c->out[0], c->out[1], c->out[2], c->out[3]);
}
static int call_sign_det(const op_call* c) {
  return L.ecdsa_sign_det(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], c->i0, c->out[0], c->out[1], c->out[2], c->out[3]);
}
static int call_custom_sign(const op_call* c) {
  return L.custom_sign(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], c->in[2], c->i0, c->out[0], c->out[1], c->out[2], c->out[3]);
}
static int call_custom_sign_det(const op_call* c) {
  return L.custom_sign_det(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], c->i1, c->i0, c->out[0], c->out[1], c->out[2], c->out[3]);
}
static int call_custom_ed_sign(const op_call* c) {
  return L.custom_ed_sign(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], c->in[2], c->i0, c->out[0], c->out[1], c->out[2], c->out[3]);
}
static int call_custom_ed_sign_det(const op_call* c) {
  return L.custom_ed_sign_det(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], c->i1, c->i0, c->out[0], c->out[1], c->out[2], c->out[3]);
}
static int call_recover(const op_call* c) {
  return L.ecdsa_recover(c->ctx, c->curve, c->n, c->in[0], c->hl, c->in[1], c->in[2], c->in[3], c->out[0], c->out[1]);
}
static int call_custom_recover(const op_call* c) {
  return L.custom_recover(c->ctx, c->curve, c->n, c->in[0], c->hl, c->in[1], c->in[2], c->in[3], c->out[0], c->out[1]);
}
static int call_decode_points(const op_call* c) { return L.decode_points(c->ctx, c->curve, c->n, c->in[0], (size_t)c->i0, c->out[0], c->out[1]); }
static int call_custom_decode_points(const op_call* c) {
  return L.custom_decode_points(c->ctx, c->curve, c->n, c->in[0], (size_t)c->i0, c->out[0], c->out[1]);
}
static int call_encode_points(const op_call* c) { return L.encode_points(c->ctx, c->curve, c->n, c->in[0], c->i0, c->out[0]); }
static int call_validate(const op_call* c) { return L.validate(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->i0, c->out[0]); }
static int call_point_add(const op_call* c) {
  return L.point_add(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->in[2], c->in[3], c->out[0], c->out[1]);
}
static int call_sig_from_der(const op_call* c) {
  return L.sig_from_der(c->ctx, c->curve, c->n, c->in[0], (size_t)c->i0, (const uint32_t*)c->in[1], c->out[0], c->out[1], c->out[2]);
}
static int call_sig_to_der(const op_call* c) {
  return L.sig_to_der(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0], 2 * (size_t)c->NB + 9, (uint32_t*)c->out[1]);
}
static int call_verify_wire(const op_call* c) {
  return L.verify_wire(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], (size_t)c->i0, (const uint32_t*)c->in[2], c->in[3],
                       (size_t)c->i1, c->out[0], c->out[1]);
}
static int call_custom_verify_wire(const op_call* c) {
  return L.custom_verify_wire(c->ctx, c->curve, c->n, c->in[0], c->hl, c->mb, c->in[1], (size_t)c->i0, (const uint32_t*)c->in[2],
                              c->in[3], (size_t)c->i1, c->out[0], c->out[1]);
}
static int call_eddsa_verify(const op_call* c) {
  return L.eddsa_verify(c->ctx, c->n, c->in[0], (const uint64_t*)c->in[1], (size_t)c->i1, c->in[2], c->in[3], c->out[0], c->out[1]);
}
static int call_eddsa_sign(const op_call* c) {
  return L.eddsa_sign(c->ctx, c->n, c->in[2], c->in[0], (const uint64_t*)c->in[1], (size_t)c->i1, c->out[0], c->out[1]);
}
static int call_eddsa_verify_base(const op_call* c) {
  return L.eddsa_verify_base(c->ctx, c->i0, c->n, c->in[0], (const uint64_t*)c->in[1], (size_t)c->i1, c->in[2], c->out[0], c->out[1], 0, NULL);
}
static int call_custom_derive(const op_call* c) { return L.custom_derive(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0], c->out[1]); }
static int call_custom_derive_wire(const op_call* c) {
  return L.custom_derive_wire(c->ctx, c->curve, c->n, c->in[0], c->in[1], (size_t)c->i0, c->out[0], c->out[1], c->out[2]);
}
static int call_custom_validate(const op_call* c) { return L.custom_validate(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->i0, c->out[0]); }
static int call_custom_encode_points(const op_call* c) { return L.custom_encode_points(c->ctx, c->curve, c->n, c->in[0], c->i0, c->out[0]); }
static int call_custom_mont_ladder(const op_call* c) { return L.custom_mont_ladder(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0], c->out[1]); }
static int call_custom_mont_validate(const op_call* c) { return L.custom_mont_validate(c->ctx, c->curve, c->n, c->in[0], c->out[0]); }
static int call_custom_mont_derive(const op_call* c) { return L.custom_mont_derive(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0], c->out[1]); }
static int call_custom_ed_decompress(const op_call* c) {
  return L.custom_ed_decompress(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->i0, c->out[0], c->out[1]);
}
static int call_custom_ed_decode_points(const op_call* c) {
  return L.custom_ed_decode_points(c->ctx, c->curve, c->n, c->in[0], (size_t)c->i0, c->out[0], c->out[1]);
}
static int call_custom_ed_validate(const op_call* c) { return L.custom_ed_validate(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0]); }
static int call_custom_ed_derive(const op_call* c) { return L.custom_ed_derive(c->ctx, c->curve, c->n, c->in[0], c->in[1], c->out[0], c->out[1]); }
static int call_custom_ed_derive_wire(const op_call* c) {
  return L.custom_ed_derive_wire(c->ctx, c->curve, c->n, c->in[0], c->in[1], (size_t)c->i0, c->out[0], c->out[1], c->out[2]);
}
static int call_custom_ed_encode_points(const op_call* c) { return L.custom_ed_encode_points(c->ctx, c->curve, c->n, c->in[0], c->i0, c->out[0]); }

/* The table.  Above each row: the synchronous export and, after `|`, callAsync's operands
 * (b0..b3; i0, i1) where the operation has a Promise form; then the result.
 * Where the two forms differ (tests/golden/addon_forms.json pins each):
 *   - only mulFixed / mulVar / mulAdd2 take caller-supplied result Buffers, and only synchronously;
 *   - synchronous mulBase, mulBase2 and ecdsaVerifyBase take the curve from ellgpu_base_info (and
 *     eddsaVerifyBase takes none); callAsync uses the curve argument index.js passes;
 *   - callAsync x25519 forces curve 7;
 *   - a refusal of the operands is thrown with its own message synchronously, and as the one
 *     `callAsync: buffer length mismatch` by callAsync;
 *   - callAsync eddsaVerifyBase needs the offsets; the synchronous form takes null and msgLen;
 *   - customSign / customSignDet / customEdSign / customEdSignDet rows are 32 bytes synchronously and
 *     the width ellgpu_curve_order_bytes reports in callAsync (32 on every id they accept);
 *   - encodePoints and validate return a bare Buffer. */
#define VERIFY_USAGE "ecdsaVerify(ctx, curve, hash, hashLen, msgBits, r, s, pub)"
#define RECOVER_USAGE "ecdsaRecover(ctx, curve, hash, hashLen, r, s, recid)"
#define WIRE_USAGE "ecdsaVerifyWire(ctx, curve, hash, hashLen, msgBits, der, stride, lens, keys, keyLen)"
#define CUSTOM_SIGN_USAGE "customSign(ctx, curve, hash, hashLen, msgBits, priv, nonces, canonical)"
#define CUSTOM_SIGN_DET_USAGE "customSignDet(ctx, curve, hash, hashLen, msgBits, priv, drbgHash, canonical)"
static const op_desc ops[] = {
  /* mulFixed(ctx, curve, k[, xy, inf]) | k -> {xy, inf} */
  {"mulFixed", 0, "c0", {"xy", "inf"}, shape_mul_fixed, call_mul_fixed, F_OWN_OUT, 0, "curve id expected", 0},
  /* mulVar(ctx, curve, k, xy[, xy, inf]) | k, xy -> {xy, inf} */
  {"mulVar", 1, "c01", {"xy", "inf"}, shape_mul_var, call_mul_var, F_OWN_OUT, 0, "curve id expected", 0},
  /* mulAdd2(ctx, curve, k1, p1|null, k2, p2[, xy, inf]) | k1, p1|null, k2, p2 -> {xy, inf}; p1 null: the generator */
  {"mulAdd2", 2, "c01?23", {"xy", "inf"}, shape_mul_add2, call_mul_add2, F_OWN_OUT, 0, "curve id expected", 0},
  /* ecdsaVerify(ctx, curve, hash, hashLen, msgBits, r, s, pub) | hash, r, s, pub -> {ok, status} */
  {"ecdsaVerify", 3, "c0hm123", {"ok", "status"}, shape_verify, call_verify, 0, 0, VERIFY_USAGE, 0},
  /* x25519(ctx, k, x) | k, x -> {x, inf} */
  {"x25519", 4, "01", {"x", "inf"}, shape_x25519, call_x25519, F_X25519, 0, 0, 0},
  /* x25519Derive(ctx, k, x) -> {x, status}: KeyPair#derive on curve25519, validate + ladder in one call */
  {"x25519Derive", -1, "01", {"x", "status"}, shape_x25519, call_x25519_derive, 0, 0, 0, 0},
  /* ecdsaSignDet(ctx, curve, hash, hashLen, msgBits, priv, canonical) | hash, priv; i0 = canonical -> {r, s, recid, ok} */
  {"ecdsaSignDet", 5, "c0hm1b?", {"r", "s", "recid", "ok"}, shape_sign, call_sign_det, 0, 0,
   "ecdsaSignDet(ctx, curve, hash, hashLen, msgBits, priv, canonical)", 0},
  /* ecdsaSign(ctx, curve, hash, hashLen, msgBits, priv, nonces, canonical) -> {r, s, recid, ok} */
  {"ecdsaSign", -1, "c0hm12b?", {"r", "s", "recid", "ok"}, shape_sign, call_sign, F_NONCES, 0,
   "ecdsaSign(ctx, curve, hash, hashLen, msgBits, priv, nonces, canonical)", 0},
  /* ecdsaRecover(ctx, curve, hash, hashLen, r, s, recid) | hash, r, s, recid -> {xy, status} */
  {"ecdsaRecover", 6, "c0h123", {"xy", "status"}, shape_recover, call_recover, 0, 0, RECOVER_USAGE, 0},
  /* ecdsaVerifyWire(ctx, curve, hash, hashLen, msgBits, der, stride, lens, keys, keyLen) | hash, der, lens, keys;
   * i0 = stride, i1 = keyLen -> {ok, err}; lens: n little-endian uint32 */
  {"ecdsaVerifyWire", 7, "c0hm1i23j", {"ok", "err"}, shape_verify_wire, call_verify_wire, 0, 0, WIRE_USAGE, 0},
  /* decodePoints(ctx, curve, enc, encLen) | enc; i0 = encLen -> {xy, status} */
  {"decodePoints", 8, "c0i", {"xy", "status"}, shape_decode, call_decode_points, 0, 0, "decodePoints(ctx, curve, enc, encLen)", 0},
  /* the same three, and decompress, on a user-defined short curve / domain (ellgpu_custom_*) */
  {"customVerifyWire", 9, "c0hm1i23j", {"ok", "err"}, shape_verify_wire, call_custom_verify_wire, 0, 0, WIRE_USAGE, 0},
  {"customRecover", 10, "c0h123", {"xy", "status"}, shape_recover, call_custom_recover, 0, 0, RECOVER_USAGE, 0},
  {"customDecodePoints", -1, "c0i", {"xy", "status"}, shape_decode, call_custom_decode_points, 0, 0, "decodePoints(ctx, curve, enc, encLen)", 0},
  /* decompress(ctx, curve, v, odd) -> {xy, ok} (ok 1 = point); customDecompress -> {xy, status} (status 0 = point) */
  {"decompress", -1, "c01", {"xy", "ok"}, shape_decompress, call_decompress, 0, 0, "curve id expected", 0},
  {"customDecompress", -1, "c01", {"xy", "status"}, shape_decompress, call_custom_decompress, 0, 0, "curve id expected", 0},
  /* customSign(ctx, curve, hash, hashLen, msgBits, priv, nonces, canonical) | hash, priv, nonces; i0 = canonical
   * customSignDet(ctx, curve, hash, hashLen, msgBits, priv, drbgHash, canonical) | hash, priv; i0 = canonical, i1 = drbgHash
   * (0 sha256, 1 sha384, 2 sha512) -> {r, s, recid, ok}: EC#sign on a user-defined domain */
  {"customSign", 11, "c0hm12b?", {"r", "s", "recid", "ok"}, shape_custom_sign, call_custom_sign, F_NONCES, 8, CUSTOM_SIGN_USAGE, 0},
  {"customSignDet", 12, "c0hm1jb?", {"r", "s", "recid", "ok"}, shape_custom_sign, call_custom_sign_det, 0, 8, CUSTOM_SIGN_DET_USAGE, 0},
  /* The key side on a user-defined short curve, synchronously through customEcdh:
   * 13 customDerive | priv, pubXY -> {x, status}      14 customDeriveWire | priv, enc; i0 = key length -> {x, status, err}
   * 15 customValidate | xy, inf|null; i0 = checkOrder -> {status}
   * 16 customEncodePoints | xy; i0 = compact, i1 = p.byteLength() -> {enc} */
  {"customDerive", 13, 0, {"x", "status"}, shape_derive, call_custom_derive, F_ECDH, 0, 0, 0},
  {"customDeriveWire", 14, 0, {"x", "status", "err"}, shape_derive, call_custom_derive_wire, F_ECDH | F_WIRE, 0, 0, 0},
  {"customValidate", 15, 0, {"status"}, shape_custom_validate, call_custom_validate, F_ECDH, 0, 0, 0},
  {"customEncodePoints", 16, 0, {"enc"}, shape_custom_encode, call_custom_encode_points, F_ECDH | F_WIDE_ENC, 0, 0, 0},
  /* on a user-defined Montgomery curve: 17 customMontLadder | k, x -> {x, inf}  18 customMontValidate | x -> {status}
   * 19 customMontDerive | priv, x -> {x, status} */
  {"customMontLadder", 17, 0, {"x", "inf"}, shape_mont_pair, call_custom_mont_ladder, F_ECDH, 0, 0, 0},
  {"customMontValidate", 18, 0, {"status"}, shape_mont_validate, call_custom_mont_validate, F_ECDH, 0, 0, 0},
  {"customMontDerive", 19, 0, {"x", "status"}, shape_mont_pair, call_custom_mont_derive, F_ECDH, 0, 0, 0},
  /* on a user-defined Edwards curve: 20 customEdDecompress | v, odd; i0 = fromY -> {xy, status}
   * 21 customEdDecodePoints | enc; i0 = row length -> {xy, status}  22 customEdValidate | xy, order|null -> {status}
   * 23 customEdDerive, 24 customEdDeriveWire, 25 customEdEncodePoints: as 13, 14, 16 */
  {"customEdDecompress", 20, 0, {"xy", "status"}, shape_ed_decompress, call_custom_ed_decompress, F_ECDH, 0, 0, 0},
  {"customEdDecodePoints", 21, 0, {"xy", "status"}, shape_ed_decode, call_custom_ed_decode_points, F_ECDH, 0, 0, 0},
  {"customEdValidate", 22, 0, {"status"}, shape_ed_validate, call_custom_ed_validate, F_ECDH, 0, 0, 0},
  {"customEdDerive", 23, 0, {"x", "status"}, shape_derive, call_custom_ed_derive, F_ECDH, 0, 0, 0},
  {"customEdDeriveWire", 24, 0, {"x", "status", "err"}, shape_derive, call_custom_ed_derive_wire, F_ECDH | F_WIRE, 0, 0, 0},
  {"customEdEncodePoints", 25, 0, {"enc"}, shape_custom_encode, call_custom_ed_encode_points, F_ECDH | F_WIDE_ENC, 0, 0, 0},
  /* customEcdh(ctx, op, curve, b0, b1|null, i0, i1) -> the result of op 13..25 */
  {"customEcdh", -1, "oc01?ij", {0}, 0, 0, F_BY_OP, 7, "customEcdh(ctx, op, curve, b0, b1, i0, i1)", 0},
  /* ECDSA on a user-defined Edwards domain: customEdVerify, customEdSign, customEdSignDet as ecdsaVerify, customSign, customSignDet */
  {"customEdVerify", 26, "c0hm123", {"ok", "status"}, shape_verify, call_custom_ed_verify, 0, 0, VERIFY_USAGE, 0},
  {"customEdSign", 27, "c0hm12b?", {"r", "s", "recid", "ok"}, shape_custom_sign, call_custom_ed_sign, F_NONCES, 8, CUSTOM_SIGN_USAGE, 0},
  {"customEdSignDet", 28, "c0hm1jb?", {"r", "s", "recid", "ok"}, shape_custom_sign, call_custom_ed_sign_det, 0, 8, CUSTOM_SIGN_DET_USAGE, 0},
  /* Fixed-base tables of caller-chosen points (handles of defineBase / defineEdBase); rows in the width of the base's curve.
   * mulBase(ctx, base, k) | k; i0 = base      mulBase2(ctx, base1, base2, k1, k2) | k1, k2; i0, i1 = the bases -> {xy, inf} */
  {"mulBase", 29, "k0", {"xy", "inf"}, shape_mul_base, call_mul_base, F_BASE_CURVE, 3, "mulBase(ctx, base, k)", "base handle expected"},
  {"mulBase2", 30, "kl01", {"xy", "inf"}, shape_mul_base2, call_mul_base2, F_BASE_CURVE, 5, "mulBase2(ctx, base1, base2, k1, k2)",
   "base handle expected"},
  /* ecdsaVerifyBase(ctx, base, hashes, hashLen, msgBits, r, s) | hashes, r, s; i0 = base -> {ok}: EC#verify against the key's table */
  {"ecdsaVerifyBase", 31, "k0hm12", {"ok"}, shape_verify_base, call_verify_base, F_BASE_CURVE, 7,
   "ecdsaVerifyBase(ctx, base, hashes, hashLen, msgBits, r, s)", 0},
  /* eddsaVerifyBase(ctx, base, msgs, offsets|null, msgLen, sigs) | msgs, offsets, sigs; i0 = base -> {ok, err}: EDDSA#verify against
   * the table of a defineEdBase handle on ed25519; offsets: n + 1 little-endian uint64 byte offsets into msgs */
  {"eddsaVerifyBase", 32, "i0?1?j?2", {"ok", "err"}, shape_eddsa_verify_base, call_eddsa_verify_base, 0, 6,
   "eddsaVerifyBase(ctx, base, msgs, offsets, msgLen, sigs)", 0},
  /* eddsaVerify(ctx, msgs, offsets|null, msgLen, sigs, pubs) -> {ok, err}      eddsaSign(ctx, msgs, offsets|null, msgLen, secrets)
   * -> {sig: n x 64, pub: n x 32} */
  {"eddsaVerify", -1, "0?1?j?23", {"ok", "err"}, shape_eddsa_verify, call_eddsa_verify, 0, 0, 0, 0},
  {"eddsaSign", -1, "0?1?j?2", {"sig", "pub"}, shape_eddsa_sign, call_eddsa_sign, 0, 0, 0, 0},
  /* encodePoints(ctx, curve, xy, compact) -> Buffer      validate(ctx, curve, xy, inf|null, checkOrder) -> Buffer (status bytes) */
  {"encodePoints", -1, "c0b", {"enc"}, shape_encode, call_encode_points, F_BARE, 0, "encodePoints(ctx, curve, xy, compact)", 0},
  {"validate", -1, "c01?b", {"status"}, shape_validate, call_validate, F_BARE, 0, "validate(ctx, curve, xy, inf|null, checkOrder)", 0},
  /* pointAdd(ctx, curve, xy1, inf1|null, xy2, inf2|null) -> {xy, inf} */
  {"pointAdd", -1, "c01?23?", {"xy", "inf"}, shape_point_add, call_point_add, 0, 0, "pointAdd(ctx, curve, xy1, inf1|null, xy2, inf2|null)", 0},
  /* sigFromDer(ctx, curve, der, stride, lens) -> {r, s, status}      sigToDer(ctx, curve, r, s) -> {der, lens} (stride = der.length / n) */
  {"sigFromDer", -1, "c0i1", {"r", "s", "status"}, shape_sig_from_der, call_sig_from_der, 0, 0, "sigFromDer(ctx, curve, der, stride, lens)", 0},
  {"sigToDer", -1, "c01", {"der", "lens"}, shape_sig_to_der, call_sig_to_der, 0, 0, "sigToDer(ctx, curve, r, s)", 0},
};
#define N_OPS (sizeof ops / sizeof ops[0])
static const op_desc* op_by_id(int id) {
  for (size_t i = 0; id >= 0 && i < N_OPS; i++) if (ops[i].id == id) return &ops[i];
  return NULL;
}

/* every synchronous export of the table: fetch the arguments, shape, allocate the results, call */
static napi_value op_sync(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 12; napi_value argv[12]; void* data = NULL;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, &data));
  const op_desc* d = (const op_desc*)data;
  if (argc < (size_t)d->min_argc) THROW(env, d->usage);
  op_call c; memset(&c, 0, sizeof c);
  c.ctx = get_ctx(env, argv[0]); if (!c.ctx) return NULL;
  int32_t op = -1; size_t a = 1;
  for (const char* s = d->args; *s; s++, a++) {
    const int lenient = s[1] == '?';
    if (*s >= '0' && *s <= '3') {
      if (!get_buf(env, argv[a], &c.in[*s - '0'], &c.len[*s - '0'], lenient)) return NULL;
    } else {
      int32_t v = 0; bool flag = 0;
      if ((*s == 'b' ? napi_get_value_bool(env, argv[a], &flag) : napi_get_value_int32(env, argv[a], &v)) != napi_ok && !lenient)
        THROW(env, d->badint ? d->badint : d->usage);
      switch (*s) {
        case 'c': c.curve = v; break;
        case 'h': c.hl = v; break;
        case 'm': c.mb = v; break;
        case 'b': c.i0 = flag ? 1 : 0; break;
        case 'i': case 'k': c.i0 = v; break;
        case 'j': case 'l': c.i1 = v; break;
        default: op = v; break;
      }
    }
    if (lenient) s++;
  }
  if (d->flags & F_BY_OP) {
    d = op_by_id(op);
    if (!d || !(d->flags & F_ECDH)) THROW(env, "customEcdh: bad op");
  }
  if ((d->flags & F_BASE_CURVE) && L.base_info(c.ctx, c.i0, &c.curve, NULL, NULL) != 0) return lib_error(env);
  c.d = d; c.B = L.field_bytes(c.curve); c.NB = L.order_bytes(c.curve);
  const char* bad = d->shape(&c);
  if (bad) THROW(env, bad);
  napi_value b[4] = {NULL, NULL, NULL, NULL}; void* p[4] = {NULL, NULL, NULL, NULL};
  bool own = false;              /* optional trailing (xy, inf) result Buffers supplied by the caller */
  if ((d->flags & F_OWN_OUT) && argc >= a + 2) {
    bool is0 = false, is1 = false;
    napi_is_buffer(env, argv[a], &is0); napi_is_buffer(env, argv[a + 1], &is1);
    own = is0 && is1;
  }
  if (own) {
    size_t l[2];
    for (int k = 0; k < 2; k++) { CHECK(env, napi_get_buffer_info(env, argv[a + k], &p[k], &l[k])); b[k] = argv[a + k]; }
    if (l[0] != c.ol[0] || l[1] != c.ol[1]) THROW(env, "result buffer length mismatch");
  } else {
    for (int k = 0; k < 4 && d->names[k]; k++) CHECK(env, result_buffer(env, c.ol[k], &p[k], &b[k]));
  }
  for (int k = 0; k < 4; k++) c.out[k] = (uint8_t*)p[k];
  uint8_t* wide = NULL;
  if (d->flags & F_WIDE_ENC) {
    wide = (uint8_t*)malloc(c.n * ECDH_ENC_MAX + 1);
    if (!wide) THROW(env, "customEcdh: out of memory");
    c.out[0] = wide;
  }
  int rc = d->call(&c);
  if (wide) {
    if (rc == 0) memcpy(p[0], wide, c.ol[0]);
    free(wide);
  }
  if (rc != 0) return lib_error(env);
  if (d->flags & F_BARE) return b[0];
  napi_value o; CHECK(env, napi_create_object(env, &o));
  for (int k = 0; k < 4 && d->names[k]; k++) CHECK(env, napi_set_named_property(env, o, d->names[k], b[k]));
  return o;
}

/* ---- asynchronous form: napi_async_work + Promise ----------------------------------
 * callAsync(op, ctx, curve, hashLen, msgBits, b0, b1, b2, b3[, i0, i1]) -> Promise of what the synchronous
 * form returns.  The call runs on a libuv worker thread, so the JS thread is not blocked.  One call per
 * context at a time: index.js serialises them. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref refs[5];          /* four input Buffers + the context external */
  int nrefs;
  op_call c;
  int rc;
  char err[512];
} async_job;

static void job_execute(napi_env env, void* data) {
  (void)env;
  async_job* j = (async_job*)data;
  j->rc = j->c.d->call(&j->c);
  if (j->rc != 0) {               /* last_error is thread-local: read it on this thread */
    const char* m = L.last_error();
    snprintf(j->err, sizeof j->err, "%s", m && *m ? m : "ellgpu error");
  }
}
static void free_cb(napi_env env, void* data, void* hint) { (void)env; (void)hint; free(data); }
/* every exit of a job: release its references (the context external first of all -- a leaked
 * reference keeps the external from ever being collected) and what it still owns */
static void job_free(napi_env env, async_job* j) {
  for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
  for (int k = 0; k < 4; k++) free(j->c.out[k]);
  free(j);
}
static void job_complete(napi_env env, napi_status status, void* data) {
  async_job* j = (async_job*)data;
  napi_value result = NULL;
  if (status == napi_ok && j->rc == 0) {
    const char* const* names = j->c.d->names;
    napi_create_object(env, &result);
    for (int k = 0; k < 4 && names[k]; k++) {
      napi_value b;
      napi_create_external_buffer(env, j->c.ol[k], j->c.out[k], free_cb, NULL, &b);
      j->c.out[k] = NULL;
      napi_set_named_property(env, result, names[k], b);
    }
    napi_resolve_deferred(env, j->deferred, result);
  } else {
    napi_value msg, errv;
    napi_create_string_utf8(env, j->rc ? j->err : "ellgpu: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &errv);
    napi_reject_deferred(env, j->deferred, errv);
  }
  g_jobs_in_flight--;
  napi_delete_async_work(env, j->work);
  job_free(env, j);
}
static napi_value fn_call_async(napi_env env, napi_callback_info info) {
  if (!need_lib(env)) return NULL;
  size_t argc = 11; napi_value argv[11];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 9) THROW(env, "callAsync(op, ctx, curve, hashLen, msgBits, b0, b1, b2, b3[, i0, i1])");
  async_job* j = (async_job*)calloc(1, sizeof *j);
  if (!j) THROW(env, "callAsync: out of memory");
  op_call* c = &j->c;
  int32_t op = -1, curve = 0, hl = 0, mb = 0, i0 = 0, i1 = 0;
  napi_get_value_int32(env, argv[0], &op);
  c->ctx = get_ctx(env, argv[1]);
  if (!c->ctx) { free(j); return NULL; }
  /* the worker thread uses the context after this call returns: hold its external so that it
   * cannot be collected under the job */
  napi_create_reference(env, argv[1], 1, &j->refs[j->nrefs++]);
  napi_get_value_int32(env, argv[2], &curve); napi_get_value_int32(env, argv[3], &hl); napi_get_value_int32(env, argv[4], &mb);
  if (argc > 9) napi_get_value_int32(env, argv[9], &i0);
  if (argc > 10) napi_get_value_int32(env, argv[10], &i1);
  c->d = op_by_id(op);
  c->curve = c->d && (c->d->flags & F_X25519) ? 7 : curve;
  c->hl = hl; c->mb = mb; c->i0 = i0; c->i1 = i1; c->promise = 1;
  c->B = L.field_bytes(c->curve); c->NB = L.order_bytes(c->curve);
  if (!c->d || c->B <= 0) { job_free(env, j); THROW(env, "callAsync: bad op / curve"); }
  for (int i = 0; i < 4; i++) {
    if (!get_buf(env, argv[5 + i], &c->in[i], &c->len[i], 1)) { job_free(env, j); return NULL; }
    if (c->in[i]) napi_create_reference(env, argv[5 + i], 1, &j->refs[j->nrefs++]);   /* keep alive */
  }
  if (c->d->shape(c)) { job_free(env, j); THROW(env, "callAsync: buffer length mismatch"); }
  for (int k = 0; k < 4; k++) {
    /* (F_WIDE_ENC: rows of the widest encoding, see ECDH_ENC_MAX; the Buffer handed back is ol[0] long) */
    size_t cap = k == 0 && (c->d->flags & F_WIDE_ENC) ? c->n * ECDH_ENC_MAX + 1 : c->ol[k];
    c->out[k] = (uint8_t*)malloc(cap ? cap : 1);
    if (!c->out[k]) { job_free(env, j); THROW(env, "callAsync: out of memory"); }
  }
  napi_value promise, name;
  CHECK(env, napi_create_promise(env, &j->deferred, &promise));
  CHECK(env, napi_create_string_utf8(env, "ellgpu", NAPI_AUTO_LENGTH, &name));
  CHECK(env, napi_create_async_work(env, NULL, name, job_execute, job_complete, j, &j->work));
  CHECK(env, napi_queue_async_work(env, j->work));
  g_jobs_in_flight++;
  return promise;
}

static napi_value init(napi_env env, napi_value exports) {
  struct { const char* name; napi_callback fn; } fns[] = {
    {"open", fn_open}, {"createContext", fn_create}, {"destroyContext", fn_destroy},
    {"defer", fn_defer}, {"collect", fn_collect}, {"combBits", fn_comb_bits},
    {"curveId", fn_curve_id}, {"fieldBytes", fn_field_bytes}, {"orderBytes", fn_order_bytes},
    {"deviceCount", fn_device_count}, {"groupSize", fn_group_size}, {"defineShort", fn_define_short},
    {"defineEdwards", fn_define_edwards}, {"defineMont", fn_define_mont}, {"defineShortDomain", fn_define_short_domain},
    {"defineEdwardsDomain", fn_define_edwards_domain}, {"defineBase", fn_define_base}, {"defineEdBase", fn_define_ed_base},
    {"releaseBase", fn_release_base}, {"baseInfo", fn_base_info}, {"callAsync", fn_call_async},
  };
  napi_add_env_cleanup_hook(env, on_env_cleanup, NULL);
  for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
    if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
  }
  /* the batch operations: their synchronous exports, and ops = {name: callAsync's id} */
  napi_value ids;
  if (napi_create_object(env, &ids) != napi_ok) return NULL;
  for (size_t i = 0; i < N_OPS; i++) {
    napi_value f, id;
    if (ops[i].args && (napi_create_function(env, ops[i].name, NAPI_AUTO_LENGTH, op_sync, (void*)&ops[i], &f) != napi_ok ||
                        napi_set_named_property(env, exports, ops[i].name, f) != napi_ok)) return NULL;
    if (ops[i].id >= 0 && (napi_create_int32(env, ops[i].id, &id) != napi_ok ||
                           napi_set_named_property(env, ids, ops[i].name, id) != napi_ok)) return NULL;
  }
  if (napi_set_named_property(env, exports, "ops", ids) != napi_ok) return NULL;
  return exports;
}
NAPI_MODULE(NODE_GYP_MODULE_NAME, init)

// extern "C" surface of libapk (include/apk.h): argument checking, curve dispatch, and the host-only wire
// formats that replace /root/reference/helper.go (MarshalProof :13-24, marshalPlonkBls12381Proof :27-88,
// MarshalPublicInputs :91-110).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <string>
#include <type_traits>

#include <hip/hip_runtime_api.h>

#include "backend.h"
#include "device_sched.h"
#include "ec.h"
#include "kernels_kzg.h"
#include "kernels_kzg_lagrange.h"
#include "kzg_recover_plan.h"   // recover_check_call
#include "plonk_protocol.h"
#include "poly_run.h"   // poly_op_check
#include "proof_codec.h"
#include "runtime_env.h"
#include "selftest_ops.h"

namespace apk {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

// One hardware queue per concurrently proving HIP stream: ROCm's default of 4 serialises a context's 16 proving streams onto
// 4 queues.  The ROCm runtime reads GPU_MAX_HW_QUEUES once, when it initialises (the process's first HIP call), so the library
// claims its queues when it is LOADED - before any HIP call made through it, and ahead of every other constructor of the
// library (priority 101: the code-object registration of the .hip files comes after).  The claim only ever raises the variable
// (runtime_env.h has the rule and APK_HW_QUEUES); this constructor is the ONLY place that writes it.  apk_runtime_read reports
// what was found and what was left; include/apk.h documents the contract for hosts that initialise HIP earlier.
// g_runtime MUST stay constant-initialised (plain ints, std::atomic<int> with constant initialisers): the constructor below runs
// before this file's dynamic initialisers, and a member initialised dynamically would be reset AFTER it and wipe the record
// (the attribute makes the compiler refuse that).
struct RuntimeRecord {
    int found, left, need, written;
    std::atomic<int> first_hip;        // -1: no HIP call through the library yet; 1 / 0: the variable still held `left` then / did not
    std::atomic<int> at_first_hip;
};
[[clang::require_constant_initialization]] static RuntimeRecord g_runtime = {HWQ_UNSET, HWQ_UNSET, HWQ_NEED, 0, {-1}, {HWQ_UNSET}};

__attribute__((constructor(101))) static void apk_claim_hw_queues() {
    const int found = hwq_parse(getenv("GPU_MAX_HW_QUEUES"));
    const HwqPlan plan = hwq_plan(found, hwq_parse(getenv("APK_HW_QUEUES")));
    g_runtime.found = found;
    g_runtime.need = plan.need;
    g_runtime.left = found;
    if (plan.write) {
        char buf[16];
        snprintf(buf, sizeof buf, "%d", plan.write);
        if (setenv("GPU_MAX_HW_QUEUES", buf, /*overwrite=*/1) == 0) { g_runtime.left = plan.write; g_runtime.written = 1; }
    }
}

void runtime_checkpoint() {
    static std::once_flag once;
    std::call_once(once, [] {
        const int now = hwq_parse(getenv("GPU_MAX_HW_QUEUES"));
        g_runtime.at_first_hip.store(now);
        g_runtime.first_hip.store(now == g_runtime.left ? 1 : 0);
    });
}

int env_int(const char* name, int dflt, int lo, int hi) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    char* end = nullptr;
    long x = strtol(v, &end, 10);
    if (end == v) return dflt;
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return (int)x;
}

template <class P>
static void mont_to_be(const void* in, uint8_t* be) {
    Fe<P> m;
    memcpy(&m, in, sizeof m);
    fe_to_be<P>(m, be);
}

template <class P>
static int be_to_mont(const uint8_t* be, void* out) {
    Fe<P> a;
    // reject non-canonical input (>= modulus)
    if (!fe_load_be<P>(be, a)) { set_error("field element is not canonical (>= modulus)"); return APK_ERR_ARG; }
    Fe<P> m = Fe<P>::to_mont(a);
    memcpy(out, &m, sizeof m);
    return APK_OK;
}

int host_fe_to_be(int curve, int field, const void* in, uint8_t* be) {
    if (curve == APK_BN254) { field ? mont_to_be<FpBN254>(in, be) : mont_to_be<FrBN254>(in, be); return APK_OK; }
    if (curve == APK_BLS12_381) { field ? mont_to_be<FpBLS12381>(in, be) : mont_to_be<FrBLS12381>(in, be); return APK_OK; }
    set_error("unsupported curve id %d", curve);
    return APK_ERR_ARG;
}

int host_fe_from_be(int curve, int field, const uint8_t* be, void* out) {
    if (curve == APK_BN254) return field ? be_to_mont<FpBN254>(be, out) : be_to_mont<FrBN254>(be, out);
    if (curve == APK_BLS12_381) return field ? be_to_mont<FpBLS12381>(be, out) : be_to_mont<FrBLS12381>(be, out);
    set_error("unsupported curve id %d", curve);
    return APK_ERR_ARG;
}

// ---- host-side execution of the SAME arithmetic templates the kernels use (selftest_ops.h; ff.h / ec.h are host+device):
// lets the CPU-only test tier check the field and curve formulas against the oracle without a GPU.
static int selftest_status(int st, const char* what, int op) {
    if (st == SELFTEST_OK) return APK_OK;
    if (st == SELFTEST_NO_UNSAT) set_error("field has no unsaturated-limb form");
    else set_error("unknown %s op %d", what, op);
    return APK_ERR_ARG;
}

template <class P>
static void feu_shape_t(int* ul, int* ub, uint32_t* headroom) {
    *ul = FeU<P>::L;
    *ub = FeU<P>::B;
    *headroom = FeU<P>::HEADROOM;
}

template <class P>
static int host_feu_batch(int op, uint64_t count, const uint32_t* in, uint32_t* out) {
    constexpr int L = FeU<P>::L;
    for (uint64_t i = 0; i < count; i++) {
        const int st = feu_op_t<P>(op, in + i * 4 * L, out + i * L);
        if (st != SELFTEST_OK) return selftest_status(st, "unsaturated", op);
    }
    return APK_OK;
}

// the device seams: the op code is checked here, before anything is launched
static bool seam_args(int curve, uint64_t count, bool ok_op, int op, const char* what) {
    if (curve != APK_BN254 && curve != APK_BLS12_381) { set_error("unsupported curve: %d", curve); return false; }
    if (!ok_op) { set_error("unknown %s op %d", what, op); return false; }
    if (count >= (1ull << 26)) { set_error("count too large"); return false; }
    return true;
}

template <class FPP>
static int g1_sum_t(const void* points, uint64_t count, void* out) {
    using A = Affine<FPP>;
    using X = XYZZ<FPP>;
    X acc = X::inf();
    for (uint64_t i = 0; i < count; i++) {
        A p;
        memcpy(&p, reinterpret_cast<const uint8_t*>(points) + i * sizeof(A), sizeof p);
        acc.madd(p);
    }
    const A r = acc.to_affine();
    memcpy(out, &r, sizeof r);
    return APK_OK;
}

}  // namespace apk

using namespace apk;

struct apk_ctx {
    Backend* be;
    int curve;
};

// Live contexts: a communicator keeps a pointer to the context it was bound to, and host languages with finalizers (the Python
// mirror; a Go host with runtime.SetFinalizer) may destroy the context FIRST.  apk_comm_destroy / apk_comm_bind ask here before they
// take their hooks off a context (comm.cpp clear_ctx_hooks): a destroyed one is simply forgotten.
#include <set>
namespace apk {
static std::mutex g_live_mu;
static std::set<const void*>& live_set() { static std::set<const void*> s; return s; }
static void ctx_register(const void* c) { std::lock_guard<std::mutex> g(g_live_mu); live_set().insert(c); }
static void ctx_forget(const void* c) { std::lock_guard<std::mutex> g(g_live_mu); live_set().erase(c); }
bool ctx_alive(const void* c) { std::lock_guard<std::mutex> g(g_live_mu); return live_set().count(c) != 0; }

// ---- the device-wide schedulers (device_sched.h): one per device ordinal, created on first use and never destroyed (contexts of
// any thread may hold a pointer until the process ends; the streams go with the runtime).  APK_MAX_SLOTS is the DEVICE's stream
// budget; APK_DEVICE_SCHED=0 turns the scheduler off - every context then has a pool and a budget of its own, as before it
// existed (for A/B runs, and as an escape hatch).  Both are read once per process.
static int sched_max_streams() { static const int v = env_int("APK_MAX_SLOTS", 16, 1, 64); return v; }
static bool sched_device_wide() { static const int v = env_int("APK_DEVICE_SCHED", 1, 0, 1); return v != 0; }
struct DeviceEntry {
    DeviceSched sched{(size_t)sched_max_streams(), /*fifo=*/true};
    std::mutex stream_mu;
    std::vector<hipStream_t> streams;     // created by the first context on the device
};
static DeviceEntry* device_entry(int device) {
    static std::mutex mu;
    static std::vector<DeviceEntry*>* entries = new std::vector<DeviceEntry*>();     // (never destroyed: see above)
    if (device < 0 || device >= 4096) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    if (entries->size() <= (size_t)device) entries->resize((size_t)device + 1, nullptr);
    if (!(*entries)[(size_t)device]) (*entries)[(size_t)device] = new DeviceEntry();
    return (*entries)[(size_t)device];
}
DeviceSched* device_sched_for(int device) {
    if (!sched_device_wide()) return nullptr;
    DeviceEntry* e = device_entry(device);
    return e ? &e->sched : nullptr;
}
int device_stream_pool(int device, void** streams, int cap, int* count) {
    DeviceEntry* e = device_entry(device);
    if (!e || !streams || !count) { set_error("device %d: no scheduler", device); return APK_ERR_ARG; }
    std::lock_guard<std::mutex> g(e->stream_mu);
    const int want = sched_max_streams();
    if (cap < want) { set_error("stream pool of %d does not fit %d", want, cap); return APK_ERR_ARG; }
    if (e->streams.empty()) {
        runtime_checkpoint();
        hipError_t he = hipSetDevice(device);
        std::vector<hipStream_t> made;
        for (int i = 0; i < want && he == hipSuccess; i++) {
            hipStream_t ps = nullptr;
            he = hipStreamCreateWithFlags(&ps, hipStreamNonBlocking);
            if (he == hipSuccess) made.push_back(ps);
        }
        if (he != hipSuccess) {
            for (hipStream_t ps : made) (void)hipStreamDestroy(ps);
            (void)hipGetLastError();
            set_error("device %d: proving streams: %s", device, hipGetErrorString(he));
            return APK_ERR_HIP;
        }
        e->streams = made;
    }
    for (int i = 0; i < want; i++) streams[i] = e->streams[(size_t)i];
    *count = want;
    return APK_OK;
}
}

extern "C" {

const char* apk_last_error(void) { return g_err.c_str(); }
int apk_abi_version(void) { return APK_ABI_VERSION; }

int apk_device_count(int* count) {
    if (!count) { set_error("null count"); return APK_ERR_ARG; }
    int n = 0;
    runtime_checkpoint();
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return APK_OK; }  // runtime present, no usable GPU
    *count = n;
    return APK_OK;
}

size_t apk_fp_bytes(int curve) { return curve == APK_BN254 ? 32 : curve == APK_BLS12_381 ? 48 : 0; }
size_t apk_g1_bytes(int curve) { return 2 * apk_fp_bytes(curve); }

int apk_ctx_create(const apk_circuit_desc* d, apk_ctx** out) {
    if (!d || !out) { set_error("null argument"); return APK_ERR_ARG; }
    *out = nullptr;
    runtime_checkpoint();
    Backend* be = nullptr;
    if (d->curve == APK_BN254) be = make_backend_bn254();
    else if (d->curve == APK_BLS12_381) be = make_backend_bls12381();
    else { set_error("unsupported curve: %d", d->curve); return APK_ERR_ARG; }  // algoplonk.go:39-41
    int r = be->init(d);
    if (r != APK_OK) { delete be; return r; }
    *out = new apk_ctx{be, d->curve};
    ctx_register(*out);
    return APK_OK;
}

int apk_msm_ctx_create(int curve, int device, const void* bases, uint64_t count, int msm_window, apk_ctx** out) {
    if (!bases || !out) { set_error("null argument"); return APK_ERR_ARG; }
    *out = nullptr;
    runtime_checkpoint();
    Backend* be = nullptr;
    if (curve == APK_BN254) be = make_backend_bn254();
    else if (curve == APK_BLS12_381) be = make_backend_bls12381();
    else { set_error("unsupported curve: %d", curve); return APK_ERR_ARG; }
    int r = be->init_msm_only(device, bases, count, msm_window);
    if (r != APK_OK) { delete be; return r; }
    *out = new apk_ctx{be, curve};
    ctx_register(*out);
    return APK_OK;
}

void apk_ctx_destroy(apk_ctx* ctx) {
    if (!ctx) return;
    ctx_forget(ctx);
    delete ctx->be;
    delete ctx;
}

#define NEED_CTX()                                          \
    if (!ctx) { set_error("null context"); return APK_ERR_ARG; }

int apk_ctx_get_vk(apk_ctx* ctx, apk_vk* out) { NEED_CTX(); if (!out) { set_error("null out"); return APK_ERR_ARG; } return ctx->be->get_vk(out); }
int apk_msm_g1(apk_ctx* ctx, int basis, const void* sc, uint64_t len, void* out) {
    NEED_CTX(); if (!sc || !out) { set_error("null argument"); return APK_ERR_ARG; }
    return ctx->be->msm(basis, sc, len, false, out);
}
int apk_msm_g1_device(apk_ctx* ctx, int basis, const void* sc, uint64_t len, void* out) {
    NEED_CTX(); if (!sc || !out) { set_error("null argument"); return APK_ERR_ARG; }
    return ctx->be->msm(basis, sc, len, true, out);
}
int apk_msm_g1_batch_device(apk_ctx* ctx, int basis, uint32_t count, const void* const* d_scalars, const uint64_t* offsets,
                            const uint64_t* lens, void* out) {
    NEED_CTX();
    if (!d_scalars || !offsets || !lens || !out) { set_error("null argument"); return APK_ERR_ARG; }
    return ctx->be->msm_batch(basis, count, d_scalars, offsets, lens, out);
}
// ---- KZG openings: arguments other than the context first, then a usable device (there is no CPU fallback), then the context
static int kzg_need_device() {
    int ndev = 0;
    runtime_checkpoint();
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e == hipSuccess && ndev > 0) return APK_OK;
    (void)hipGetLastError();
    set_error("no HIP device available (%s); libapk has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    return APK_ERR_HIP;
}
static int kzg_open_any(apk_ctx* ctx, const void* poly, uint64_t len, bool on_device, const void* point, void* out_h, void* out_value) {
    if (!poly || !point || !out_h || !out_value) { set_error("null argument"); return APK_ERR_ARG; }
    if (len == 0 || len >= (1ull << 31)) { set_error("kzg: %llu coefficients", (unsigned long long)len); return APK_ERR_ARG; }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_open(poly, len, on_device, point, out_h, out_value);
}
static int kzg_batch_open_any(apk_ctx* ctx, uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, const void* digests,
                              const void* point, const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) {
    if (!polys || !lens || !point || !out_h || !out_values || (extra_len && !extra)) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0 || count > APK_KZG_MAX_POLYS) { set_error("kzg: %u polynomials (1..%d)", count, APK_KZG_MAX_POLYS); return APK_ERR_ARG; }
    for (uint32_t i = 0; i < count; i++) {
        if (!polys[i]) { set_error("kzg: polynomial %u is null", i); return APK_ERR_ARG; }
        if (lens[i] == 0 || lens[i] >= (1ull << 31)) { set_error("kzg: polynomial %u has %llu coefficients", i, (unsigned long long)lens[i]); return APK_ERR_ARG; }
    }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_batch_open(count, polys, lens, on_device, digests, point, extra, extra_len, out_h, out_values, out_gamma);
}
int apk_kzg_open(apk_ctx* ctx, const void* poly, uint64_t len, const void* point_fr, void* out_h, void* out_value) {
    return kzg_open_any(ctx, poly, len, false, point_fr, out_h, out_value);
}
int apk_kzg_open_device(apk_ctx* ctx, const void* d_poly, uint64_t len, const void* point_fr, void* out_h, void* out_value) {
    return kzg_open_any(ctx, d_poly, len, true, point_fr, out_h, out_value);
}
int apk_kzg_batch_open(apk_ctx* ctx, uint32_t count, const void* const* polys, const uint64_t* lens, const void* digests, const void* point_fr,
                       const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) {
    return kzg_batch_open_any(ctx, count, polys, lens, false, digests, point_fr, extra, extra_len, out_h, out_values, out_gamma);
}
int apk_kzg_batch_open_device(apk_ctx* ctx, uint32_t count, const void* const* d_polys, const uint64_t* lens, const void* digests,
                              const void* point_fr, const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) {
    return kzg_batch_open_any(ctx, count, d_polys, lens, true, digests, point_fr, extra, extra_len, out_h, out_values, out_gamma);
}
static int kzg_open_multi_any(apk_ctx* ctx, uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, const void* points,
                              void* out_h, void* out_values) {
    if (!polys || !lens || !points || !out_h || !out_values) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0 || count > APK_KZG_MAX_POLYS) { set_error("kzg: %u openings (1..%d)", count, APK_KZG_MAX_POLYS); return APK_ERR_ARG; }
    for (uint32_t i = 0; i < count; i++) {
        if (!polys[i]) { set_error("kzg: polynomial %u is null", i); return APK_ERR_ARG; }
        if (lens[i] == 0 || lens[i] >= (1ull << 31)) { set_error("kzg: polynomial %u has %llu coefficients", i, (unsigned long long)lens[i]); return APK_ERR_ARG; }
    }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_open_multi(count, polys, lens, on_device, points, out_h, out_values);
}
int apk_kzg_open_multi(apk_ctx* ctx, uint32_t count, const void* const* polys, const uint64_t* lens, const void* points, void* out_h,
                       void* out_values) {
    return kzg_open_multi_any(ctx, count, polys, lens, false, points, out_h, out_values);
}
int apk_kzg_open_multi_device(apk_ctx* ctx, uint32_t count, const void* const* d_polys, const uint64_t* lens, const void* points, void* out_h,
                              void* out_values) {
    return kzg_open_multi_any(ctx, count, d_polys, lens, true, points, out_h, out_values);
}
// ---- the openings of one polynomial at every point of its domain (kzg_all_run.h): the checks in the same order
int apk_kzg_all_prepare(apk_ctx* ctx, const void* srs_g1, uint64_t count) {
    if (!srs_g1) { set_error("null argument"); return APK_ERR_ARG; }
    const uint64_t n = ctx && ctx_alive(ctx) ? ctx->be->domain_size() : 0;
    if (count == 0 || (n && count < n - 1)) { set_error("kzg: %llu SRS points for a domain of %llu", (unsigned long long)count, (unsigned long long)n); return APK_ERR_ARG; }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_all_prepare(srs_g1, count);
}
static int kzg_open_all_any(apk_ctx* ctx, const void* poly, uint64_t len, bool on_device, void* out_h, void* out_values) {
    if (!poly || !out_h) { set_error("null argument"); return APK_ERR_ARG; }
    if (len == 0 || len >= (1ull << 31)) { set_error("kzg: %llu coefficients", (unsigned long long)len); return APK_ERR_ARG; }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_open_all(poly, len, on_device, out_h, out_values);
}
int apk_kzg_open_all(apk_ctx* ctx, const void* poly, uint64_t len, void* out_h, void* out_values) {
    return kzg_open_all_any(ctx, poly, len, false, out_h, out_values);
}
int apk_kzg_open_all_device(apk_ctx* ctx, const void* d_poly, uint64_t len, void* out_h, void* out_values) {
    return kzg_open_all_any(ctx, d_poly, len, true, out_h, out_values);
}
// ---- the openings of one polynomial on every coset of its domain (kzg_cosets_run.h): the checks in the same order
int apk_kzg_cosets_prepare(apk_ctx* ctx, const void* srs_g1, uint64_t count, uint32_t coset_size) {
    if (!srs_g1) { set_error("null argument"); return APK_ERR_ARG; }
    if (coset_size < 2 || (coset_size & (coset_size - 1))) { set_error("kzg: cosets of %u points (a power of two, at least 2)", coset_size); return APK_ERR_ARG; }
    const uint64_t n = ctx && ctx_alive(ctx) ? ctx->be->domain_size() : 0;
    if (count == 0 || (n && (coset_size > n / 2 || count < n - coset_size))) {
        set_error("kzg: %llu SRS points and cosets of %u points for a domain of %llu", (unsigned long long)count, coset_size, (unsigned long long)n);
        return APK_ERR_ARG;
    }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_cosets_prepare(srs_g1, count, coset_size);
}
static int kzg_open_cosets_any(apk_ctx* ctx, const void* poly, uint64_t len, bool on_device, void* out_h, void* out_values) {
    if (!poly || !out_h) { set_error("null argument"); return APK_ERR_ARG; }
    if (len == 0 || len >= (1ull << 31)) { set_error("kzg: %llu coefficients", (unsigned long long)len); return APK_ERR_ARG; }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_open_cosets(poly, len, on_device, out_h, out_values);
}
int apk_kzg_open_cosets(apk_ctx* ctx, const void* poly, uint64_t len, void* out_h, void* out_values) {
    return kzg_open_cosets_any(ctx, poly, len, false, out_h, out_values);
}
int apk_kzg_open_cosets_device(apk_ctx* ctx, const void* d_poly, uint64_t len, void* out_h, void* out_values) {
    return kzg_open_cosets_any(ctx, d_poly, len, true, out_h, out_values);
}
// ---- many polynomials on every coset in one call (kzg_cosets_multi_run.h): a usable device and a live context, then EVERY rule in the
// order of include/apk.h - the state of the context first - which the planner states (kzg_fk20_plan.h fk20_multi_check)
static int kzg_open_cosets_multi_any(apk_ctx* ctx, uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, void* out_h,
                                     void* out_values) {
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_open_cosets_multi(count, polys, lens, on_device, out_h, out_values);
}
int apk_kzg_open_cosets_multi(apk_ctx* ctx, uint32_t count, const void* const* polys, const uint64_t* lens, void* out_h, void* out_values) {
    return kzg_open_cosets_multi_any(ctx, count, polys, lens, false, out_h, out_values);
}
int apk_kzg_open_cosets_multi_device(apk_ctx* ctx, uint32_t count, const void* const* d_polys, const uint64_t* lens, void* out_h, void* out_values) {
    return kzg_open_cosets_multi_any(ctx, count, d_polys, lens, true, out_h, out_values);
}
// ---- the polynomial back from a sufficient set of its cells (kzg_recover_run.h): the checks in the same order; the context-free
// rules are the planner's (kzg_recover_plan.h), which apk_kzg_recover_cosets_host (verify_api.cpp) states the same way
static int kzg_recover_cosets_any(apk_ctx* ctx, uint32_t coset_size, uint32_t count, const uint64_t* indices, const void* values, uint64_t len,
                                  bool on_device, void* out_poly) {
    if (!indices || !values || !out_poly) { set_error("null argument"); return APK_ERR_ARG; }
    const RecoverVerdict v = recover_check_call(coset_size, count, len);
    if (v.rc != APK_OK) { set_error("%s", v.message); return v.rc; }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_recover_cosets(coset_size, count, indices, values, len, on_device, out_poly);
}
int apk_kzg_recover_cosets(apk_ctx* ctx, uint32_t coset_size, uint32_t count, const uint64_t* indices, const void* values, uint64_t len,
                           void* out_poly) {
    return kzg_recover_cosets_any(ctx, coset_size, count, indices, values, len, false, out_poly);
}
int apk_kzg_recover_cosets_device(apk_ctx* ctx, uint32_t coset_size, uint32_t count, const uint64_t* indices, const void* d_values, uint64_t len,
                                  void* d_out_poly) {
    return kzg_recover_cosets_any(ctx, coset_size, count, indices, d_values, len, true, d_out_poly);
}
int apk_kzg_shape(int* lane_chunk, int* block_span) {
    if (!lane_chunk || !block_span) { set_error("null argument"); return APK_ERR_ARG; }
    static_assert(KZG_MAX_POLYS == APK_KZG_MAX_POLYS, "kernels_kzg.h and include/apk.h agree on the batch size");
    *lane_chunk = KZG_LANE_CHUNK;
    *block_span = KZG_BLOCK_SPAN;
    return APK_OK;
}
// ---- the same in evaluation form (kernels_kzg_lagrange.h): the checks in the same order
static int kzg_open_lagrange_any(apk_ctx* ctx, const void* evals, uint64_t len, bool on_device, const void* point, void* out_h, void* out_value) {
    if (!evals || !point || !out_h || !out_value) { set_error("null argument"); return APK_ERR_ARG; }
    if (len == 0 || len >= (1ull << 31)) { set_error("kzg: %llu values", (unsigned long long)len); return APK_ERR_ARG; }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_open_lagrange(evals, len, on_device, point, out_h, out_value);
}
static int kzg_batch_open_lagrange_any(apk_ctx* ctx, uint32_t count, const void* const* evals, bool on_device, const void* digests,
                                       const void* point, const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) {
    if (!evals || !point || !out_h || !out_values || (extra_len && !extra)) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0 || count > APK_KZG_MAX_POLYS) { set_error("kzg: %u vectors (1..%d)", count, APK_KZG_MAX_POLYS); return APK_ERR_ARG; }
    for (uint32_t i = 0; i < count; i++)
        if (!evals[i]) { set_error("kzg: vector %u is null", i); return APK_ERR_ARG; }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_batch_open_lagrange(count, evals, on_device, digests, point, extra, extra_len, out_h, out_values, out_gamma);
}
int apk_kzg_open_lagrange(apk_ctx* ctx, const void* evals, uint64_t len, const void* point_fr, void* out_h, void* out_value) {
    return kzg_open_lagrange_any(ctx, evals, len, false, point_fr, out_h, out_value);
}
int apk_kzg_open_lagrange_device(apk_ctx* ctx, const void* d_evals, uint64_t len, const void* point_fr, void* out_h, void* out_value) {
    return kzg_open_lagrange_any(ctx, d_evals, len, true, point_fr, out_h, out_value);
}
int apk_kzg_batch_open_lagrange(apk_ctx* ctx, uint32_t count, const void* const* evals, const void* digests, const void* point_fr,
                                const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) {
    return kzg_batch_open_lagrange_any(ctx, count, evals, false, digests, point_fr, extra, extra_len, out_h, out_values, out_gamma);
}
int apk_kzg_batch_open_lagrange_device(apk_ctx* ctx, uint32_t count, const void* const* d_evals, const void* digests, const void* point_fr,
                                       const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) {
    return kzg_batch_open_lagrange_any(ctx, count, d_evals, true, digests, point_fr, extra, extra_len, out_h, out_values, out_gamma);
}
static int kzg_open_multi_lagrange_any(apk_ctx* ctx, uint32_t count, const void* const* evals, bool on_device, const void* points, void* out_h,
                                       void* out_values) {
    if (!evals || !points || !out_h || !out_values) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0 || count > APK_KZG_MAX_POLYS) { set_error("kzg: %u openings (1..%d)", count, APK_KZG_MAX_POLYS); return APK_ERR_ARG; }
    const int rc = kzg_need_device();
    if (rc != APK_OK) return rc;
    NEED_CTX();
    return ctx->be->kzg_open_multi_lagrange(count, evals, on_device, points, out_h, out_values);      // (a null vector: the context's answer)
}
int apk_kzg_open_multi_lagrange(apk_ctx* ctx, uint32_t count, const void* const* evals, const void* points, void* out_h, void* out_values) {
    return kzg_open_multi_lagrange_any(ctx, count, evals, false, points, out_h, out_values);
}
int apk_kzg_open_multi_lagrange_device(apk_ctx* ctx, uint32_t count, const void* const* d_evals, const void* points, void* out_h,
                                       void* out_values) {
    return kzg_open_multi_lagrange_any(ctx, count, d_evals, true, points, out_h, out_values);
}
int apk_kzg_lagrange_shape(int* lane_chunk, int* block_span) {
    if (!lane_chunk || !block_span) { set_error("null argument"); return APK_ERR_ARG; }
    *lane_chunk = KZG_LAG_LANE_CHUNK;
    *block_span = KZG_LAG_BLOCK_SPAN;
    return APK_OK;
}
int apk_ctx_set_commit_hook(apk_ctx* ctx, apk_commit_hook hook, void* user) { NEED_CTX(); return ctx->be->set_commit_hook(hook, user); }
int apk_device_copy(apk_ctx* ctx, void* d, const void* s, size_t b) { NEED_CTX(); return ctx->be->dev_copy(d, s, b); }
int apk_ctx_set_wire_hook(apk_ctx* ctx, apk_wire_hook hook, void* user) { NEED_CTX(); return ctx->be->set_wire_hook(hook, user); }
int apk_ctx_set_subcoset(apk_ctx* ctx, int k, int world, apk_gather_hook hook, void* user) { NEED_CTX(); return ctx->be->set_subcoset(k, world, hook, user); }
int apk_coset_ntt_device(apk_ctx* ctx, const void* d_in, uint64_t len, void* d_out) { NEED_CTX(); return ctx->be->coset_ntt_dev(d_in, len, d_out); }
int apk_ntt(apk_ctx* ctx, int which, int inverse, int coset, void* data) {
    NEED_CTX(); if (!data) { set_error("null data"); return APK_ERR_ARG; }
    return ctx->be->ntt(which, inverse, coset, data);
}
int apk_prove(apk_ctx* ctx, const void* L, const void* R, const void* O, const void* pub, const void* bl,
              const void* const* pi2, apk_proof* out) {
    NEED_CTX();
    return ctx->be->prove(L, R, O, false, pub, bl, pi2, out);
}
int apk_prove_device(apk_ctx* ctx, const void* L, const void* R, const void* O, const void* pub, const void* bl,
                     const void* const* pi2, apk_proof* out) {
    NEED_CTX();
    return ctx->be->prove(L, R, O, true, pub, bl, pi2, out);
}
// page-locked host memory for apk_prove's inputs (include/apk.h)
static int host_mem_device(int device) {
    int ndev = 0;
    runtime_checkpoint();
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) { (void)hipGetLastError(); set_error("no HIP device available (%s); libapk has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e)); return APK_ERR_HIP; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (%d devices)", device, ndev); return APK_ERR_ARG; }
    e = hipSetDevice(device);
    if (e != hipSuccess) { set_error("hipSetDevice: %s", hipGetErrorString(e)); return APK_ERR_HIP; }
    return APK_OK;
}
int apk_host_alloc(int device, size_t bytes, void** p) {
    if (!p || bytes == 0) { set_error("null argument"); return APK_ERR_ARG; }
    *p = nullptr;
    int rc = host_mem_device(device);
    if (rc != APK_OK) return rc;
    hipError_t e = hipHostMalloc(p, bytes, hipHostMallocPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; set_error("hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); return APK_ERR_HIP; }
    return APK_OK;
}
int apk_host_free(void* p) {
    if (!p) return APK_OK;
    hipError_t e = hipHostFree(p);
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipHostFree: %s", hipGetErrorString(e)); return APK_ERR_HIP; }
    return APK_OK;
}
int apk_host_register(void* p, size_t bytes) {
    if (!p || bytes == 0) { set_error("null argument"); return APK_ERR_ARG; }
    int rc = host_mem_device(0);
    if (rc != APK_OK) return rc;
    hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipHostRegister(%zu): %s", bytes, hipGetErrorString(e)); return APK_ERR_HIP; }
    return APK_OK;
}
int apk_host_unregister(void* p) {
    if (!p) return APK_OK;
    hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("hipHostUnregister: %s", hipGetErrorString(e)); return APK_ERR_HIP; }
    return APK_OK;
}

int apk_device_alloc(apk_ctx* ctx, size_t bytes, void** p) { NEED_CTX(); return ctx->be->dev_alloc(bytes, p); }
int apk_device_free(apk_ctx* ctx, void* p) { NEED_CTX(); return ctx->be->dev_free(p); }
int apk_device_upload(apk_ctx* ctx, void* d, const void* s, size_t b) { NEED_CTX(); return ctx->be->dev_upload(d, s, b); }
int apk_device_download(apk_ctx* ctx, void* d, const void* s, size_t b) { NEED_CTX(); return ctx->be->dev_download(d, s, b); }
int apk_stats_enable(apk_ctx* ctx, int en) { NEED_CTX(); return ctx->be->stats_enable(en); }
int apk_stats_read(apk_ctx* ctx, apk_stats* out, int reset) { NEED_CTX(); if (!out) { set_error("null out"); return APK_ERR_ARG; } return ctx->be->stats_read(out, reset); }
int apk_ctx_msm_window(apk_ctx* ctx) { if (!ctx || !ctx->be) return 0; return ctx->be->msm_window(); }
int apk_device_sched_read(int device, apk_device_sched* out, int reset) {
    if (!out) { set_error("null out"); return APK_ERR_ARG; }
    if (device < 0 || device >= 4096) { set_error("device %d out of range", device); return APK_ERR_ARG; }
    memset(out, 0, sizeof *out);
    out->max_streams = (uint32_t)sched_max_streams();
    out->device_wide = sched_device_wide() ? 1u : 0u;
    DeviceSched* sc = device_sched_for(device);
    if (!sc) return APK_OK;      // APK_DEVICE_SCHED=0: nothing is counted per device
    const DeviceSched::Counts c = sc->read(reset != 0);
    out->contexts = c.contexts; out->max_streams = c.max_streams;
    out->streams_in_use = c.streams_in_use; out->streams_peak = c.streams_peak;
    out->proofs_in_flight = c.proofs_in_flight; out->proofs_peak = c.proofs_peak;
    out->waiting = c.waiting;
    return APK_OK;
}
int apk_paths_read(apk_ctx* ctx, apk_path_counts* out, int reset) { NEED_CTX(); if (!out) { set_error("null out"); return APK_ERR_ARG; } return ctx->be->paths_read(out, reset); }
int apk_runtime_read(apk_runtime* out) {
    if (!out) { set_error("null out"); return APK_ERR_ARG; }
    memset(out, 0, sizeof *out);
    out->hw_queues_found = g_runtime.found; out->hw_queues_left = g_runtime.left;
    out->hw_queues_need = g_runtime.need; out->hw_queues_written = g_runtime.written;
    out->hw_queues_now = hwq_parse(getenv("GPU_MAX_HW_QUEUES"));
    out->first_hip_call = g_runtime.first_hip.load();
    out->hw_queues_at_first_hip = g_runtime.at_first_hip.load();
    return APK_OK;
}

int apk_g1_mul_batch(int curve, int device, const void* base, const void* scalars, uint64_t count, void* out) {
    if (!base || !scalars || !out) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0) return APK_OK;
    if (count >= (1ull << 31)) { set_error("count too large"); return APK_ERR_ARG; }
    runtime_checkpoint();
    if (curve == APK_BN254) return g1_mul_batch_bn254(device, base, scalars, count, out);
    if (curve == APK_BLS12_381) return g1_mul_batch_bls12381(device, base, scalars, count, out);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_g1_decompress(int curve, int device, const uint8_t* compressed, uint64_t count, void* out) {
    if (!compressed || !out) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0) return APK_OK;
    if (count >= (1ull << 31)) { set_error("count too large"); return APK_ERR_ARG; }
    runtime_checkpoint();
    if (curve == APK_BN254) return g1_decompress_bn254(device, compressed, count, out);
    if (curve == APK_BLS12_381) return g1_decompress_bls12381(device, compressed, count, out);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_g1_to_lagrange(int curve, int device, const void* points, uint64_t n, void* out) {
    if (!points || !out) { set_error("null argument"); return APK_ERR_ARG; }
    runtime_checkpoint();
    if (curve == APK_BN254) return g1_to_lagrange_bn254(device, points, n, out);
    if (curve == APK_BLS12_381) return g1_to_lagrange_bls12381(device, points, n, out);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_host_fe_op(int curve, int field, int op, const void* a, const void* b, void* out) {
    if (!a || !out) { set_error("null argument"); return APK_ERR_ARG; }
    if (curve == APK_BN254) return selftest_status(field ? fe_op_t<FpBN254>(op, a, b, out) : fe_op_t<FrBN254>(op, a, b, out), "field", op);
    if (curve == APK_BLS12_381) return selftest_status(field ? fe_op_t<FpBLS12381>(op, a, b, out) : fe_op_t<FrBLS12381>(op, a, b, out), "field", op);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_host_g1_op(int curve, int op, const void* p, const void* q, void* out) {
    if (!p || !out || (op != 2 && !q)) { set_error("null argument"); return APK_ERR_ARG; }
    if (curve == APK_BN254) return selftest_status(g1_op_t<FrBN254, FpBN254>(op, p, q, out), "g1", op);
    if (curve == APK_BLS12_381) return selftest_status(g1_op_t<FrBLS12381, FpBLS12381>(op, p, q, out), "g1", op);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_feu_shape(int curve, int field, int* ul, int* ub, uint32_t* headroom) {
    if (!ul || !ub || !headroom) { set_error("null argument"); return APK_ERR_ARG; }
    if (curve == APK_BN254) { field ? feu_shape_t<FpBN254>(ul, ub, headroom) : feu_shape_t<FrBN254>(ul, ub, headroom); return APK_OK; }
    if (curve == APK_BLS12_381) { field ? feu_shape_t<FpBLS12381>(ul, ub, headroom) : feu_shape_t<FrBLS12381>(ul, ub, headroom); return APK_OK; }
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_host_feu_op(int curve, int field, int op, uint64_t count, const void* in, void* out) {
    if (count && (!in || !out)) { set_error("null argument"); return APK_ERR_ARG; }
    const uint32_t* i = static_cast<const uint32_t*>(in);
    uint32_t* o = static_cast<uint32_t*>(out);
    if (curve == APK_BN254) return field ? host_feu_batch<FpBN254>(op, count, i, o) : host_feu_batch<FrBN254>(op, count, i, o);
    if (curve == APK_BLS12_381) return field ? host_feu_batch<FpBLS12381>(op, count, i, o) : host_feu_batch<FrBLS12381>(op, count, i, o);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_device_fe_op(int curve, int field, int op, int device, uint64_t count, const void* a, const void* b, void* out) {
    if (count && (!a || !b || !out)) { set_error("null argument"); return APK_ERR_ARG; }
    if (!seam_args(curve, count, (op >= 0 && op <= 4) || (op >= 10 && op <= 14), op, "field")) return APK_ERR_ARG;
    if (count == 0) return APK_OK;
    runtime_checkpoint();
    return curve == APK_BN254 ? fe_op_device_bn254(device, field, op, count, a, b, out) : fe_op_device_bls12381(device, field, op, count, a, b, out);
}

int apk_device_feu_op(int curve, int field, int op, int device, uint64_t count, const void* in, void* out) {
    if (count && (!in || !out)) { set_error("null argument"); return APK_ERR_ARG; }
    if (!seam_args(curve, count, (op >= 0 && op <= 29) || (op >= 40 && op <= 48), op, "unsaturated")) return APK_ERR_ARG;
    if (count == 0) return APK_OK;
    runtime_checkpoint();
    return curve == APK_BN254 ? feu_op_device_bn254(device, field, op, count, in, out) : feu_op_device_bls12381(device, field, op, count, in, out);
}

int apk_device_g1_op(int curve, int op, int device, uint64_t count, const void* p, const void* q, void* out) {
    const bool unary = op == 2 || op == 21;
    if (count && (!p || !out || (!unary && !q))) { set_error("null argument"); return APK_ERR_ARG; }
    if (!seam_args(curve, count, (op >= 0 && op <= 3) || (op >= 10 && op <= 15) || op == 20 || op == 21, op, "g1")) return APK_ERR_ARG;
    if (count == 0) return APK_OK;
    runtime_checkpoint();
    return curve == APK_BN254 ? g1_op_device_bn254(device, op, count, p, q, out) : g1_op_device_bls12381(device, op, count, p, q, out);
}

int apk_device_poly_op(int curve, int op, int device, const apk_poly_args* args) {
    if (curve != APK_BN254 && curve != APK_BLS12_381) { set_error("unsupported curve: %d", curve); return APK_ERR_ARG; }
    if (const char* why = poly_op_check(op, args)) { set_error("polynomial-stage op %d: %s", op, why); return APK_ERR_ARG; }
    runtime_checkpoint();
    return curve == APK_BN254 ? poly_op_device_bn254(device, op, args) : poly_op_device_bls12381(device, op, args);
}

int apk_g1_sum(int curve, const void* points, uint64_t count, void* out) {
    if (!out || (count && !points)) { set_error("null argument"); return APK_ERR_ARG; }
    if (curve == APK_BN254) return g1_sum_t<FpBN254>(points, count, out);
    if (curve == APK_BLS12_381) return g1_sum_t<FpBLS12381>(points, count, out);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_fe_from_be(int curve, int field, const uint8_t* be, void* out) {
    if (!be || !out) { set_error("null argument"); return APK_ERR_ARG; }
    return host_fe_from_be(curve, field, be, out);
}
int apk_fe_to_be(int curve, int field, const void* in, uint8_t* be) {
    if (!be || !in) { set_error("null argument"); return APK_ERR_ARG; }
    return host_fe_to_be(curve, field, in, be);
}

// the wire formats themselves: proof_codec.h (the readers live beside the verifier, verify_api.cpp)
int apk_marshal_proof(const apk_proof* p, uint8_t* out, size_t cap, size_t* len) {
    if (!p || !out || !len) { set_error("null argument"); return APK_ERR_ARG; }
    CodecError err;
    const int rc = marshal_proof(p, out, cap, len, &err);
    if (rc != APK_OK) set_error("%s", err.msg);
    return rc;
}

int apk_marshal_public_inputs(int curve, const void* pub, uint32_t nb_public, uint8_t* out, size_t cap) {
    if ((!pub && nb_public) || !out) { set_error("null argument"); return APK_ERR_ARG; }
    CodecError err;
    const int rc = marshal_public_inputs(curve, pub, nb_public, out, cap, &err);
    if (rc != APK_OK) set_error("%s", err.msg);
    return rc;
}

int apk_hash_fr(int curve, const void* g1_affine, void* out_fr) {
    if (!g1_affine || !out_fr) { set_error("null argument"); return APK_ERR_ARG; }
    if (!apk_g1_bytes(curve)) { set_error("unsupported curve: %d", curve); return APK_ERR_ARG; }
    auto hash = [&](auto proto) {
        using Proto = decltype(proto);
        typename Proto::Aff p;
        memcpy(&p, g1_affine, sizeof p);
        const typename Proto::Fr r = Proto::hash_fr(p);
        memcpy(out_fr, &r, sizeof r);
    };
    if (curve == APK_BN254) hash(PlonkProtocol<FrBN254, FpBN254>{}); else hash(PlonkProtocol<FrBLS12381, FpBLS12381>{});
    return APK_OK;
}

}  // extern "C"

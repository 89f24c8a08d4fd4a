// Curve-erased interface between the C-ABI (apk_api.cpp) and the per-curve HIP backends
// (backend_impl.h, instantiated in backend_bn254.hip / backend_bls12381.hip).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/apk.h"

namespace apk {

void set_error(const char* fmt, ...);

// Run-time knob from the environment, clamped to [lo, hi] (a value outside the range can never reach a launch configuration
// or an allocation size: nothing may abort across the C-ABI); `dflt` when the variable is unset or not a number.
int env_int(const char* name, int dflt, int lo, int hi);

// is this apk_ctx* still a live context (created and not yet destroyed)?  apk_api.cpp keeps the registry.
bool ctx_alive(const void* ctx);

// The device-wide scheduler (device_sched.h): one per device ordinal, created on first use, alive until the process ends;
// null when APK_DEVICE_SCHED=0 (every context then keeps a stream pool and a budget of its own).  apk_api.cpp keeps the registry.
class DeviceSched;
DeviceSched* device_sched_for(int device);
// the device's proving streams (hipStream_t), max_streams of them, created on the first call and never destroyed: lent to the
// contexts whose leads hold the matching stream ids
int device_stream_pool(int device, void** streams, int cap, int* count);

struct Backend {
    virtual ~Backend() {}
    virtual int init(const apk_circuit_desc* d) = 0;
    virtual int init_msm_only(int device, const void* bases, uint64_t count, int msm_window) = 0;
    virtual int get_vk(apk_vk* out) = 0;
    virtual int msm(int basis, const void* scalars, uint64_t len, bool on_device, void* out) = 0;
    virtual int msm_batch(int basis, uint32_t count, const void* const* d_scalars, const uint64_t* offsets, const uint64_t* lens, void* out) = 0;
    virtual int kzg_open(const void* poly, uint64_t len, bool on_device, const void* point, void* out_h, void* out_value) = 0;
    virtual int kzg_batch_open(uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, const void* digests,
                               const void* point, const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) = 0;
    // count (polynomial, point) pairs, one H and one value each
    virtual int kzg_open_multi(uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, const void* points,
                               void* out_h, void* out_values) = 0;
    // the same over the Lagrange SRS, from the n values on the domain (circuit contexts only: APK_ERR_STATE on an MSM-only one)
    virtual int kzg_open_lagrange(const void* evals, uint64_t len, bool on_device, const void* point, void* out_h, void* out_value) = 0;
    virtual int kzg_batch_open_lagrange(uint32_t count, const void* const* evals, bool on_device, const void* digests, const void* point,
                                        const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) = 0;
    // count (vector, point) pairs in evaluation form, one H and one value each
    virtual int kzg_open_multi_lagrange(uint32_t count, const void* const* evals, bool on_device, const void* points, void* out_h,
                                        void* out_values) = 0;
    // the openings of one polynomial at every point of the domain (kzg_all_run.h); circuit contexts only
    virtual int kzg_all_prepare(const void* srs_g1, uint64_t count) = 0;
    virtual int kzg_open_all(const void* poly, uint64_t len, bool on_device, void* out_h, void* out_values) = 0;
    // the openings of one polynomial on every coset of coset_size points of the domain (kzg_cosets_run.h); circuit contexts only
    virtual int kzg_cosets_prepare(const void* srs_g1, uint64_t count, uint32_t coset_size) = 0;
    virtual int kzg_open_cosets(const void* poly, uint64_t len, bool on_device, void* out_h, void* out_values) = 0;
    // the same for `count` polynomials in one call, polynomial-major (kzg_cosets_multi_run.h); ALL its argument rules are checked here
    virtual int kzg_open_cosets_multi(uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, void* out_h,
                                      void* out_values) = 0;
    // the polynomial back from `count` of its cells (kzg_recover_run.h); circuit contexts only, no prepare call
    virtual int kzg_recover_cosets(uint32_t coset_size, uint32_t count, const uint64_t* indices, const void* values, uint64_t len, bool on_device,
                                   void* out_poly) = 0;
    virtual int set_commit_hook(apk_commit_hook fn, void* user) = 0;
    virtual int dev_copy(void* d, const void* s, size_t bytes) = 0;
    virtual int set_wire_hook(apk_wire_hook fn, void* user) = 0;
    virtual int set_subcoset(int k, int G, apk_gather_hook fn, void* user) = 0;
    virtual int device_ordinal() = 0;
    virtual int msm_window() = 0;         // the signed-digit window width the context's tables were built for
    virtual uint64_t domain_size() = 0;   // n; 0 on an MSM-only context
    virtual int coset_ntt_dev(const void* d_in, uint64_t len, void* d_out) = 0;
    virtual int ntt(int which, int inverse, int coset, void* data) = 0;
    virtual int prove(const void* L, const void* R, const void* O, bool on_device, const void* pub, const void* blinding,
                      const void* const* pi2, apk_proof* out) = 0;
    virtual int dev_alloc(size_t bytes, void** p) = 0;
    virtual int dev_free(void* p) = 0;
    virtual int dev_upload(void* d, const void* s, size_t bytes) = 0;
    virtual int dev_download(void* d, const void* s, size_t bytes) = 0;
    virtual int stats_enable(int enable) = 0;
    virtual int stats_read(apk_stats* out, int reset) = 0;
    virtual int paths_read(apk_path_counts* out, int reset) = 0;
};

int g1_mul_batch_bn254(int device, const void* base, const void* scalars, uint64_t count, void* out);
int g1_mul_batch_bls12381(int device, const void* base, const void* scalars, uint64_t count, void* out);
int g1_decompress_bn254(int device, const uint8_t* in, uint64_t count, void* out);
int g1_decompress_bls12381(int device, const uint8_t* in, uint64_t count, void* out);
int g1_to_lagrange_bn254(int device, const void* points, uint64_t n, void* out);
int g1_to_lagrange_bls12381(int device, const void* points, uint64_t n, void* out);
// the test seams (include/apk.h apk_device_fe_op / apk_device_feu_op / apk_device_g1_op): one op per lane, host buffers in and out
int fe_op_device_bn254(int device, int field, int op, uint64_t count, const void* a, const void* b, void* out);
int fe_op_device_bls12381(int device, int field, int op, uint64_t count, const void* a, const void* b, void* out);
int feu_op_device_bn254(int device, int field, int op, uint64_t count, const void* in, void* out);
int feu_op_device_bls12381(int device, int field, int op, uint64_t count, const void* in, void* out);
int g1_op_device_bn254(int device, int op, uint64_t count, const void* p, const void* q, void* out);
int g1_op_device_bls12381(int device, int op, uint64_t count, const void* p, const void* q, void* out);
// the polynomial-stage seam (include/apk.h apk_device_poly_op): one stage of kernels_poly.h, host arrays in and out
int poly_op_device_bn254(int device, int op, const apk_poly_args* args);
int poly_op_device_bls12381(int device, int op, const apk_poly_args* args);
// the batch verifier's device half (kernels_lincomb.h; lincomb_bn254.hip / lincomb_bls12381.hip): host arrays in and out
int g1_lincomb_segments_bn254(int device, const void* points, const void* scalars, const uint64_t* seg, uint32_t nb_segments, void* out);
int g1_lincomb_segments_bls12381(int device, const void* points, const void* scalars, const uint64_t* seg, uint32_t nb_segments, void* out);
int g1_check_points_bn254(int device, const void* points, uint64_t count, uint8_t* flags);      // bit 0: off the curve, bit 1: outside the subgroup
int g1_check_points_bls12381(int device, const void* points, uint64_t count, uint8_t* flags);
// the fold of many coset openings' values (kernels_kzg_cosets_fold.h, in the same two units): q_c = sum_k scale_k step_k^c U_(k,c) over
// `count` host rows of 2^log_l Fr, 1 <= log_l <= 10; tw: the 512 powers of the inverse 1 024-th root; count = 0 only opens the device
int kzg_cosets_fold_bn254(int device, int log_l, uint32_t count, const void* values, const void* scale, const void* step, const void* tw, void* out);
int kzg_cosets_fold_bls12381(int device, int log_l, uint32_t count, const void* values, const void* scale, const void* step, const void* tw, void* out);
Backend* make_backend_bn254();
Backend* make_backend_bls12381();

// host-only helpers implemented per curve (no GPU): used by marshal / conversions / hash_fr
int host_fe_from_be(int curve, int field, const uint8_t* be, void* out);
int host_fe_to_be(int curve, int field, const void* in, uint8_t* be);

}  // namespace apk

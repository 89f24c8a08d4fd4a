// The runner of apk_kzg_recover_cosets: the context's one table, a slot's scratch and the launch sequences over them, beside the
// kernels (kernels_kzg_recover.h) and free of the prover - no slot, gate, gang, NTT or MSM.  Every function queues plain launches
// on `st` and returns; the backend (backend_impl.h kzg_recover_cosets) picks the slot, runs the three size-n NTTs between the
// sequences and waits.  The grids, the LDS bytes and the coefficient range of the check are kzg_recover_plan.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_buf.h"
#include "kernels_kzg_recover.h"
#include "poly_run.h"     // PlainLaunch, poly_tail_nonzero

namespace apk {

// A slot's scratch, allocated on its first call, all or none, and freed with the context.  The coset size is the CALL's, so the
// part that depends on n' grows when a call brings more cosets than any before it (the slot is the caller's alone meanwhile, and
// every earlier call on it has been waited for).
//   sc     2n scalars: a (E, then PG and Q in place) and b (P, then f) - no transform reads what it writes
//   small  3n' scalars: zH, 1 / zG, the roots
//   idx    n' int32 (the row map), n' uint32 (the missing cosets), the flag word of the tail check
// BN254 at 2^17, l = 64: 8 MiB + 192 KiB + 16 KiB; BLS12-381 at 2^14, l = 64: 1 MiB + 24 KiB + 2 KiB.
template <class FRP>
struct KzgRecoverScratch {
    using Fr = Fe<FRP>;
    DevBuf sc, small, idx;
    uint32_t n = 0, np_cap = 0;
    uint32_t epoch = 0;          // of the last call on this slot: what a non-zero tail stamps into the flag word
    void release() { sc.release(); small.release(); idx.release(); n = 0; np_cap = 0; }
    int ensure(hipStream_t st, uint32_t n_, uint32_t np) {      // (the flag word is cleared on the caller's stream: ordered before its launches)
        if (sc.p && np <= np_cap) return APK_OK;
        int rc = sc.p ? APK_OK : sc.alloc((size_t)2 * n_ * sizeof(Fr));
        if (rc == APK_OK) rc = small.alloc((size_t)3 * np * sizeof(Fr));
        if (rc == APK_OK) rc = idx.alloc((size_t)2 * np * sizeof(uint32_t) + 16);
        if (rc == APK_OK && hipMemsetAsync(flag_at(np), 0, 16, st) != hipSuccess) { set_error("kzg: recovery scratch"); rc = APK_ERR_HIP; }
        if (rc != APK_OK) { release(); return rc; }
        n = n_; np_cap = np;
        return APK_OK;
    }
    Fr* a() const { return ptr<Fr>(sc); }
    Fr* b() const { return ptr<Fr>(sc) + n; }
    Fr* zh() const { return ptr<Fr>(small); }
    Fr* zg_inv() const { return ptr<Fr>(small) + np_cap; }
    Fr* roots() const { return ptr<Fr>(small) + (size_t)2 * np_cap; }
    int32_t* row_of() const { return ptr<int32_t>(idx); }
    uint32_t* missing() const { return ptr<uint32_t>(idx) + np_cap; }
    uint32_t* flag() const { return flag_at(np_cap); }
    uint32_t* flag_at(uint32_t np) const { return ptr<uint32_t>(idx) + (size_t)2 * np; }
};

// Steps (1) and (2): the plan's row map and missing cosets (host memory the caller keeps until it has waited) to the device, the
// roots, zH and 1 / zG, then E in ks.a().  values: device, k rows of l.  tw: the context's w^e, e < n / 2, Montgomery.  gl = g^l.
template <class FRP>
int kzg_recover_scatter(hipStream_t st, const RecoverPlan& p, const KzgRecoverScratch<FRP>& ks, const Fe<FRP>* values, const Fe<FRP>* tw,
                        const Fe<FRP>& gl) {
    HIPCHK(hipMemcpyAsync(ks.row_of(), p.row_of.data(), (size_t)p.np * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (p.m) {
        HIPCHK(hipMemcpyAsync(ks.missing(), p.missing.data(), (size_t)p.m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        kzg_recover_roots_kernel<FRP><<<cdiv(p.m, KZG_RECOVER_THREADS), KZG_RECOVER_THREADS, 0, st>>>(ks.missing(), p.m, tw, p.log_l, p.n / 2, ks.roots());
        KCHK();
    }
    kzg_recover_vanish_kernel<FRP><<<p.vanish.grid, p.vanish.block, 0, st>>>(ks.roots(), p.m, tw, p.np, p.log_l, p.n / 2, gl, ks.zh(), ks.zg_inv());
    KCHK();
    kzg_recover_scatter_kernel<FRP><<<p.scatter.grid, p.scatter.block, 0, st>>>(values, ks.row_of(), ks.zh(), p.n, p.log_np, p.log_l, ks.a());
    KCHK();
    return APK_OK;
}

// Step (5), in place on ks.a()
template <class FRP>
int kzg_recover_divide(hipStream_t st, const RecoverPlan& p, const KzgRecoverScratch<FRP>& ks) {
    kzg_recover_divide_kernel<FRP><<<p.divide.grid, p.divide.block, 0, st>>>(ks.a(), ks.zg_inv(), p.n, p.np);
    KCHK();
    return APK_OK;
}

// f in ks.b(): the coefficients in [check_lo, check_hi) must be zero - a non-zero word stamps the call's epoch into the flag
// word, which is copied to *h_flag - and, for a device destination, the check_lo coefficients go out unless it did.
template <class FRP>
int kzg_recover_finish(hipStream_t st, const RecoverPlan& p, KzgRecoverScratch<FRP>& ks, Fe<FRP>* d_out, uint32_t* h_flag) {
    static_assert(sizeof(Fe<FRP>) == 2 * sizeof(uint4), "a scalar is two 16-byte records of tail_nonzero_kernel");
    ks.epoch++;
    if (p.check_hi > p.check_lo)
        CHK(poly_tail_nonzero(PlainLaunch{}, st, reinterpret_cast<const uint4*>(ks.b() + p.check_lo), (uint32_t)(2 * (p.check_hi - p.check_lo)), ks.epoch, ks.flag()));
    HIPCHK(hipMemcpyAsync(h_flag, ks.flag(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (d_out) {
        kzg_recover_emit_kernel<FRP><<<cdiv((uint32_t)p.check_lo, KZG_RECOVER_THREADS), KZG_RECOVER_THREADS, 0, st>>>(ks.b(), (uint32_t)p.check_lo, ks.flag(), ks.epoch, d_out);
        KCHK();
    }
    return APK_OK;
}

}  // namespace apk

// The runner of apk_kzg_open_all: the context's tables, a slot's scratch and the launch sequences over them, beside the kernels
// (kernels_kzg_all.h) and free of the prover - no slot, gate, gang, NTT or MSM.  Every function queues plain launches on `st` and
// returns; the backend (backend_impl.h kzg_fk20_*) picks the slot, runs the three size-n NTTs that make A^ and the values, and waits.
// The integer rules - which lanes of the gather share a launch - are kzg_fk20_plan.h's; kzg_fk20_tail, the sequence from the pointwise
// products to the affine results, is shared with kzg_cosets_run.h, where it runs over n' = n / l points.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_buf.h"
#include "kernels_kzg_all.h"
#include "kzg_fk20_plan.h"
#include "msm_plan.h"      // cdiv

namespace apk {

// What the context keeps once apk_kzg_all_prepare has run; read-only afterwards.
//   that      T^ = DFT_2n of the reversed SRS: 2n affine points, natural order
//   glv       the split of w_2n^j, j < n (APK_KZG_ALL_GLV=1)
//   tw_inv    w_2n^(-j), j < n, Montgomery (APK_KZG_ALL_GLV=0: lagrange_stage_kernel's table of the inverse size-2n transform)
//   pre       w_2n^m, m < n, in the NTT's radix: the `pre` operand that makes the odd half of A^
//   scale     1 / (2n) in the NTT's radix: the inverse transform's factor, carried by A^
template <class FRP, class FPP>
struct KzgAllTables {
    DevBuf that, glv, tw_inv, pre, scale;
    Fe<FPP> beta;          // Montgomery
    bool use_glv = false;
    void release() { that.release(); glv.release(); tw_inv.release(); pre.release(); scale.release(); }
};

// A slot's scratch, allocated on its first call, all or none, and freed with the context.
//   work      2n XYZZ points: the size-2n transform, then in its first n points the size-n transform; the n affine results are
//             written behind them (n affine points fit the n XYZZ points the gather has left free)
//   sc        3n scalars: the even half of A^, the odd half, the values f(w^i)
template <class FRP, class FPP>
struct KzgAllScratch {
    using Fr = Fe<FRP>;
    using Pt = XYZZ<FPP>;
    using Aff = Affine<FPP>;
    DevBuf work, sc;
    uint32_t n = 0;
    int ensure(uint32_t n_) {
        if (work.p) return APK_OK;
        n = n_;
        CHK(work.alloc((size_t)2 * n * sizeof(Pt)));
        const int rc = sc.alloc((size_t)3 * n * sizeof(Fr));
        if (rc != APK_OK) work.release();
        return rc;
    }
    Pt* points() const { return ptr<Pt>(work); }
    Aff* result() const { return reinterpret_cast<Aff*>(ptr<Pt>(work) + n); }
    Fr* a_even() const { return ptr<Fr>(sc); }
    Fr* a_odd() const { return ptr<Fr>(sc) + n; }
    Fr* values() const { return ptr<Fr>(sc) + (size_t)2 * n; }
};

// log(points) stages over work[0 .. points): bit-reversed in, natural out.  log_n2 = log(2n), the size the tables were made for.
// plain_tw: the plain form's table for this transform and direction (powers of its generator, Montgomery, points / 2 entries).
// stages >= 0: only the first `stages` of them, which leaves points >> stages transforms of 2^stages points side by side, block b
// the one of the elements b' + (points >> stages) u, b' = b bit-reversed (kzg_cosets_run.h).
template <class FRP, class FPP>
int kzg_all_stages(hipStream_t st, const KzgAllTables<FRP, FPP>& T, XYZZ<FPP>* work, uint32_t points, int log_points, int log_n2,
                   bool inverse, const Fe<FRP>* plain_tw, int stages = -1) {
    const uint32_t half = points / 2, n_tab = 1u << (log_n2 - 1);
    for (int t = 0; t < (stages < 0 ? log_points : stages); t++) {
        if (T.use_glv)
            kzg_all_stage_glv_kernel<FPP><<<cdiv(half, KZG_ALL_THREADS), KZG_ALL_THREADS, 0, st>>>(work, ptr<KzgAllTwiddle>(T.glv), T.beta, half, t,
                                                                                                  log_n2 - 1 - t, n_tab, inverse ? 1 : 0);
        else
            lagrange_stage_kernel<FRP, FPP><<<cdiv(half, 128), 128, 0, st>>>(work, plain_tw, points, log_points, t);
        KCHK();
    }
    return APK_OK;
}

// T^ = DFT_2n(t): d_t = the 2n affine points (s_(n-2) .. s_0, infinity x (n+1)); T.that receives the result.  work: 2n points.
// tw_fwd: powers of w_2n, n entries (plain form only).
template <class FRP, class FPP>
int kzg_all_build_that(hipStream_t st, const KzgAllTables<FRP, FPP>& T, const Affine<FPP>* d_t, uint32_t n, int log_n, XYZZ<FPP>* work,
                       const Fe<FRP>* tw_fwd) {
    const uint32_t n2 = 2 * n;
    lagrange_load_kernel<FPP><<<cdiv(n2, 256), 256, 0, st>>>(d_t, n2, log_n + 1, work);
    KCHK();
    CHK((kzg_all_stages<FRP, FPP>(st, T, work, n2, log_n + 1, log_n + 1, false, tw_fwd)));
    kzg_all_finish_kernel<FPP><<<cdiv(n2, KZG_ALL_THREADS), KZG_ALL_THREADS, 0, st>>>(work, n2, ptr<Affine<FPP>>(T.that));
    KCHK();
    return APK_OK;
}

// The tail of both open calls: from the pointwise products in work (2m points, bit-reversed) to the m affine results.  Inverse
// stages over 2m points (work = c, natural order), the gather launches kzg_fk20_plan.h lists (fk20_gather: which lanes may share a
// launch - two launches from m = 8 on), forward stages over m points, finish.  tw_inv: w_2m^(-j), j < m; tw_fwd: w_m^j, j < m / 2
// (Montgomery, plain form only).
template <class FRP, class FPP>
int kzg_fk20_tail(hipStream_t st, const KzgAllTables<FRP, FPP>& T, XYZZ<FPP>* work, uint32_t m, int log_m, int log_n2, const Fe<FRP>* tw_inv,
                  const Fe<FRP>* tw_fwd, Affine<FPP>* result) {
    CHK((kzg_all_stages<FRP, FPP>(st, T, work, 2 * m, log_m + 1, log_n2, true, tw_inv)));
    const Fk20Gather g = fk20_gather(m);
    for (int i = 0; i < g.count; i++) {
        const Fk20Range r = g.launch[i];
        kzg_all_gather_kernel<FPP><<<cdiv(r.k1 - r.k0, KZG_ALL_THREADS), KZG_ALL_THREADS, 0, st>>>(work, m, log_m, r.k0, r.k1);
        KCHK();
    }
    CHK((kzg_all_stages<FRP, FPP>(st, T, work, m, log_m, log_n2, false, tw_fwd)));
    kzg_all_finish_kernel<FPP><<<cdiv(m, KZG_ALL_THREADS), KZG_ALL_THREADS, 0, st>>>(work, m, result);
    KCHK();
    return APK_OK;
}

// From A^ (ks.a_even(), ks.a_odd()) to the n openings in ks.result().  tw_n: powers of w, n / 2 entries, Montgomery (plain form).
template <class FRP, class FPP>
int kzg_all_open(hipStream_t st, const KzgAllTables<FRP, FPP>& T, const KzgAllScratch<FRP, FPP>& ks, uint32_t n, int log_n,
                 const Fe<FRP>* tw_n) {
    kzg_all_pointwise_kernel<FRP, FPP><<<cdiv(2 * n, KZG_ALL_THREADS), KZG_ALL_THREADS, 0, st>>>(ks.a_even(), ks.a_odd(), ptr<Affine<FPP>>(T.that), 2 * n,
                                                                                                log_n + 1, ks.points());
    KCHK();
    return kzg_fk20_tail<FRP, FPP>(st, T, ks.points(), n, log_n, log_n + 1, ptr<Fe<FRP>>(T.tw_inv), tw_n, ks.result());
}

}  // namespace apk

// The runner of apk_kzg_open_cosets: the context's table, a slot's scratch and the launch sequences over them, beside the kernels
// (kernels_kzg_cosets.h) and free of the prover - no slot, gate, gang, NTT or MSM.  Every function queues plain launches on `st`
// and returns; the backend (backend_impl.h kzg_cosets_*) picks the slot, runs the size-n NTT of the values and the 2l size-n'
// NTTs that make A^, and waits.  The stages in the exponent are kzg_all_run.h's (kzg_all_stages) over the twiddles of
// KzgAllTables, which whichever of apk_kzg_all_prepare and apk_kzg_cosets_prepare runs first builds; so is the sequence behind the
// pointwise sums (kzg_fk20_tail).  The integer rules of both calls are kzg_fk20_plan.h's.
// The batched form - many polynomials per call, side by side in these launches (apk_kzg_open_cosets_multi) - lives in
// kzg_cosets_multi_run.h and kernels_kzg_cosets_multi.h; it reads the tables below and leaves this path alone.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_buf.h"
#include "kernels_kzg_cosets.h"
#include "kzg_all_run.h"

namespace apk {

// What the context keeps once apk_kzg_cosets_prepare has run; read-only afterwards.  n' = n / l.
//   tab       tab[(4 i + v) l + c] = [2^(64 v)] T^_c[i]: 8n affine points (kernels_kzg_cosets.h "THE TABLE")
//   pre       w_2n'^u, u < n', in the NTT's radix: the `pre` operand that makes the odd half of every A^_c
//   scale     1 / (2n') / R in the NTT's radix (R = 2^256, the Montgomery radix): the inverse transform's factor, and A^ comes out
//             of the NTT as plain integers
//   tw_inv    w_2n'^(-j), j < n', Montgomery;  tw_fwd  (w^l)^j, j < n' / 2, Montgomery (APK_KZG_ALL_GLV=0: lagrange_stage_kernel's
//             tables of the inverse size-2n' and the forward size-n' transform)
struct KzgCosetsTables {
    DevBuf tab, pre, scale, tw_inv, tw_fwd;
    uint32_t l = 0;
    int log_l = 0;
    void release() { tab.release(); pre.release(); scale.release(); tw_inv.release(); tw_fwd.release(); l = 0; log_l = 0; }
};

// A slot's scratch, allocated on its first call, all or none, and freed with the context.  (The 2n-point transform of the prepare
// call runs in the slot's KzgAllScratch.)
//   work      2n' XYZZ points: the size-2n' transform, then in its first n' points the size-n' transform; the n' affine results
//             are written behind them (as in KzgAllScratch)
//   sc        5n scalars: the l gathered sequences a_c, the even halves of A^_c, the odd halves, NTT_n(f), the same coset-major
// BN254 at 2^17, l = 64: 384 KiB + 20 MiB; BLS12-381 at 2^14, l = 64: 96 KiB + 2.5 MiB.
template <class FRP, class FPP>
struct KzgCosetsScratch {
    using Fr = Fe<FRP>;
    using Pt = XYZZ<FPP>;
    using Aff = Affine<FPP>;
    DevBuf work, sc;
    uint32_t n = 0, np = 0;
    int ensure(uint32_t n_, uint32_t np_) {
        if (work.p) return APK_OK;
        n = n_; np = np_;
        CHK(work.alloc((size_t)2 * np * sizeof(Pt)));
        const int rc = sc.alloc((size_t)5 * n * sizeof(Fr));
        if (rc != APK_OK) work.release();
        return rc;
    }
    Pt* points() const { return ptr<Pt>(work); }
    Aff* result() const { return reinterpret_cast<Aff*>(ptr<Pt>(work) + np); }
    Fr* gathered() const { return ptr<Fr>(sc); }
    Fr* a_even() const { return ptr<Fr>(sc) + n; }
    Fr* a_odd() const { return ptr<Fr>(sc) + (size_t)2 * n; }
    Fr* values() const { return ptr<Fr>(sc) + (size_t)3 * n; }
    Fr* values_by_coset() const { return ptr<Fr>(sc) + (size_t)4 * n; }
};

// The table from d_t = 2n affine points with d_t[c + l u] = t_c[u] (u < 2n'): loaded bit-reversed over all 2n points, the first
// log(2n') stages transform the l sequences side by side.  work: 2n points.  tw_fwd: powers of w_2n, n entries (plain form only).
template <class FRP, class FPP>
int kzg_cosets_build_table(hipStream_t st, const KzgAllTables<FRP, FPP>& T, const KzgCosetsTables& C, const Affine<FPP>* d_t, uint32_t n,
                           int log_n, XYZZ<FPP>* work, const Fe<FRP>* tw_fwd) {
    const uint32_t n2 = 2 * n;
    const int log_np2 = log_n + 1 - C.log_l;
    lagrange_load_kernel<FPP><<<cdiv(n2, 256), 256, 0, st>>>(d_t, n2, log_n + 1, work);
    KCHK();
    CHK((kzg_all_stages<FRP, FPP>(st, T, work, n2, log_n + 1, log_n + 1, false, tw_fwd, log_np2)));
    kzg_cosets_table_kernel<FPP><<<cdiv(n2, 128), 128, 0, st>>>(work, n2, log_np2, C.log_l, ptr<Affine<FPP>>(C.tab));
    KCHK();
    return APK_OK;
}

// f (len coefficients) to the l sequences a_c in ks.gathered()
template <class FRP, class FPP>
int kzg_cosets_split(hipStream_t st, const KzgCosetsTables& C, const KzgCosetsScratch<FRP, FPP>& ks, const Fe<FRP>* f, uint32_t len,
                     uint32_t n, int log_n) {
    kzg_cosets_split_kernel<FRP><<<cdiv(n, 256), 256, 0, st>>>(f, len, n, log_n - C.log_l, C.log_l, ks.gathered());
    KCHK();
    return APK_OK;
}

// ks.values() = NTT_n(f) to ks.values_by_coset()
template <class FRP, class FPP>
int kzg_cosets_values(hipStream_t st, const KzgCosetsTables& C, const KzgCosetsScratch<FRP, FPP>& ks, uint32_t n, int log_n) {
    kzg_cosets_values_kernel<FRP><<<cdiv(n, 256), 256, 0, st>>>(ks.values(), n, log_n - C.log_l, C.log_l, ks.values_by_coset());
    KCHK();
    return APK_OK;
}

// From A^ (ks.a_even(), ks.a_odd()) to the n' proofs in ks.result(): the pointwise sums, then kzg_all_run.h's tail over n' points.
// log_n = log of the context's domain (the twiddle records are those of the size-2n domain).
template <class FRP, class FPP>
int kzg_cosets_open(hipStream_t st, const KzgAllTables<FRP, FPP>& T, const KzgCosetsTables& C, const KzgCosetsScratch<FRP, FPP>& ks,
                    uint32_t n, int log_n) {
    using Fr = Fe<FRP>;
    const int log_np = log_n - C.log_l;
    const uint32_t np = n >> C.log_l, np2 = 2 * np;
    const int log_group = fk20_pointwise_log_group(C.log_l);
    const uint32_t per_block = (uint32_t)KZG_COSETS_THREADS >> log_group;
    kzg_cosets_pointwise_kernel<FRP, FPP><<<cdiv(np2, per_block), KZG_COSETS_THREADS, 0, st>>>(ks.a_even(), ks.a_odd(), ptr<Affine<FPP>>(C.tab), np2,
                                                                                              log_np + 1, C.log_l, log_group, ks.points());
    KCHK();
    return kzg_fk20_tail<FRP, FPP>(st, T, ks.points(), np, log_np, log_n + 1, ptr<Fr>(C.tw_inv), ptr<Fr>(C.tw_fwd), ks.result());
}

}  // namespace apk

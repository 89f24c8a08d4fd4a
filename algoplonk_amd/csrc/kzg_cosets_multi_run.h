// The runner of apk_kzg_open_cosets_multi: a slot's scratch for a group of G polynomials and the launch sequences over it, beside the
// kernels (kernels_kzg_cosets_multi.h) and free of the prover - no slot, gate, gang, NTT or MSM.  Every function queues plain
// launches on `st` and returns; the backend (backend_impl.h kzg_open_cosets_multi) picks the slot, walks the planner's groups, runs
// the G size-n NTTs of the values and the 2 G l size-n' NTTs that make A^, and waits once.  The context's table and twiddles are the
// single call's (kzg_cosets_run.h KzgCosetsTables, kzg_all_run.h KzgAllTables), the stages in the exponent kzg_all_stages as it
// stands, and every index, size and grid kzg_fk20_plan.h's (Fk20Multi).
#pragma once
#include <hip/hip_runtime.h>

#include "dev_buf.h"
#include "kernels_kzg_cosets_multi.h"
#include "kzg_cosets_run.h"

namespace apk {

// A slot's scratch, allocated on its first such call, all or none, and freed with the context; released and allocated again when a
// call brings a larger group than any before it (before anything is queued: the slot's stream is idle then).
//   pts       3 G n' XYZZ points: `second` (G n'), then `work` (G 2n'); the G n' affine results are written where work was
//   sc        5 G n scalars: the rows a_(b,c), the even halves of A^, the odd halves, NTT_n(f_b), the same coset-major
//   up        G n scalars: the host form's uploads
// G = 16, l = 64: BN254 at 2^17 12 MiB + 320 MiB + 64 MiB, BLS12-381 at 2^14 2.25 MiB + 40 MiB + 8 MiB.
template <class FRP, class FPP>
struct KzgCosetsMultiScratch {
    using Fr = Fe<FRP>;
    using Pt = XYZZ<FPP>;
    using Aff = Affine<FPP>;
    DevBuf pts, sc, up;
    uint32_t G = 0;      // the group the areas are laid out for (at most `cap`, the one they were allocated for)
    uint32_t cap = 0;
    size_t n = 0, np = 0;
    int ensure(const Fk20Multi& m) {
        G = m.G; n = m.s.n; np = m.s.np;
        if (m.G <= cap) return APK_OK;
        release();
        int rc = pts.alloc(m.scratch_points() * sizeof(Pt));
        if (rc == APK_OK) rc = sc.alloc(m.scratch_scalars() * sizeof(Fr));
        if (rc == APK_OK) rc = up.alloc(m.upload_scalars() * sizeof(Fr));
        if (rc != APK_OK) { release(); return rc; }
        cap = m.G;
        return APK_OK;
    }
    void release() { pts.release(); sc.release(); up.release(); cap = 0; }
    Pt* second() const { return ptr<Pt>(pts); }
    Pt* work() const { return ptr<Pt>(pts) + G * np; }
    Aff* result() const { return reinterpret_cast<Aff*>(work()); }
    Fr* gathered() const { return ptr<Fr>(sc); }
    Fr* a_even() const { return ptr<Fr>(sc) + G * n; }
    Fr* a_odd() const { return ptr<Fr>(sc) + 2 * G * n; }
    Fr* values() const { return ptr<Fr>(sc) + 3 * G * n; }
    Fr* values_by_coset() const { return ptr<Fr>(sc) + 4 * G * n; }
    Fr* upload(uint32_t b) const { return ptr<Fr>(up) + b * n; }
};

// ks.values() = NTT_n(f_b), b < G, to ks.values_by_coset()
template <class FRP, class FPP>
int kzg_cosets_multi_values(hipStream_t st, const Fk20Multi& m, const KzgCosetsMultiScratch<FRP, FPP>& ks) {
    kzg_cosets_values_multi_kernel<FRP><<<m.grid_scalars(), 256, 0, st>>>(ks.values(), m.G * m.s.n, m.s.log_n, m.s.log_np, m.s.log_l, ks.values_by_coset());
    KCHK();
    return APK_OK;
}

// f_b (len_b coefficients), b < G, to the G l rows a_(b,c) in ks.gathered()
template <class FRP, class FPP>
int kzg_cosets_multi_split(hipStream_t st, const Fk20Multi& m, const KzgCosetsMultiScratch<FRP, FPP>& ks, const KzgCosetsMultiSrc<FRP>& src) {
    kzg_cosets_split_multi_kernel<FRP><<<m.grid_scalars(), 256, 0, st>>>(src, m.G * m.s.n, m.s.log_n, m.s.log_np, m.s.log_l, ks.gathered());
    KCHK();
    return APK_OK;
}

// From A^ (ks.a_even(), ks.a_odd()) to the G n' proofs in ks.result(): the pointwise sums over the context's table, log(2n') inverse
// stages over G 2n' points, the gather to the second array, log(n') forward stages over G n' points, finish.  log_n2 = log(2n), the
// size the twiddle records were made for.
template <class FRP, class FPP>
int kzg_cosets_multi_open(hipStream_t st, const KzgAllTables<FRP, FPP>& T, const KzgCosetsTables& C, const Fk20Multi& m,
                          const KzgCosetsMultiScratch<FRP, FPP>& ks) {
    using Fr = Fe<FRP>;
    const Fk20Shape& s = m.s;
    const int log_n2 = s.log_n + 1;
    kzg_cosets_pointwise_multi_kernel<FRP, FPP><<<dim3(m.grid_pointwise_x(), m.grid_pointwise_y()), KZG_COSETS_THREADS, 0, st>>>(
        ks.a_even(), ks.a_odd(), ptr<Affine<FPP>>(C.tab), s.pair_big(), s.log_np + 1, s.log_l, fk20_pointwise_log_group(s.log_l), ks.work());
    KCHK();
    CHK((kzg_all_stages<FRP, FPP>(st, T, ks.work(), m.big_points(), s.log_np + 1, log_n2, true, ptr<Fr>(C.tw_inv))));
    kzg_cosets_gather_multi_kernel<FPP><<<m.grid_points(), KZG_ALL_THREADS, 0, st>>>(ks.work(), m.small_points(), s.np, s.log_np, ks.second());
    KCHK();
    CHK((kzg_all_stages<FRP, FPP>(st, T, ks.second(), m.small_points(), s.log_np, log_n2, false, ptr<Fr>(C.tw_fwd))));
    kzg_all_finish_kernel<FPP><<<m.grid_points(), KZG_ALL_THREADS, 0, st>>>(ks.second(), m.small_points(), ks.result());
    KCHK();
    return APK_OK;
}

}  // namespace apk

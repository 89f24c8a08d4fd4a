// The KZG openings' runner: a slot's scratch and the launch sequences of an opening on it, beside the kernels (kernels_kzg.h,
// kernels_kzg_lagrange.h) and free of the prover - no slot, gate, gang, MSM or transcript.  Every function queues its launches
// on `st` and returns; the backend (backend_impl.h kzg_*) picks the slot, commits the quotient and waits.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>

#include "dev_buf.h"
#include "gang_kernel.h"   // poly1_kernel: a kernel functor launched alone
#include "kernels_kzg.h"
#include "kernels_kzg_lagrange.h"
#include "slot_pinned.h"

namespace apk {

// The scratch of a slot's openings, allocated on the slot's first one for polynomials of up to `bases` coefficients (the SRS),
// and the only place that knows its layout.
//   coefficient form   q: the quotient.  aux: KZG_MAX_POLYS rows of workgroup totals (row stride = the workgroups of the longest
//                      polynomial the SRS takes), then KZG_MAX_POLYS values
//   evaluation form    q: the n inverses 1 / (w^i - z), then the quotient's n values in place; the word that receives m when
//                      z = w^m sits in element n (the MSM reads n scalars).  aux: KZG_MAX_POLYS rows of workgroup partials (row
//                      stride = lag_blocks(n); the workgroups' products before them and the quotient's partials after them use
//                      row 0), then KZG_MAX_POLYS values.  Both fit what ensure() allocates when fits() says so.
//   evaluation form at several points (kzg_lag_group_open): row r of a group keeps its inverses, then in place its quotient, in
//                      quot_row(r) and its m word in element n of that row (ensure_multi() sizes every row like q: n + 1 <= bases);
//                      row r of aux (stride lag_blocks(n), r < KZG_GROUP <= KZG_MAX_POLYS) carries that row's workgroup
//                      products, then its partial sums, then its quotient's partials; the rows' values go to the front of the
//                      same value area.  Nothing beyond what fits() already guarantees.
template <class FRP>
struct KzgScratch {
    using Fr = Fe<FRP>;
    static_assert(PIN_FR + KZG_MAX_POLYS * sizeof(Fr) <= PIN_TAIL, "the values fit the pinned buffer's scalar area");
    DevBuf q, aux;
    uint32_t bases = 0;
    static uint32_t blocks(uint32_t len) { return (uint32_t)(((uint64_t)len + KZG_BLOCK_SPAN - 1) / KZG_BLOCK_SPAN); }      // workgroups over len coefficients
    static uint32_t lag_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + KZG_LAG_BLOCK_SPAN - 1) / KZG_LAG_BLOCK_SPAN); }   // ... over n values
    static size_t aux_elems(uint32_t bases) {
        const size_t rows = (size_t)KZG_MAX_POLYS * blocks(bases) + KZG_MAX_POLYS;
        return rows > bases ? rows : bases;
    }
    static bool fits(uint32_t bases, uint32_t n) { return (size_t)n + 1 <= bases && (size_t)KZG_MAX_POLYS * lag_blocks(n) + KZG_MAX_POLYS <= aux_elems(bases); }
    int ensure(uint32_t bases_) {      // all or nothing
        if (q.p) return APK_OK;
        bases = bases_;
        CHK(q.alloc((size_t)bases * sizeof(Fr)));
        const int rc = aux.alloc(aux_elems(bases) * sizeof(Fr));
        if (rc != APK_OK) q.release();
        return rc;
    }
    // openings at several points: the further quotient vectors of a group of `width` <= KZG_GROUP rows (row 0 uses q), each sized
    // like q, allocated on the slot's first such call - a context's width never changes.  All or nothing.
    DevBuf q_more[KZG_GROUP - 1];
    int ensure_multi(uint32_t bases_, uint32_t width) {
        CHK(ensure(bases_));
        if (width < 2 || q_more[width - 2].p) return APK_OK;
        for (uint32_t i = 0; i + 1 < width; i++) {
            const int rc = q_more[i].alloc((size_t)bases * sizeof(Fr));
            if (rc == APK_OK) continue;
            while (i-- > 0) q_more[i].release();
            return rc;
        }
        return APK_OK;
    }
    Fr* quot_row(uint32_t r) const { return r ? ptr<Fr>(q_more[r - 1]) : quot(); }
    Fr* quot() const { return ptr<Fr>(q); }
    Fr* rows() const { return ptr<Fr>(aux); }
    uint32_t row_stride() const { return blocks(bases); }
    Fr* values() const { return rows() + (size_t)KZG_MAX_POLYS * row_stride(); }
    Fr* lag_values(uint32_t n) const { return rows() + (size_t)KZG_MAX_POLYS * lag_blocks(n); }
    uint32_t* lag_at(uint32_t n) const { return reinterpret_cast<uint32_t*>(quot() + n); }
    uint32_t* lag_at_row(uint32_t r, uint32_t n) const { return reinterpret_cast<uint32_t*>(quot_row(r) + n); }
};

// The vectors of a batch as the kernels' argument; host vectors get device copies in `staged` (count buffers) for the length of
// the call - a convenience form: callers on the hot path keep theirs resident.
template <class FRP>
int kzg_stage(uint32_t count, const void* const* vecs, const uint64_t* lens, bool on_device, std::vector<DevBuf>& staged, KzgPolys<FRP>& a) {
    using Fr = Fe<FRP>;
    a.count = count;
    for (uint32_t i = 0; i < count; i++) {
        a.len[i] = (uint32_t)lens[i];
        if (a.len[i] > a.max_len) a.max_len = a.len[i];
        a.f[i] = reinterpret_cast<const Fr*>(vecs[i]);
        if (on_device) continue;
        CHK(staged[i].alloc(lens[i] * sizeof(Fr)));
        HIPCHK(hipMemcpy(staged[i].p, vecs[i], lens[i] * sizeof(Fr), hipMemcpyHostToDevice));
        a.f[i] = ptr<Fr>(staged[i]);
    }
    return APK_OK;
}

// The vectors of `count` (vector, point) pairs on the device, d_vec[i]; host vectors get device copies in `staged` (count buffers)
// for the length of the call - a pointer that occurs several times is staged once, as long as its longest use.
template <class FRP>
int kzg_stage_pairs(uint32_t count, const void* const* vecs, const uint64_t* lens, bool on_device, std::vector<DevBuf>& staged, const Fe<FRP>** d_vec) {
    using Fr = Fe<FRP>;
    for (uint32_t i = 0; i < count; i++) {
        d_vec[i] = reinterpret_cast<const Fr*>(vecs[i]);
        if (on_device) continue;
        uint32_t first = i;
        uint64_t longest = lens[i];
        for (uint32_t j = 0; j < count; j++)
            if (vecs[j] == vecs[i]) { if (j < first) first = j; if (lens[j] > longest) longest = lens[j]; }
        if (first < i) { d_vec[i] = d_vec[first]; continue; }
        CHK(staged[i].alloc(longest * sizeof(Fr)));
        HIPCHK(hipMemcpy(staged[i].p, vecs[i], longest * sizeof(Fr), hipMemcpyHostToDevice));
        d_vec[i] = ptr<Fr>(staged[i]);
    }
    return APK_OK;
}

// ---- the two forms of an opening ----------------------------------------------------------------------------------------------
// A form holds the point and queues, on `st` and over the scratch `ks`:
//   evaluate   the a.count values, into the scratch's value area and on their way to h_val - written there by the last kernel
//              through d_pinned_val (the device's view of h_val) where the form can and there is one, else copied
//   divide     the quotient of the fold (weights a.coef) into ks.quot(): quot_len(a) scalars for the MSM over the form's SRS.
//              vals: the values the host folded with, null for a single opening.
// VALUES_FIRST: a single opening evaluates before it divides (else its value falls out of the division, to h_val).

// coefficient form (kernels_kzg.h), over the canonical SRS: any length the scratch takes, any point
template <class FRP>
struct KzgCoefForm {
    using Fr = Fe<FRP>;
    static constexpr bool VALUES_FIRST = false;
    static constexpr const char* NOUN = "polynomials";
    Fr z;
    const Fr& point() const { return z; }
    static uint32_t quot_len(const KzgPolys<FRP>& a) { return a.max_len - 1; }     // 0: a constant, the quotient is the zero polynomial
    int evaluate(hipStream_t st, const KzgScratch<FRP>& ks, const KzgPolys<FRP>& a, Fr*, void* h_val) const {
        Fr* d_val = ks.values();
        KzgRows<FRP> rows{};
        rows.tot = ks.rows(); rows.stride = ks.row_stride();
        for (uint32_t i = 0; i < a.count; i++) rows.len[i] = a.len[i];
        poly1_kernel<KzgEvalBlockK<FRP>, KZG_THREADS><<<dim3(ks.blocks(a.max_len), a.count), KZG_THREADS, 0, st>>>(a, z, rows);
        KCHK();
        poly1_kernel<KzgCarryK<FRP>, KZG_THREADS><<<a.count, KZG_THREADS, 0, st>>>(rows, z, d_val);
        KCHK();
        HIPCHK(hipMemcpyAsync(h_val, d_val, a.count * sizeof(Fr), hipMemcpyDeviceToHost, st));
        return APK_OK;
    }
    // three launches and the value's copy: the fold's value is recomputed on the device, with a.coef
    int divide(hipStream_t st, const KzgScratch<FRP>& ks, const KzgPolys<FRP>& a, const Fr*, void* h_val) const {
        const uint32_t L = a.max_len, nb = ks.blocks(L);
        Fr* q = ks.quot();
        Fr* tot = ks.rows();
        Fr* d_val = ks.values();
        KzgRows<FRP> rows{};
        rows.tot = tot; rows.stride = ks.row_stride(); rows.len[0] = L;
        poly1_kernel<KzgFoldBlockK<FRP>, KZG_THREADS><<<nb, KZG_THREADS, 0, st>>>(a, z, q, tot);
        KCHK();
        poly1_kernel<KzgCarryK<FRP>, KZG_THREADS><<<1, KZG_THREADS, 0, st>>>(rows, z, d_val);
        KCHK();
        if (nb > 1) {      // (the last workgroup has no carry)
            poly1_kernel<KzgApplyK<FRP>, KZG_THREADS><<<nb - 1, KZG_THREADS, 0, st>>>((const Fr*)tot, z, L, q);
            KCHK();
        }
        HIPCHK(hipMemcpyAsync(h_val, d_val, sizeof(Fr), hipMemcpyDeviceToHost, st));
        return APK_OK;
    }
};

// Openings at several points, coefficient form: the launches of ONE group of rows <= KZG_GROUP openings, each a polynomial at its
// own point (g.f, g.len, g.z filled in by the caller; g.q is set here).  Row r's quotient lands in ks.quot_row(r) - len[r] - 1
// scalars for the MSM - its workgroup totals use row r of the scratch's rows, and the rows' values go to the front of the value
// area and from there to h_val.  Needs ks.ensure_multi() for at least `rows` rows.
template <class FRP>
int kzg_group_divide(hipStream_t st, const KzgScratch<FRP>& ks, KzgGroup<FRP>& g, uint32_t rows, void* h_val) {
    using Fr = Fe<FRP>;
    uint32_t longest = 0;
    for (uint32_t r = 0; r < rows; r++) {
        g.q[r] = ks.quot_row(r);
        if (g.len[r] > longest) longest = g.len[r];
    }
    const uint32_t nb = ks.blocks(longest);
    Fr* tot = ks.rows();
    Fr* d_val = ks.values();
    poly1_kernel<KzgGroupBlockK<FRP>, KZG_THREADS><<<dim3(nb, rows), KZG_THREADS, 0, st>>>(g, tot, ks.row_stride());
    KCHK();
    poly1_kernel<KzgGroupCarryK<FRP>, KZG_THREADS><<<rows, KZG_THREADS, 0, st>>>(g, tot, ks.row_stride(), d_val);
    KCHK();
    if (nb > 1) {      // (a row's last workgroup has no carry)
        poly1_kernel<KzgGroupApplyK<FRP>, KZG_THREADS><<<dim3(nb - 1, rows), KZG_THREADS, 0, st>>>(g, (const Fr*)tot, ks.row_stride());
        KCHK();
    }
    HIPCHK(hipMemcpyAsync(h_val, d_val, rows * sizeof(Fr), hipMemcpyDeviceToHost, st));
    return APK_OK;
}

// scale = (z^n - 1)/n; on_domain: z^n == 1; whole = 1/(z^n - 1), on the domain 1/n (kernels_kzg_lagrange.h)
template <class FRP>
struct KzgLagPoint { Fe<FRP> z, scale, whole; uint32_t on_domain; };
template <class FRP>
KzgLagPoint<FRP> kzg_lag_point(const void* point, uint32_t log_n, const Fe<FRP>& n_inv) {
    using Fr = Fe<FRP>;
    KzgLagPoint<FRP> pt;
    memcpy(&pt.z, point, sizeof pt.z);
    Fr zn = pt.z;
    for (uint32_t i = 0; i < log_n; i++) zn = Fr::sqr(zn);
    pt.on_domain = zn == Fr::one() ? 1u : 0u;
    pt.scale = (zn - Fr::one()) * n_inv;
    pt.whole = pt.on_domain ? n_inv : Fr::inv(zn - Fr::one());
    return pt;
}
// evaluation form (kernels_kzg_lagrange.h), over the Lagrange SRS: n values on the domain of w; tw[k] = w^k for k < n/2
template <class FRP>
struct KzgLagForm {
    using Fr = Fe<FRP>;
    static constexpr bool VALUES_FIRST = true;
    static constexpr const char* NOUN = "vectors";
    KzgLagPoint<FRP> pt;
    const Fr* tw;
    uint32_t n;
    const Fr& point() const { return pt.z; }
    uint32_t quot_len(const KzgPolys<FRP>&) const { return n; }
    // launches 1a, 1b and 2: the inverses, then the values
    int evaluate(hipStream_t st, const KzgScratch<FRP>& ks, const KzgPolys<FRP>& a, Fr* d_pinned_val, void* h_val) const {
        const uint32_t nb = ks.lag_blocks(n);
        Fr* part = ks.rows();
        Fr* d_val = ks.lag_values(n);
        uint32_t* at = ks.lag_at(n);
        // (the workgroup products borrow row 0 of the partials: launch 1b has read them before launch 2 writes there)
        poly1_kernel<KzgLagProdK<FRP>, KZG_THREADS><<<nb, KZG_THREADS, 0, st>>>(tw, n, pt.z, part, at);
        KCHK();
        poly1_kernel<KzgLagInvK<FRP>, KZG_THREADS><<<nb, KZG_THREADS, 0, st>>>(tw, n, pt.z, (const Fr*)part, pt.whole, pt.on_domain, (const uint32_t*)at, ks.quot());
        KCHK();
        if (!pt.on_domain) {
            poly1_kernel<KzgLagSumK<FRP>, KZG_THREADS><<<dim3(nb, a.count), KZG_THREADS, 0, st>>>(a, tw, n, (const Fr*)ks.quot(), part);
            KCHK();
        }
        poly1_kernel<KzgLagValueK<FRP>, KZG_THREADS><<<a.count, KZG_THREADS, 0, st>>>(a, (const Fr*)part, nb, pt.scale, pt.on_domain, (const uint32_t*)at, d_val, d_pinned_val);
        KCHK();
        if (!d_pinned_val) HIPCHK(hipMemcpyAsync(h_val, d_val, a.count * sizeof(Fr), hipMemcpyDeviceToHost, st));
        return APK_OK;
    }
    // launch 3.  The fold's value: sum gamma^i vals[i] by value or, without vals, the one evaluate() left on the device.
    int divide(hipStream_t st, const KzgScratch<FRP>& ks, const KzgPolys<FRP>& a, const Fr* vals, void*) const {
        const uint32_t nb = ks.lag_blocks(n);
        Fr* q = ks.quot();
        Fr* part = ks.rows();
        const uint32_t* at = ks.lag_at(n);
        const Fr* d_v = vals ? nullptr : ks.lag_values(n);
        Fr v = vals ? vals[0] : Fr::zero();
        for (uint32_t i = 1; vals && i < a.count; i++) v = v + a.coef[i] * vals[i];
        poly1_kernel<KzgLagQuotK<FRP>, KZG_THREADS><<<nb, KZG_THREADS, 0, st>>>(a, tw, n, d_v, v, pt.on_domain, at, q, part);
        KCHK();
        if (pt.on_domain) {
            poly1_kernel<KzgLagFillK<FRP>, KZG_THREADS><<<1, KZG_THREADS, 0, st>>>(tw, n, (const Fr*)part, nb, at, q);
            KCHK();
        }
        return APK_OK;
    }
};

// Openings at several points, evaluation form: the launches of ONE group of rows <= KZG_GROUP openings, each a vector of n values
// at its own point (g.f, g.z, g.scale, g.whole, g.on_domain filled in by the caller from kzg_lag_point; g.q and g.at are set
// here).  Row r's quotient lands in ks.quot_row(r) - n scalars for the MSM over the Lagrange SRS - and the rows' values go to
// the front of the value area and from there to h_val.  At most six launches whatever the number of rows; the sum launch is left
// out when every row is on the domain, the fill launch when none is.  Needs ks.ensure_multi() for at least `rows` rows and
// ks.fits(bases, n).
template <class FRP>
int kzg_lag_group_open(hipStream_t st, const KzgScratch<FRP>& ks, KzgLagGroup<FRP>& g, uint32_t rows, uint32_t n, const Fe<FRP>* tw, void* h_val) {
    using Fr = Fe<FRP>;
    uint32_t on = 0;
    for (uint32_t r = 0; r < rows; r++) {
        g.q[r] = ks.quot_row(r);
        g.at[r] = ks.lag_at_row(r, n);
        if (g.on_domain[r]) on++;
    }
    const uint32_t nb = ks.lag_blocks(n);
    Fr* aux = ks.rows();
    Fr* d_val = ks.lag_values(n);
    const dim3 grid(nb, rows);
    poly1_kernel<KzgLagGroupProdK<FRP>, KZG_THREADS><<<grid, KZG_THREADS, 0, st>>>(g, tw, n, aux, nb);
    KCHK();
    poly1_kernel<KzgLagGroupInvK<FRP>, KZG_THREADS><<<grid, KZG_THREADS, 0, st>>>(g, tw, n, (const Fr*)aux, nb);
    KCHK();
    if (on < rows) {
        poly1_kernel<KzgLagGroupSumK<FRP>, KZG_THREADS><<<grid, KZG_THREADS, 0, st>>>(g, tw, n, aux, nb);
        KCHK();
    }
    poly1_kernel<KzgLagGroupValueK<FRP>, KZG_THREADS><<<rows, KZG_THREADS, 0, st>>>(g, (const Fr*)aux, nb, nb, n, d_val);
    KCHK();
    poly1_kernel<KzgLagGroupQuotK<FRP>, KZG_THREADS><<<grid, KZG_THREADS, 0, st>>>(g, tw, n, (const Fr*)d_val, aux, nb);
    KCHK();
    if (on) {
        poly1_kernel<KzgLagGroupFillK<FRP>, KZG_THREADS><<<rows, KZG_THREADS, 0, st>>>(g, tw, n, (const Fr*)aux, nb, nb);
        KCHK();
    }
    HIPCHK(hipMemcpyAsync(h_val, d_val, rows * sizeof(Fr), hipMemcpyDeviceToHost, st));
    return APK_OK;
}

}  // namespace apk

// apk_kzg_recover_cosets_host (include/apk.h): steps (1) - (6) of kernels_kzg_recover.h on the calling thread, in host field
// arithmetic with a radix-2 transform like the one coset_interpolate (kzg_protocol.h) uses.  Host only: no HIP include, builds
// with plain g++.  The rules are kzg_recover_plan.h's, the result bytes the device call's: it is what the CPU tier and the
// stand-alone sanitizer program (tools/san/kzg_recover_check.cpp) exercise, and the GPU tier's second witness.
#pragma once
#include <string.h>
#include <utility>
#include <vector>

#include "ff.h"
#include "kzg_recover_plan.h"

namespace apk {

template <class FRP>
struct KzgRecoverHost {
    using Fr = Fe<FRP>;

    static Fr from_u64(uint64_t v) {
        Fr a = Fr::zero();
        a.l[0] = (uint32_t)v;
        a.l[1] = (uint32_t)(v >> 32);
        return Fr::to_mont(a);
    }
    static Fr domain_root(int log_n) {      // the generator of the domain of 2^log_n points, Montgomery
        Fr a;
        for (int i = 0; i < Fr::N; i++) a.l[i] = FRP::root(i);
        Fr w = Fr::to_mont(a);
        for (int i = 0; i < FRP::ADICITY - log_n; i++) w = Fr::sqr(w);
        return w;
    }
    // v[t] = sum_c v[c] root^(c t), in place; root generates the domain of 2^log points
    static void transform(std::vector<Fr>& v, int log, const Fr& root) {
        const uint32_t n = 1u << log;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t j = 0;
            for (int b = 0; b < log; b++) j |= ((i >> b) & 1u) << (log - 1 - b);
            if (i < j) std::swap(v[i], v[j]);
        }
        for (int t = 0; t < log; t++) {
            const uint32_t half = 1u << t;
            const Fr wt = Fr::pow_u64(root, (uint64_t)(n >> (t + 1)));
            for (uint32_t base = 0; base < n; base += 2 * half) {
                Fr tw = Fr::one();
                for (uint32_t k = 0; k < half; k++) {
                    const Fr u = v[base + k], x = v[base + k + half] * tw;
                    v[base + k] = u + x;
                    v[base + k + half] = u - x;
                    tw = tw * wt;
                }
            }
        }
    }

    // values: k rows of l; out: len coefficients, written only with APK_OK.  APK_OK or APK_ERR_VERIFY.
    static int run(const RecoverPlan& p, const Fr* values, uint64_t len, Fr* out) {
        const uint32_t n = p.n, np = p.np, l = p.l;
        const Fr w = domain_root(p.log_n), w_inv = Fr::inv(w), g = from_u64(FRP::COSET_SHIFT), g_inv = Fr::inv(g);
        const Fr n_inv = Fr::inv(from_u64(n)), wl = Fr::pow_u64(w, l), gl = Fr::pow_u64(g, l);
        // (1)
        std::vector<Fr> a(np), zh(np, Fr::one()), zg_inv(np, Fr::one());
        Fr cur = Fr::one();
        for (uint32_t t = 0; t < np; t++) { a[t] = cur; cur = cur * wl; }
        for (uint32_t t = 0; t < np; t++) {
            const Fr y = gl * a[t];
            for (uint32_t i : p.missing) { zh[t] = zh[t] * (a[t] - a[i]); zg_inv[t] = zg_inv[t] * (y - a[i]); }
            zg_inv[t] = Fr::inv(zg_inv[t]);
        }
        // (2), (3)
        std::vector<Fr> e(n, Fr::zero());
        for (uint32_t i = 0; i < np; i++)
            if (p.row_of[i] >= 0)
                for (uint32_t j = 0; j < l; j++) e[i + (size_t)np * j] = values[(size_t)p.row_of[i] * l + j] * zh[i];
        transform(e, p.log_n, w_inv);
        // (4): P(g w^q); the 1 / n of (3) rides in the powers of g
        cur = n_inv;
        for (uint32_t c = 0; c < n; c++) { e[c] = e[c] * cur; cur = cur * g; }
        transform(e, p.log_n, w);
        // (5), (6)
        for (uint32_t q = 0; q < n; q++) e[q] = e[q] * zg_inv[q & (np - 1)];
        transform(e, p.log_n, w_inv);
        cur = n_inv;
        for (uint32_t c = 0; c < n; c++) { e[c] = e[c] * cur; cur = cur * g_inv; }
        for (uint64_t c = p.check_lo; c < p.check_hi; c++)
            if (!e[c].is_zero()) return APK_ERR_VERIFY;
        memcpy(out, e.data(), (size_t)len * sizeof(Fr));
        return APK_OK;
    }
};

// the whole call behind the C-ABI: `values` and `out_poly` as the caller holds them (any alignment)
template <class FRP>
inline RecoverVerdict kzg_recover_host(uint64_t n, uint32_t l, uint32_t count, const uint64_t* indices, const void* values, uint64_t len, void* out_poly) {
    RecoverVerdict v = recover_check_call(l, count, len);
    if (v.rc != APK_OK) return v;
    if (n < 4 || (n & (n - 1)) || n > (1ull << 24) || __builtin_ctzll(n) > FRP::ADICITY) {
        v.rc = APK_ERR_ARG;
        snprintf(v.message, sizeof v.message, "kzg: a domain of %llu points (a power of two in [4, 2^24])", (unsigned long long)n);
        return v;
    }
    const RecoverPlan p = recover_plan(n, l, count, indices, len);
    if (p.verdict.rc != APK_OK) return p.verdict;
    std::vector<Fe<FRP>> rows((size_t)count * l), f((size_t)len);
    memcpy(rows.data(), values, rows.size() * sizeof(Fe<FRP>));
    v.rc = KzgRecoverHost<FRP>::run(p, rows.data(), len, f.data());
    if (v.rc == APK_OK) memcpy(out_poly, f.data(), f.size() * sizeof(Fe<FRP>));
    else snprintf(v.message, sizeof v.message, "kzg: the cells are not those of one polynomial of %llu coefficients (a non-zero coefficient in [%llu, %llu))",
                  (unsigned long long)len, (unsigned long long)p.check_lo, (unsigned long long)p.check_hi);
    return v;
}

}  // namespace apk

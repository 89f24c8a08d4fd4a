// Sanitizer tier: the host form of the recovery from cells (algoplonk_amd/csrc/kzg_recover_host.h, what
// apk_kzg_recover_cosets_host runs) and its planner driven stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer - no
// libapk, no GPU, no interpreter:
//     make -C algoplonk_amd/csrc san-kzg-recover && tools/san/kzg_recover_check
// For both curves and a list of (n, l, known cosets) it recovers from
//     "cells"   the cells of f_c = (c + 1)^3 + 7, c < k l, with len = k l (APK_OK: f itself) and len = k l - 1 (APK_ERR_VERIFY, the
//               destination - pre-filled - untouched),
//     "short"   the cells of the same polynomial cut to k l - l + 1 coefficients, with that len,
//     "rows"    arbitrary rows that are no polynomial's cells, with len = k l,
// checks the verdicts, that "cells" and "short" return f, and prints every case
//     R <curve> <n> <l> <len> <rc> : <indices> : <k l values, hex> : <len coefficients, hex>
// so that tests/test_kzg_recover_host.py can hold them to its big-integer model.  Prints KZG RECOVER CHECK OK when nothing is wrong.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../algoplonk_amd/csrc/kzg_recover_host.h"

using namespace apk;

template <class P>
static void print_fe(const Fe<P>& mont) {
    const Fe<P> a = Fe<P>::from_mont(mont);
    for (int i = Fe<P>::N - 1; i >= 0; i--) printf("%08x", a.l[i]);
}

template <class FR>
static int one_case(int curve, uint32_t n, uint32_t l, const std::vector<uint64_t>& idx, const std::vector<Fe<FR>>& rows, uint64_t len, int want_rc,
                    const std::vector<Fe<FR>>* want) {
    using Fr = Fe<FR>;
    std::vector<uint8_t> out((size_t)len * sizeof(Fr) + 1, 0xa5), before = out;
    // (out + 1: the call takes the caller's bytes at any alignment)
    const RecoverVerdict v = kzg_recover_host<FR>(n, l, (uint32_t)idx.size(), idx.data(), rows.data(), len, out.data() + 1);
    int bad = 0;
    if (v.rc != want_rc) { printf("curve %d n %u l %u len %llu: rc %d (%s), expected %d\n", curve, n, l, (unsigned long long)len, v.rc, v.message, want_rc); bad++; }
    if (v.rc != APK_OK && out != before) { printf("curve %d n %u l %u: the destination was written with rc %d\n", curve, n, l, v.rc); bad++; }
    std::vector<Fr> f((size_t)len);
    if (v.rc == APK_OK) memcpy(f.data(), out.data() + 1, (size_t)len * sizeof(Fr));
    if (v.rc == APK_OK && want)
        for (uint64_t c = 0; c < len; c++)
            if (f[c] != (c < want->size() ? (*want)[c] : Fr::zero())) { printf("curve %d n %u l %u: coefficient %llu differs\n", curve, n, l, (unsigned long long)c); bad++; break; }
    printf("R %d %u %u %llu %d :", curve, n, l, (unsigned long long)len, v.rc);
    for (uint64_t i : idx) printf(" %llu", (unsigned long long)i);
    printf(" :");
    for (const Fr& x : rows) { printf(" "); print_fe(x); }
    printf(" :");
    if (v.rc == APK_OK) for (const Fr& x : f) { printf(" "); print_fe(x); }
    printf("\n");
    return bad;
}

template <class FR>
static std::vector<Fe<FR>> cells_of(const std::vector<Fe<FR>>& f, int log_n, uint32_t l, const std::vector<uint64_t>& idx) {
    using H = KzgRecoverHost<FR>;
    using Fr = Fe<FR>;
    const uint32_t n = 1u << log_n, np = n / l;
    const Fr w = H::domain_root(log_n);
    std::vector<Fr> rows;
    for (uint64_t i : idx)
        for (uint32_t j = 0; j < l; j++) {
            const Fr x = Fr::pow_u64(w, i + (uint64_t)np * j);
            Fr acc = Fr::zero();
            for (size_t c = f.size(); c-- > 0;) acc = acc * x + f[c];
            rows.push_back(acc);
        }
    return rows;
}

template <class FR>
static int run(int curve, int log_n, uint32_t l, const std::vector<uint64_t>& idx) {
    using H = KzgRecoverHost<FR>;
    using Fr = Fe<FR>;
    const uint32_t n = 1u << log_n, k = (uint32_t)idx.size(), kl = k * l;
    std::vector<Fr> f(kl);
    for (uint32_t c = 0; c < kl; c++) { const Fr x = H::from_u64(c + 1); f[c] = x * x * x + H::from_u64(7); }
    int bad = 0;
    const std::vector<Fr> cells = cells_of<FR>(f, log_n, l, idx);
    bad += one_case<FR>(curve, n, l, idx, cells, kl, APK_OK, &f);
    bad += one_case<FR>(curve, n, l, idx, cells, kl - 1, APK_ERR_VERIFY, nullptr);
    std::vector<Fr> cut(f.begin(), f.begin() + (kl - l + 1));
    bad += one_case<FR>(curve, n, l, idx, cells_of<FR>(cut, log_n, l, idx), cut.size(), APK_OK, &cut);
    std::vector<Fr> rows(kl);
    for (uint32_t c = 0; c < kl; c++) rows[c] = H::from_u64(0x9e3779b97f4a7c15ull * (c + 3)) * H::from_u64(0xc2b2ae3d27d4eb4full + c) + H::from_u64(c);
    bad += one_case<FR>(curve, n, l, idx, rows, kl, APK_OK, nullptr);
    return bad;
}

int main() {
    struct Shape { int log_n; uint32_t l; std::vector<uint64_t> idx; };
    const std::vector<Shape> shapes = {
        {2, 2, {1}}, {3, 2, {3, 1}}, {3, 2, {0, 1, 2, 3}}, {3, 4, {1}}, {3, 4, {1, 0}}, {4, 4, {3, 0}}, {4, 2, {7, 2, 5, 0, 1}},
        {6, 8, {0, 2, 4, 6}}, {6, 2, {31, 1, 17, 8, 9, 30, 2, 3, 4, 5, 6, 7, 0, 16, 18, 19}},
    };
    int bad = 0;
    for (const Shape& s : shapes) {
        bad += run<FrBN254>(APK_BN254, s.log_n, s.l, s.idx);
        bad += run<FrBLS12381>(APK_BLS12_381, s.log_n, s.l, s.idx);
    }
    // the refusals reach the caller through the same entry
    uint8_t out[64];
    const uint64_t two[2] = {1, 1};
    const Fe<FrBN254> rows[4] = {};
    if (kzg_recover_host<FrBN254>(8, 2, 2, two, rows, 4, out).rc != APK_ERR_ARG) { printf("a repeated index was accepted\n"); bad++; }
    if (kzg_recover_host<FrBN254>(8, 2, 1, two, rows, 3, out).rc != APK_ERR_ARG) { printf("too few cells were accepted\n"); bad++; }
    if (kzg_recover_host<FrBN254>(12, 2, 1, two, rows, 2, out).rc != APK_ERR_ARG) { printf("n = 12 was accepted\n"); bad++; }
    if (bad) { printf("KZG RECOVER CHECK FAILED: %d\n", bad); return 1; }
    printf("KZG RECOVER CHECK OK: %zu shapes per curve\n", shapes.size());
    return 0;
}

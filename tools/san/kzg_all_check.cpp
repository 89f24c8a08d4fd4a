// Sanitizer tier: algoplonk_amd/csrc/kzg_all_twiddles.h (the twiddle split behind apk_kzg_open_all's stage kernel) driven stand-alone
// under AddressSanitizer + UndefinedBehaviorSanitizer - no libapk, no GPU, no interpreter:
//     make -C algoplonk_amd/csrc san-kzg-all && tools/san/kzg_all_check [log_2n]
// For both curves and every j < n (2n = 2^log_2n, default 2^12) it holds the table's record to
//     k1 + k2 lambda = w_2n^j (mod r),  |k1|, |k2| < 2^HALF_BITS,
// and the reflected record the inverse transforms read to  -(k1 + k2 lambda)[n - j] = w_2n^(-j).  Every record is printed
//     tw <curve> <j> <neg> <k1 hex> <k2 hex>
// after a line  lambda <curve> <hex> <omega_2n hex>  so that tests/test_kzg_all_host.py can hold them to the same rule in big integers.
// Prints KZG ALL CHECK OK when nothing is wrong.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../algoplonk_amd/csrc/backend.h"
#include "../../algoplonk_amd/csrc/kzg_all_twiddles.h"

namespace apk {
void set_error(const char*, ...) {}
int env_int(const char*, int dflt, int, int) { return dflt; }
}  // namespace apk

using namespace apk;

template <class FR>
static Fe<FR> from_words(const uint32_t* w, int count) {
    Fe<FR> a = Fe<FR>::zero();
    for (int i = 0; i < count && i < Fe<FR>::N; i++) a.l[i] = w[i];
    return Fe<FR>::to_mont(a);
}

template <class FR>
static void print_fe(const Fe<FR>& mont) {
    const Fe<FR> a = Fe<FR>::from_mont(mont);
    for (int i = Fe<FR>::N - 1; i >= 0; i--) printf("%08x", a.l[i]);
}

template <class FR, class FP>
static int run(int curve, int log_2n) {
    using Fr = Fe<FR>;
    using G = GlvParams<FP>;
    const uint32_t n = 1u << (log_2n - 1);
    const Fr w = kzg_all_root_2n<FR>(log_2n - 1);
    uint32_t lw[8];
    for (int i = 0; i < 4; i++) { lw[2 * i] = (uint32_t)G::lambda[i]; lw[2 * i + 1] = (uint32_t)(G::lambda[i] >> 32); }
    const Fr lambda = from_words<FR>(lw, 8);
    printf("lambda %d ", curve); print_fe(lambda); printf(" "); print_fe(w); printf("\n");
    std::vector<KzgAllTwiddle> tab;
    if (!kzg_all_split_table<FR, FP>(n, w, tab) || tab.size() != n) { printf("curve %d: the split failed\n", curve); return 1; }
    std::vector<Fr> value(n);
    Fr cur = Fr::one();
    int bad = 0;
    for (uint32_t j = 0; j < n; j++, cur = cur * w) {
        const KzgAllTwiddle& t = tab[j];
        // both halves below 2^HALF_BITS: nothing above bit HALF_BITS - 1 of the five words
        const uint32_t top = 32 * KZG_ALL_HALF_WORDS - G::HALF_BITS;
        if ((t.k1[KZG_ALL_HALF_WORDS - 1] >> (32 - top)) || (t.k2[KZG_ALL_HALF_WORDS - 1] >> (32 - top)) || t.neg > 3u || t.pad != 0u) bad++;
        Fr a = from_words<FR>(t.k1, KZG_ALL_HALF_WORDS), b = from_words<FR>(t.k2, KZG_ALL_HALF_WORDS);
        if (t.neg & 1u) a = Fr::neg(a);
        if (t.neg & 2u) b = Fr::neg(b);
        value[j] = a + b * lambda;
        if (value[j] != cur) bad++;
        printf("tw %d %u %u ", curve, j, t.neg);
        for (int i = KZG_ALL_HALF_WORDS - 1; i >= 0; i--) printf("%08x", t.k1[i]);
        printf(" ");
        for (int i = KZG_ALL_HALF_WORDS - 1; i >= 0; i--) printf("%08x", t.k2[i]);
        printf("\n");
    }
    // the reflection the inverse transforms use: w_2n^(-j) = -w_2n^(n - j), and the size-n transform's even entries
    cur = Fr::one();
    const Fr winv = Fr::inv(w);
    for (uint32_t j = 1; j < n; j++) {
        cur = cur * winv;
        if (Fr::neg(value[n - j]) != cur) bad++;
    }
    const Fr w_n = Fr::sqr(w);
    cur = Fr::one();
    for (uint32_t j = 0; j < n / 2; j++, cur = cur * w_n)
        if (value[2 * j] != cur) bad++;
    if (bad) printf("curve %d: %d records are wrong\n", curve, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    const int log_2n = argc > 1 ? atoi(argv[1]) : 12;
    if (log_2n < 4 || log_2n > 20) { printf("log_2n out of range\n"); return 2; }
    int rc = run<FrBN254, FpBN254>(0, log_2n);
    rc |= run<FrBLS12381, FpBLS12381>(1, log_2n);
    if (rc) return 1;
    printf("KZG ALL CHECK OK: %u twiddles per curve\n", 1u << (log_2n - 1));
    return 0;
}

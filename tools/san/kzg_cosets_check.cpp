// Sanitizer tier: the coset opening's host rule in algoplonk_amd/csrc/kzg_protocol.h (coset_interpolate, coset_check: what
// apk_kzg_verify_coset runs) driven stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer - no libapk, no GPU, no
// interpreter:
//     make -C algoplonk_amd/csrc san-kzg-cosets && tools/san/kzg_cosets_check
// For both curves and (n, l) = (8, 2), (8, 4), (64, 8), with a tau it knows, it opens f_k = (k + 1)^3 + 7 on every coset in the
// field - H_i = [(f(tau) - I_i(tau)) / (tau^l - a_i)] G1 - and holds
//     the interpolant of the coset's values to f mod (X^l - a_i), coefficient by coefficient,
//     coset_check to accept the first and the last coset, and to reject a changed value, the next index and [tau^(l/2)]G2.
// Every interpolant is printed
//     I <curve> <n> <l> <index> : <l values, hex> : <l coefficients, hex>
// so that tests/test_kzg_cosets_host.py can hold them to its big-integer model.  Prints KZG COSETS CHECK OK when nothing is wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../algoplonk_amd/csrc/backend.h"
#include "../../algoplonk_amd/csrc/kzg_protocol.h"

namespace apk {
void set_error(const char*, ...) {}
int env_int(const char*, int dflt, int, int) { return dflt; }
int g1_lincomb_segments_bn254(int, const void*, const void*, const uint64_t*, uint32_t, void*) { return APK_ERR_HIP; }
int g1_lincomb_segments_bls12381(int, const void*, const void*, const uint64_t*, uint32_t, void*) { return APK_ERR_HIP; }
}  // namespace apk

using namespace apk;

// the curves' G1 generators, big-endian hex
static const char* const G1_X[2] = {"1", "17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"};
static const char* const G1_Y[2] = {"2", "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1"};

template <class P>
static Fe<P> from_hex(const char* s) {
    Fe<P> a = Fe<P>::zero();
    const size_t len = strlen(s);
    for (size_t k = 0; k < len; k++) {
        const char ch = s[len - 1 - k];
        const uint32_t d = ch <= '9' ? (uint32_t)(ch - '0') : (uint32_t)(ch - 'a' + 10);
        if (k / 8 < (size_t)Fe<P>::N) a.l[k / 8] |= d << (4 * (k % 8));
    }
    return Fe<P>::to_mont(a);
}

template <class P>
static Fe<P> from_u64(uint64_t v) {
    Fe<P> a = Fe<P>::zero();
    a.l[0] = (uint32_t)v;
    a.l[1] = (uint32_t)(v >> 32);
    return Fe<P>::to_mont(a);
}

template <class P>
static void print_fe(const Fe<P>& mont) {
    const Fe<P> a = Fe<P>::from_mont(mont);
    for (int i = Fe<P>::N - 1; i >= 0; i--) printf("%08x", a.l[i]);
}

template <class Fr>
static Fr horner(const std::vector<Fr>& f, const Fr& z) {
    Fr acc = Fr::zero();
    for (size_t k = f.size(); k-- > 0;) acc = acc * z + f[k];
    return acc;
}

template <class FR, class FP, class PP, int CURVE_ID>
static int run(int log_n, int log_l) {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    using V = typename K::V;
    using Fr = Fe<FR>;
    using Aff = Affine<FP>;
    using G2 = typename K::G2;
    const uint32_t n = 1u << log_n, l = 1u << log_l, np = n / l;
    const Aff G{from_hex<FP>(G1_X[CURVE_ID]), from_hex<FP>(G1_Y[CURVE_ID])};
    if (G.is_inf() || !K::point_ok(G)) { printf("curve %d: the generator is not a point of the group\n", CURVE_ID); return 1; }
    const Fr tau = from_u64<FR>(0x9e3779b97f4a7c15ull) * from_u64<FR>(0xc2b2ae3d27d4eb4full) + from_u64<FR>(12345);
    const Fr w = K::domain_root(log_n);
    std::vector<Fr> f(n);
    for (uint32_t k = 0; k < n; k++) { const Fr x = from_u64<FR>(k + 1); f[k] = x * x * x + from_u64<FR>(7); }
    std::vector<Aff> srs(l);
    Fr tp = Fr::one();
    for (uint32_t c = 0; c < l; c++, tp = tp * tau) srs[c] = V::smul(G, tp).to_affine();
    const Fr tau_l = tp;
    G2 g2[2] = {G2::generator(), G2::template mul<FR>(G2::generator(), Fr::from_mont(tau_l))};
    G2 g2_half[2] = {g2[0], G2::template mul<FR>(G2::generator(), Fr::from_mont(Fr::pow_u64(tau, l / 2)))};
    const Fr ft = horner(f, tau);
    const Aff digest = V::smul(G, ft).to_affine();
    int bad = 0;
    for (uint32_t i = 0; i < np; i++) {
        const Fr a = Fr::pow_u64(w, (uint64_t)i * l);
        std::vector<Fr> values(l), rem(l, Fr::zero());
        for (uint32_t j = 0; j < l; j++) values[j] = horner(f, Fr::pow_u64(w, (uint64_t)i + (uint64_t)np * j));
        for (uint32_t c = 0; c < l; c++)
            for (uint32_t m = np; m-- > 0;) rem[c] = rem[c] * a + f[c + l * m];
        std::vector<Fr> co = values;
        K::coset_interpolate(log_n, log_l, i, co);
        printf("I %d %u %u %u :", CURVE_ID, n, l, i);
        for (const Fr& v : values) { printf(" "); print_fe(v); }
        printf(" :");
        for (const Fr& v : co) { printf(" "); print_fe(v); }
        printf("\n");
        for (uint32_t c = 0; c < l; c++) if (co[c] != rem[c]) bad++;
        const Fr hs = (ft - horner(rem, tau)) * Fr::inv(tau_l - a);
        const Aff H = V::smul(G, hs).to_affine();
        const char* why = "";
        if (i != 0 && i + 1 != np) continue;      // (the pairing checks on the first and the last coset: they are slow under the sanitizers)
        if (!K::coset_check(G, g2, srs.data(), log_n, log_l, i, digest, values.data(), H, &why)) { printf("coset %u: rejected (%s)\n", i, why); bad++; }
        if (i + 1 == np) {      // the rejections, once per shape
            std::vector<Fr> changed = values;
            changed[l - 1] = changed[l - 1] + Fr::one();
            if (K::coset_check(G, g2, srs.data(), log_n, log_l, i, digest, changed.data(), H, &why)) { printf("coset %u: a changed value was accepted\n", i); bad++; }
            if (K::coset_check(G, g2, srs.data(), log_n, log_l, i - 1, digest, values.data(), H, &why)) { printf("coset %u: accepted as coset %u\n", i, i - 1); bad++; }
            if (K::coset_check(G, g2_half, srs.data(), log_n, log_l, i, digest, values.data(), H, &why)) { printf("coset %u: accepted against [tau^(l/2)]G2\n", i); bad++; }
        }
    }
    if (bad) printf("curve %d n %u l %u: %d checks failed\n", CURVE_ID, n, l, bad);
    return bad ? 1 : 0;
}

int main() {
    static const int SHAPES[3][2] = {{3, 1}, {3, 2}, {6, 3}};
    int rc = 0;
    for (const auto& s : SHAPES) {
        rc |= run<FrBN254, FpBN254, PairBN254, APK_BN254>(s[0], s[1]);
        rc |= run<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(s[0], s[1]);
    }
    if (rc) { printf("KZG COSETS CHECK FAILED\n"); return 1; }
    printf("KZG COSETS CHECK OK: 3 shapes per curve\n");
    return 0;
}

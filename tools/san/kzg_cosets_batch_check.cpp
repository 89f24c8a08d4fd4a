// Sanitizer tier: the batched coset verifier's host rule in algoplonk_amd/csrc/kzg_protocol.h (cosets_weights, cosets_fold,
// cosets_check: what apk_kzg_batch_verify_cosets runs with device -1) driven stand-alone under AddressSanitizer +
// UndefinedBehaviorSanitizer - no libapk, no GPU, no interpreter:
//     make -C algoplonk_amd/csrc san-kzg-cosets-batch && tools/san/kzg_cosets_batch_check
// For both curves and (n, l) = (8, 2), (8, 4), (64, 8), with a tau it knows, it opens f_k = (k + 1)^3 + 7 and g_k = (k + 2)^2 on
// every coset in the field and holds cosets_check to
//     accept every coset of f in one batch, and the cosets of f and g interleaved (two digests),
//     give coset_check's verdict on a batch of one, good and bad,
//     reject a changed value, a row's digest_of pointing at the other polynomial, an index off by one and [tau^(l/2)]G2,
//     reject the same row twice with H + P in one copy and H - P in the other.
// The fold of the first batch under its hashed weights is printed
//     Q <curve> <n> <l> <count> : <count indices> : <count weights, hex> : <count x l values, hex> : <l coefficients, hex>
// so that tests/test_kzg_cosets_batch_host.py can hold it to its big-integer model.  Prints KZG COSETS BATCH CHECK OK when nothing
// is wrong.
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
int g1_check_points_bn254(int, const void*, uint64_t, uint8_t*) { return APK_ERR_HIP; }
int g1_check_points_bls12381(int, const void*, uint64_t, uint8_t*) { return APK_ERR_HIP; }
int kzg_cosets_fold_bn254(int, int, uint32_t, const void*, const void*, const void*, const void*, void*) { return APK_ERR_HIP; }
int kzg_cosets_fold_bls12381(int, int, uint32_t, const void*, const void*, const void*, const void*, void*) { return APK_ERR_HIP; }
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
struct Shape {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    using V = typename K::V;
    using Fr = Fe<FR>;
    using Aff = Affine<FP>;
    using G2 = typename K::G2;
    static constexpr int FPB = K::FPB;

    int log_n, log_l;
    uint32_t n, l, np;
    Aff G;
    std::vector<Aff> srs, digests;
    G2 g2[2], g2_half[2];
    uint8_t g2_bytes[2][4 * FPB], g2_half_bytes[4 * FPB];
    std::vector<std::vector<Fr>> values[2];       // [polynomial][coset] -> l values
    std::vector<Aff> hs[2];
    std::vector<Fr> h_scalars[2];

    static void g2_to_bytes(const G2& q, uint8_t* out) {
        memcpy(out, &q.x, sizeof q.x);
        memcpy(out + sizeof q.x, &q.y, sizeof q.y);
    }
    Shape(int ln, int ll) : log_n(ln), log_l(ll), n(1u << ln), l(1u << ll), np(n / l) {
        G = Aff{from_hex<FP>(G1_X[CURVE_ID]), from_hex<FP>(G1_Y[CURVE_ID])};
        const Fr tau = from_u64<FR>(0x9e3779b97f4a7c15ull) * from_u64<FR>(0xc2b2ae3d27d4eb4full) + from_u64<FR>(12345);
        const Fr w = K::domain_root(log_n);
        srs.resize(l);
        Fr tp = Fr::one();
        for (uint32_t c = 0; c < l; c++, tp = tp * tau) srs[c] = V::smul(G, tp).to_affine();
        const Fr tau_l = tp;
        g2[0] = g2_half[0] = G2::generator();
        g2[1] = G2::template mul<FR>(G2::generator(), Fr::from_mont(tau_l));
        g2_half[1] = G2::template mul<FR>(G2::generator(), Fr::from_mont(Fr::pow_u64(tau, l / 2)));
        g2_to_bytes(g2[0], g2_bytes[0]);
        g2_to_bytes(g2[1], g2_bytes[1]);
        g2_to_bytes(g2_half[1], g2_half_bytes);
        for (int p = 0; p < 2; p++) {
            std::vector<Fr> f(n);
            for (uint32_t k = 0; k < n; k++) {
                const Fr x = from_u64<FR>(k + 1 + p);
                f[k] = p == 0 ? x * x * x + from_u64<FR>(7) : x * x;
            }
            const Fr ft = horner(f, tau);
            digests.push_back(V::smul(G, ft).to_affine());
            for (uint32_t i = 0; i < np; i++) {
                const Fr a = Fr::pow_u64(w, (uint64_t)i * l);
                std::vector<Fr> vals(l), rem(l, Fr::zero());
                for (uint32_t j = 0; j < l; j++) vals[j] = horner(f, Fr::pow_u64(w, (uint64_t)i + (uint64_t)np * j));
                for (uint32_t c = 0; c < l; c++)
                    for (uint32_t m = np; m-- > 0;) rem[c] = rem[c] * a + f[c + l * m];
                const Fr h = (ft - horner(rem, tau)) * Fr::inv(tau_l - a);
                values[p].push_back(vals);
                h_scalars[p].push_back(h);
                hs[p].push_back(V::smul(G, h).to_affine());
            }
        }
    }

    struct Batch {
        std::vector<uint32_t> digest_of;
        std::vector<uint64_t> index;
        std::vector<Fr> values;
        std::vector<Aff> hs;
    };
    void push(Batch& b, int p, uint32_t i) const {
        b.digest_of.push_back((uint32_t)p);
        b.index.push_back(i);
        b.values.insert(b.values.end(), values[p][i].begin(), values[p][i].end());
        b.hs.push_back(hs[p][i]);
    }
    int check(const Batch& b, uint32_t nb_digests, bool half = false) const {
        const char* why = "";
        return K::cosets_check(-1, G, half ? g2_half : g2, g2_bytes[0], half ? g2_half_bytes : g2_bytes[1], srs.data(), log_n, log_l, nb_digests,
                               digests.data(), (uint32_t)b.hs.size(), b.digest_of.data(), b.index.data(), b.values.data(), b.hs.data(), &why);
    }

    int run() const {
        int bad = 0;
        auto expect = [&](int got, int want, const char* what) {
            if (got != want) { printf("curve %d n %u l %u: %s: got %d, want %d\n", CURVE_ID, n, l, what, got, want); bad++; }
        };
        if (G.is_inf() || !K::point_ok(G)) { printf("curve %d: the generator is not a point of the group\n", CURVE_ID); return 1; }
        Batch all, both;
        for (uint32_t i = 0; i < np; i++) push(all, 0, i);
        for (uint32_t i = 0; i < np; i++) { push(both, 0, i); push(both, 1, np - 1 - i); }
        expect(check(all, 1), APK_OK, "every coset of one polynomial");
        expect(check(both, 2), APK_OK, "two polynomials interleaved");
        {   // the fold of the first batch under its own weights, printed for the model
            const uint32_t count = np;
            std::vector<Fr> lambda(count), q(l);
            K::cosets_weights(G, g2_bytes[0], g2_bytes[1], n, l, 1, digests.data(), count, all.digest_of.data(), all.index.data(), all.values.data(),
                              all.hs.data(), lambda.data());
            if (const char* why = K::cosets_scalars_ok(log_n, log_l, count, all.index.data(), lambda.data(), all.values.data())) { printf("%s\n", why); bad++; }
            expect(K::cosets_fold(-1, log_n, log_l, count, all.index.data(), lambda.data(), all.values.data(), q.data()), APK_OK, "the fold");
            printf("Q %d %u %u %u :", CURVE_ID, n, l, count);
            for (uint64_t i : all.index) printf(" %llu", (unsigned long long)i);
            printf(" :");
            for (const Fr& v : lambda) { printf(" "); print_fe(v); }
            printf(" :");
            for (const Fr& v : all.values) { printf(" "); print_fe(v); }
            printf(" :");
            for (const Fr& v : q) { printf(" "); print_fe(v); }
            printf("\n");
        }
        // a batch of one against coset_check, good and bad
        for (int changed = 0; changed < 2; changed++) {
            Batch one;
            push(one, 0, np - 1);
            if (changed) one.values[l - 1] = one.values[l - 1] + Fr::one();
            const char* why = "";
            const bool single = K::coset_check(G, g2, srs.data(), log_n, log_l, np - 1, digests[0], one.values.data(), one.hs[0], &why);
            expect(check(one, 1), single ? APK_OK : APK_ERR_VERIFY, "a batch of one against coset_check");
            expect(single ? 1 : 0, changed ? 0 : 1, "coset_check itself");
        }
        {
            Batch b = both;
            b.values[b.values.size() / 2] = b.values[b.values.size() / 2] + Fr::one();
            expect(check(b, 2), APK_ERR_VERIFY, "one changed value");
            b = both;
            b.digest_of[1] = 0;
            expect(check(b, 2), APK_ERR_VERIFY, "a row pointing at the other polynomial");
            b = all;
            b.index[np - 1] = np - 2;
            expect(check(b, 1), APK_ERR_VERIFY, "an index off by one");
            expect(check(all, 1, /*half=*/true), APK_ERR_VERIFY, "[tau^(l/2)]G2");
        }
        {   // the same row twice, H + P and H - P: equal weights would cancel the error
            Batch b;
            push(b, 0, 0);
            push(b, 0, 0);
            b.hs[0] = V::smul(G, h_scalars[0][0] + from_u64<FR>(5)).to_affine();
            b.hs[1] = V::smul(G, h_scalars[0][0] - from_u64<FR>(5)).to_affine();
            expect(check(b, 1), APK_ERR_VERIFY, "opposite errors in two copies of a row");
            b.hs[0] = b.hs[1] = hs[0][0];
            expect(check(b, 1), APK_OK, "the same row twice");
        }
        return bad ? 1 : 0;
    }
};

int main() {
    static const int SHAPES[3][2] = {{3, 1}, {3, 2}, {6, 3}};
    int rc = 0;
    for (const auto& s : SHAPES) {
        rc |= Shape<FrBN254, FpBN254, PairBN254, APK_BN254>(s[0], s[1]).run();
        rc |= Shape<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(s[0], s[1]).run();
    }
    if (rc) { printf("KZG COSETS BATCH CHECK FAILED\n"); return 1; }
    printf("KZG COSETS BATCH CHECK OK: 3 shapes per curve\n");
    return 0;
}

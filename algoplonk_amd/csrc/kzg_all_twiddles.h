// HOST-only: the twiddles of the transforms in the exponent behind apk_kzg_open_all (kernels_kzg_all.h), split once per context.
// Every butterfly of those transforms multiplies a point by a power of w_2n, the generator of the size-2n domain.  The powers are
// constants of the context, so each w_2n^j, j < n, is split here with host_msm.h's glv_split: k = k1 + k2 lambda (mod r), both
// halves below 2^HALF_BITS, and the stage kernel walks k1 and k2 together over P and phi(P) - half the doublings of the plain
// chain.  The other twiddles are read from the same table:
//   size-n transform   w^j = w_2n^(2j): the even entries
//   inverse twiddles   w_2n^(-j) = -w_2n^(n - j) (w_2n^n = -1): entry n - j with both signs flipped
// No HIP in here: tools/san/kzg_all_check.cpp runs it under ASAN + UBSAN.
#pragma once
#include <stdint.h>
#include <vector>

#include "ff.h"
#include "host_msm.h"   // U256, glv_split (glv_params.h)

namespace apk {

// |k1|, |k2| as HALF_BITS-bit magnitudes, least significant word first; neg: bit 0 = k1 is negative, bit 1 = k2 is negative
constexpr int KZG_ALL_HALF_WORDS = 5;
struct KzgAllTwiddle {
    uint32_t k1[KZG_ALL_HALF_WORDS], k2[KZG_ALL_HALF_WORDS];
    uint32_t neg, pad;
};
static_assert(sizeof(KzgAllTwiddle) == 48, "a twiddle record is twelve words");

// the generator of the size-2n domain (n = 2^log_n), Montgomery form: the context's omega is its square
template <class FRP>
inline Fe<FRP> kzg_all_root_2n(int log_n) {
    Fe<FRP> a;
    for (int i = 0; i < Fe<FRP>::N; i++) a.l[i] = FRP::root(i);
    Fe<FRP> w = Fe<FRP>::to_mont(a);
    for (int i = 0; i < FRP::ADICITY - log_n - 1; i++) w = Fe<FRP>::sqr(w);
    return w;
}

// out[j] = the split of w_2n^j for j < n.  False when a half does not fit HALF_BITS (never seen: the caller then takes the plain
// stage kernel).
template <class FRP, class FPP>
inline bool kzg_all_split_table(uint32_t n, const Fe<FRP>& w_2n, std::vector<KzgAllTwiddle>& out) {
    using Fr = Fe<FRP>;
    static_assert(Fr::N == 8, "Fr is 256 bits wide");
    static_assert(GlvParams<FPP>::HALF_BITS <= 32 * KZG_ALL_HALF_WORDS, "a half fits the record");
    out.assign(n, KzgAllTwiddle{});
    Fr cur = Fr::one();
    for (uint32_t j = 0; j < n; j++) {
        const Fr plain = Fr::from_mont(cur);
        U256 k, k1, k2;
        for (int i = 0; i < 4; i++) k.w[i] = (uint64_t)plain.l[2 * i] | (uint64_t)plain.l[2 * i + 1] << 32;
        bool n1 = false, n2 = false;
        if (!glv_split<FPP>(k, k1, n1, k2, n2)) return false;
        KzgAllTwiddle& t = out[j];
        for (int i = 0; i < KZG_ALL_HALF_WORDS; i++) {
            t.k1[i] = (uint32_t)(k1.w[i >> 1] >> (32 * (i & 1)));
            t.k2[i] = (uint32_t)(k2.w[i >> 1] >> (32 * (i & 1)));
        }
        t.neg = (n1 ? 1u : 0u) | (n2 ? 2u : 0u);
        cur = cur * w_2n;
    }
    return true;
}

}  // namespace apk

// The rules of the KZG primitives (include/apk.h apk_kzg_*), stated ONCE for the opening calls (backend_impl.h) and the two
// verification calls (verify_api.cpp): the fold challenge, the fold itself and the pairing equation.  Host only: no HIP include,
// builds with plain g++ against verify_host.h (pairing, point checks) and plonk_protocol.h (encodings).
//
// The shapes are gnark-crypto's kzg package: deriveGamma hashes "gamma", the point, the digests, the claimed values and the
// caller's data transcript; BatchVerifySinglePoint folds digests and values with the powers of that challenge and hands the
// result to Verify.  For the operands in the order PLONK uses them - digests [lin] [L] [R] [O] [S1] [S2] [Qcp_i], their claimed
// values, extra = the 32 bytes of Z(omega zeta) - the challenge is PlonkProtocol::gamma_kzg (tests/test_kzg_host.py holds it
// against the executed reference template's recorded value).
#pragma once
#include <mutex>
#include <string.h>
#include <vector>

#include "plonk_protocol.h"
#include "verify_host.h"

namespace apk {

// sha256("gamma" || point || digests... || values... || extra), reduced mod r like every other challenge; raw = the 32 bytes
template <class FRP, class FPP>
inline Fe<FRP> kzg_fold_challenge(const Fe<FRP>& point, const Affine<FPP>* digests, const Fe<FRP>* values, uint32_t count,
                                  const uint8_t* extra, size_t extra_len, uint8_t raw[32]) {
    typename PlonkProtocol<FRP, FPP>::Transcript t("gamma");
    t.scalar(point);
    for (uint32_t i = 0; i < count; i++) t.point(digests[i]);
    for (uint32_t i = 0; i < count; i++) t.scalar(values[i]);
    if (extra_len) t.bytes(extra, extra_len);
    t.done(raw);
    return fr_from_be<FRP>(raw);
}

// in-memory Montgomery limbs below the modulus?
template <class P>
inline bool kzg_fe_canonical(const Fe<P>& m) {
    const Fe<P> q = Fe<P>::modulus();
    for (int w = P::N - 1; w >= 0; w--)
        if (m.l[w] != q.l[w]) return m.l[w] < q.l[w];
    return false;
}

template <class FRP, class FPP, class PP, int CURVE_ID>
struct KzgProtocol {
    using Fr = Fe<FRP>;
    using Aff = Affine<FPP>;
    using Pt = XYZZ<FPP>;
    using G2 = G2Aff<FPP, PP>;
    using V = HostVerifier<FRP, FPP, PP, CURVE_ID>;
    static constexpr int FPB = FPP::N * 4;

    // (folded digest, folded value) = (sum gamma^i digest_i, sum gamma^i value_i)
    static void kzg_fold(const Fr& gamma, const Aff* digests, const Fr* values, uint32_t count, Aff& digest, Fr& value) {
        Pt d = Pt::inf();
        Fr v = Fr::zero(), g = Fr::one();
        for (uint32_t i = 0; i < count; i++) {
            if (i == 0) d.madd(digests[0]); else d.add(V::smul(digests[i], g));
            v = v + g * values[i];
            g = g * gamma;
        }
        digest = d.to_affine();
        value = v;
    }

    // A G1 point a caller supplies: coordinates below p, on the curve, and (BLS12-381) in the prime-order subgroup
    static bool point_ok(const Aff& p) {
        if (!kzg_fe_canonical<FPP>(p.x) || !kzg_fe_canonical<FPP>(p.y)) return false;
        return V::g1_on_curve(p) && V::g1_in_subgroup(p);
    }

    // e(digest - v G1 + z H, G2_0) e(-H, G2_1) == 1
    static bool kzg_check(const Aff& g1, const G2* g2, const Aff& digest, const Fr& z, const Fr& v, const Aff& H) {
        if (!point_ok(digest) || !point_ok(H)) return false;
        Pt A = Pt::from_affine(digest);
        Pt vg = V::smul(g1, v);
        vg.neg_inplace();
        A.add(vg);
        A.add(V::smul(H, z));
        Pt B = Pt::from_affine(H);
        B.neg_inplace();
        return pairing_check2<FPP, PP>(A.to_affine(), g2[0], B.to_affine(), g2[1]);
    }

    // The key's points: G1 a finite curve point, both G2 points finite, on the twist and of order r.  The G2 subgroup test (two
    // scalar multiplications by r on the twist) is remembered per key, by value.  Returns a message, or null when the key is good.
    static const char* key_load(const apk_kzg_vk* vk, Aff& g1, G2* g2) {
        memcpy(&g1, vk->g1, sizeof g1);
        if (g1.is_inf() || !point_ok(g1)) return "kzg key: G1 is not a point of the group";
        for (int j = 0; j < 2; j++) {
            memcpy(&g2[j].x, vk->g2[j], sizeof(g2[j].x));
            memcpy(&g2[j].y, vk->g2[j] + 2 * FPB, sizeof(g2[j].y));
            g2[j].inf = g2[j].x.is_zero() && g2[j].y.is_zero();
            if (g2[j].inf || !g2[j].on_curve()) return "kzg key: a G2 point is not a point of the twist";
        }
        std::vector<uint8_t> blob(1 + 8 * FPB);
        blob[0] = (uint8_t)CURVE_ID;
        memcpy(&blob[1], vk->g2[0], 4 * FPB);
        memcpy(&blob[1 + 4 * FPB], vk->g2[1], 4 * FPB);
        static std::mutex mu;
        static std::vector<std::vector<uint8_t>> seen;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (const auto& b : seen) if (b == blob) return nullptr;
        }
        for (int j = 0; j < 2; j++)
            if (!G2::template mul<FRP>(g2[j], Fr::modulus()).inf) return "kzg key: a G2 point is not in the prime-order subgroup";
        std::lock_guard<std::mutex> lk(mu);
        if (seen.size() >= 16) seen.erase(seen.begin());
        seen.push_back(std::move(blob));
        return nullptr;
    }
};

}  // namespace apk

// The rules that decide whether a PLONK proof verifies, each stated ONCE for the prover (backend_impl.h), the host verifier
// (verify_host.h) and the C API (apk_api.cpp): byte encodings, the Fiat-Shamir transcript, hash-to-field, PI(zeta) and the
// scalars of the linearised polynomial, which commitment each of them multiplies in [lin] (lin_coefs) and the powers of gamma'
// that fold the batched opening (fold).  Host only: no HIP include, builds with plain g++ against ec.h, ff.h and sha256.h.
//
// Everything here is pinned by the reference's verifier templates (verifier/templateLogicSigBN254.go, lines cited at each
// step; BLS12-381 twin: templateLogicSigBLS12_381.go); the formulas are written from the identity in SURVEY.md App. E.  The
// independent implementations the tests hold this file against are oracle/plonk.py and algoplonk_amd/plonk.py.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/apk.h"
#include "ec.h"
#include "sha256.h"

namespace apk {

// ---- encodings ---------------------------------------------------------------------------------------------------------
// 32 big-endian bytes (any 256-bit value) -> Fr Montgomery, reduced mod r (templateLogicSigBN254.go:137-140)
template <class FRP>
inline Fe<FRP> fr_from_be(const uint8_t* be) {
    Fe<FRP> a;
    for (int i = 0; i < 8; i++) {
        const uint8_t* p = be + 32 - 4 * (i + 1);
        a.l[i] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
    }
    return Fe<FRP>::to_mont(a);
}
template <class P>
inline void fe_to_be(const Fe<P>& m, uint8_t* be) {
    const Fe<P> c = Fe<P>::from_mont(m);
    constexpr int N = P::N;
    for (int i = 0; i < N; i++) {
        uint8_t* p = be + 4 * (N - 1 - i);
        p[0] = (uint8_t)(c.l[i] >> 24); p[1] = (uint8_t)(c.l[i] >> 16); p[2] = (uint8_t)(c.l[i] >> 8); p[3] = (uint8_t)c.l[i];
    }
}
// gnark Marshal()/RawBytes(): X||Y big-endian (helper.go:35-72).  Infinity: BLS12-381 = 0x40 then zeros (verifier/verifier.go:95-99,
// the `_fs` constants of templateLogicSigBLS12_381.go:73-84); BN254 = all zeros - the BN254 template feeds ONE constant to the
// transcript and to the AVM's ec ops (templateLogicSigBN254.go:57-61,131-132), which take only the all-zero encoding: pinned by
// executing that template (tests/golden/template_verdicts.json, circuits whose [Qk] / [Qm] are the point at infinity).
template <class FPP>
inline void g1_raw(const Affine<FPP>& p, uint8_t* out) {
    constexpr int FPB = FPP::N * 4;
    if (p.is_inf()) {
        memset(out, 0, 2 * FPB);
        if (FPB == 48) out[0] = 0x40;
        return;
    }
    fe_to_be<FPP>(p.x, out);
    fe_to_be<FPP>(p.y, out + FPB);
}

template <class FRP, class FPP>
struct PlonkProtocol {
    using Fr = Fe<FRP>;
    using Aff = Affine<FPP>;
    static constexpr int FPB = FPP::N * 4;   // bytes per Fp element

    struct Transcript {
        Sha256 h;
        explicit Transcript(const char* name) { h.update(name, strlen(name)); }
        void bytes(const uint8_t* p, size_t n) { h.update(p, n); }
        void point(const Aff& p) { uint8_t b[2 * FPB]; g1_raw(p, b); h.update(b, 2 * FPB); }
        void scalar(const Fr& s) { uint8_t b[32]; fe_to_be<FRP>(s, b); h.update(b, 32); }
        void done(uint8_t out[32]) { h.final(out); }
    };

    // gnark fr.Hash(msg, "BSB22-Plonk", 1) = expand_msg_xmd(sha256, 48 bytes) mod r over a point's raw bytes, as the verifier
    // recomputes it (templateLogicSigBN254.go:386-397)
    static Fr hash_fr(const uint8_t* raw) {
        static const uint8_t dst_prime[12] = {'B', 'S', 'B', '2', '2', '-', 'P', 'l', 'o', 'n', 'k', 0x0b};
        uint8_t b0[32], b1[32], b2[32], zeros[64] = {0}, x[32];
        const uint8_t lib[3] = {0x00, 0x30, 0x00}, one = 1, two = 2;
        Sha256 h;
        h.update(zeros, 64); h.update(raw, 2 * FPB); h.update(lib, 3); h.update(dst_prime, 12); h.final(b0);
        h.reset(); h.update(b0, 32); h.update(&one, 1); h.update(dst_prime, 12); h.final(b1);
        for (int i = 0; i < 32; i++) x[i] = b0[i] ^ b1[i];
        h.reset(); h.update(x, 32); h.update(&two, 1); h.update(dst_prime, 12); h.final(b2);
        // (int(b1) * 2^128 + int(b2[:16])) mod r
        uint8_t lo[32] = {0};
        memcpy(lo + 16, b2, 16);
        Fr t = Fr::zero();
        t.l[4] = 1;
        return fr_from_be<FRP>(b1) * Fr::to_mont(t) + fr_from_be<FRP>(lo);
    }
    static Fr hash_fr(const Aff& p) { uint8_t raw[2 * FPB]; g1_raw(p, raw); return hash_fr(raw); }

    // ---- the five challenges (templateLogicSigBN254.go:131-140,280-286) ------------------------------
    // Each writes its raw 32 bytes - the next challenge hashes them - and returns the reduced Fr.
    struct KeyPoints { Aff ql, qr, qm, qo, qk, s1, s2, s3, qcp[APK_MAX_COMMITMENTS]; uint32_t k; };   // k = number of [Qcp]
    // evaluations at zeta of L, R, O, S1, S2, Qcp_i and of Z at omega zeta: the proof's claimed values 1.. and its zshift_value
    struct Evals { Fr l, r, o, s1, s2, qcp[APK_MAX_COMMITMENTS], zw; };

    static Fr gamma(const KeyPoints& key, const Fr* pub, uint32_t nb_public, const Aff& L, const Aff& R, const Aff& O, uint8_t raw[32]) {
        Transcript t("gamma");
        t.point(key.s1); t.point(key.s2); t.point(key.s3);
        t.point(key.ql); t.point(key.qr); t.point(key.qm); t.point(key.qo); t.point(key.qk);
        for (uint32_t i = 0; i < key.k; i++) t.point(key.qcp[i]);
        for (uint32_t i = 0; i < nb_public; i++) t.scalar(pub[i]);
        t.point(L); t.point(R); t.point(O);
        t.done(raw);
        return fr_from_be<FRP>(raw);
    }
    static Fr beta(const uint8_t gamma_raw[32], uint8_t raw[32]) {
        Transcript t("beta");
        t.bytes(gamma_raw, 32);
        t.done(raw);
        return fr_from_be<FRP>(raw);
    }
    static Fr alpha(const uint8_t beta_raw[32], const Aff* bsb, uint32_t k, const Aff& Z, uint8_t raw[32]) {
        Transcript t("alpha");
        t.bytes(beta_raw, 32);
        for (uint32_t i = 0; i < k; i++) t.point(bsb[i]);
        t.point(Z);
        t.done(raw);
        return fr_from_be<FRP>(raw);
    }
    static Fr zeta(const uint8_t alpha_raw[32], const Aff* H, uint8_t raw[32]) {   // H = [H1][H2][H3]
        Transcript t("zeta");
        t.bytes(alpha_raw, 32);
        t.point(H[0]); t.point(H[1]); t.point(H[2]);
        t.done(raw);
        return fr_from_be<FRP>(raw);
    }
    // gamma' of the batched opening: a transcript of its own that starts again at the label "gamma"
    static Fr gamma_kzg(const Fr& zeta, const Aff& lin, const Aff& L, const Aff& R, const Aff& O, const KeyPoints& key, const Fr& lin_z,
                        const Evals& e, uint8_t raw[32]) {
        Transcript t("gamma");
        t.scalar(zeta);
        t.point(lin); t.point(L); t.point(R); t.point(O); t.point(key.s1); t.point(key.s2);
        for (uint32_t i = 0; i < key.k; i++) t.point(key.qcp[i]);
        t.scalar(lin_z); t.scalar(e.l); t.scalar(e.r); t.scalar(e.o); t.scalar(e.s1); t.scalar(e.s2);
        for (uint32_t i = 0; i < key.k; i++) t.scalar(e.qcp[i]);
        t.scalar(e.zw);
        t.done(raw);
        return fr_from_be<FRP>(raw);
    }

    // ---- what depends on zeta and the statement alone (templateLogicSigBN254.go:142-194,220-226) ------------------------
    //   pi   PI(zeta) = sum pub_i L_i(zeta) + sum cval_j L_{nb_public + cci_j}(zeta), cval_j = hash_fr([Bsb_j])
    //   l0   L_0(zeta);  L_i(X) = w^i (X^n - 1) / (n (X - w^i)), one shared inversion for every row
    //   h    the scalars of [H1][H2][H3] in [lin]: -(zeta^n - 1) * zeta^((n+2) j)
    //   ok   false when zeta lies on the domain (probability ~ n / r): the values are then meaningless
    // None of it needs the proof's evaluations, so the prover works it out while the GPU evaluates.
    struct AtZeta { Fr pi, l0, h[3]; bool ok; };
    static AtZeta at_zeta(const Fr& zeta, uint64_t n, const Fr& omega, const Fr& n_inv, const Fr* pub, uint32_t nb_public, const Fr* cval,
                          const uint32_t* cci, uint32_t k) {
        AtZeta z;
        const Fr zh = Fr::pow_u64(zeta, n) - Fr::one();   // zeta^n - 1
        const Fr zn2 = (zh + Fr::one()) * zeta * zeta;      // zeta^(n+2)
        z.h[0] = Fr::neg(zh); z.h[1] = z.h[0] * zn2; z.h[2] = z.h[1] * zn2;
        // rows 0 .. nb_public-1 (row 0 also without public inputs: L_0), then nb_public + cci_j
        const uint32_t first = nb_public ? nb_public : 1, m = first + k;
        std::vector<Fr> w(m), pref(m + 1);
        pref[0] = Fr::one();
        for (uint32_t i = 0; i < m; i++) {
            w[i] = i == 0 ? Fr::one() : i < first ? w[i - 1] * omega : Fr::pow_u64(omega, (uint64_t)nb_public + cci[i - first]);
            pref[i + 1] = pref[i] * (zeta - w[i]);
        }
        z.ok = !pref[m].is_zero();
        Fr inv = Fr::inv(pref[m]);
        const Fr scale = zh * n_inv;
        z.pi = Fr::zero();
        z.l0 = Fr::zero();
        for (uint32_t i = m; i-- > 0;) {
            const Fr li = w[i] * scale * inv * pref[i];      // = L_row(zeta)
            inv = inv * (zeta - w[i]);
            if (i >= first) z.pi = z.pi + cval[i - first] * li;
            else if (i < nb_public) z.pi = z.pi + pub[i] * li;
            if (i == 0) z.l0 = li;
        }
        return z;
    }

    // ---- the scalars of the linearisation that need the evaluations (App. E; templateLogicSigBN254.go:195-218,231-254) ---
    //   lin_z   the opening of the linearised polynomial the verifier expects - the quotient identity holds exactly for an
    //           honest prover, so this IS lin(zeta)
    //   c_s3, c_z   the scalars of [S3] and [Z] in [lin];  u = the coset shift
    struct LinScalars { Fr lin_z, c_s3, c_z; };
    static LinScalars lin_scalars(const Fr& gamma, const Fr& beta, const Fr& alpha, const Fr& zeta, const Fr& u, const AtZeta& z, const Evals& e) {
        const Fr alpha2 = alpha * alpha, a2l0 = alpha2 * z.l0;
        const Fr perm = alpha * e.zw * (e.l + beta * e.s1 + gamma) * (e.r + beta * e.s2 + gamma);
        const Fr bu = beta * u, bu2 = bu * u;
        LinScalars s;
        s.lin_z = Fr::neg(z.pi + perm * (e.o + gamma) - a2l0);
        s.c_s3 = perm * beta;
        s.c_z = a2l0 - alpha * (e.l + beta * zeta + gamma) * (e.r + bu * zeta + gamma) * (e.o + bu2 * zeta + gamma);
        return s;
    }

    // ---- [lin]: which scalar multiplies which commitment (App. E "lin(X)"; templateLogicSigBN254.go:231-254) -------------
    //   [lin] = ql [Ql] + qr [Qr] + qm [Qm] + qo [Qo] + [Qk] + s3 [S3] + z [Z] + sum h_j [H_j+1] + sum bsb_i [Bsb_i]
    // [Qk] enters with coefficient one: it has no field here.  The fields are named, not ordered: the prover (its device
    // combination and its host partition) and the verifier (the batch kernels' term order) each keep an order of their own.
    struct LinCoefs { Fr ql, qr, qm, qo, s3, z, h[3], bsb[APK_MAX_COMMITMENTS]; };
    static LinCoefs lin_coefs(const Evals& e, const AtZeta& at, const LinScalars& s, uint32_t k) {
        LinCoefs c{};
        c.ql = e.l; c.qr = e.r; c.qm = e.l * e.r; c.qo = e.o;
        c.s3 = s.c_s3; c.z = s.c_z;
        for (int j = 0; j < 3; j++) c.h[j] = at.h[j];
        for (uint32_t i = 0; i < k; i++) c.bsb[i] = e.qcp[i];
        return c;
    }

    // ---- the fold of the batched opening at zeta (templateLogicSigBN254.go:287-321) --------------------------------------
    //   gpow[i] = gk^(i+1) for L, R, O, S1, S2, Qcp_0 ..: the scalar of that polynomial (prover) or commitment (verifier) beside lin
    //   returns the folded claim  lin_z + sum gpow[i] * value_i  - the verifier's; the prover needs only the powers
    static Fr fold(const Fr& gk, const Fr& lin_z, const Evals& e, uint32_t k, Fr gpow[5 + APK_MAX_COMMITMENTS]) {
        const Fr vals[5] = {e.l, e.r, e.o, e.s1, e.s2};
        Fr c = lin_z, g = gk;
        for (uint32_t i = 0; i < 5 + k; i++) {
            gpow[i] = g;
            c = c + g * (i < 5 ? vals[i] : e.qcp[i - 5]);
            g = g * gk;
        }
        return c;
    }
};

}  // namespace apk

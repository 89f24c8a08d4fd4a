// HOST-side PLONK verifier: the library's mirror of gnark's `plonk.Verify(proof, vk, publicWitness)`, which the reference
// runs right after the prover inside `(*CompiledCircuit).Verify` (/root/reference/algoplonk.go:93) - so that the host-side
// mirror of that API never hands out a `VerifiedProof` it has not verified.  No GPU work: ~25 G1 scalar multiplications and
// one two-pair pairing check, all on the calling thread.
//
// What it checks is pinned by the reference's own verifier templates (the same statement gnark's Verify checks):
//   transcript gamma, beta, alpha, zeta            verifier/templateLogicSigBN254.go:131-140
//   PI(zeta) incl. the BSB22 hash_fr terms         :142-194
//   linearised polynomial: opening + commitment    :195-278
//   gamma', folded commitment / evaluation         :280-321
//   batching of the two openings, pairing check    :322-356      (BLS12-381 twin: templateLogicSigBLS12_381.go)
// The formulas are written from the identity in SURVEY.md App. E.  The oracle (oracle/plonk.py::verify, a transcription of
// the template) is an independent implementation; tests/test_verify_host.py holds the two against each other.
//
// Pairing: plain ate pairing a(Q, P) = f_{T,Q}(P)^((p^12-1)/r), T = |t - 1|, on the tower Fp2 = Fp[u]/(u^2+1),
// Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v); affine Miller loop on the twist, no Frobenius maps; the final
// exponentiation is (p^6 - 1) by conjugate/inverse, then the plain power (p^6+1)/r.  Any non-degenerate bilinear pairing
// decides e(A, G2_0) e(B, G2_1) = 1; constants from tools/gen_pairing_params.py (checked numerically there).
#pragma once
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <string.h>
#include <vector>

#include "ec.h"
#include "pairing_params.h"
#include "plonk_protocol.h"
#include "sha256.h"

namespace apk {

template <class FP, class PP>
struct Fp2 {
    using F = Fe<FP>;
    F c0, c1;
    static Fp2 zero() { return {F::zero(), F::zero()}; }
    static Fp2 one() { return {F::one(), F::zero()}; }
    static Fp2 from_fp(const F& a) { return {a, F::zero()}; }
    bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    bool operator==(const Fp2& o) const { return c0 == o.c0 && c1 == o.c1; }
    static Fp2 add(const Fp2& a, const Fp2& b) { return {F::add(a.c0, b.c0), F::add(a.c1, b.c1)}; }
    static Fp2 sub(const Fp2& a, const Fp2& b) { return {F::sub(a.c0, b.c0), F::sub(a.c1, b.c1)}; }
    static Fp2 neg(const Fp2& a) { return {F::neg(a.c0), F::neg(a.c1)}; }
    static Fp2 dbl(const Fp2& a) { return add(a, a); }
    static Fp2 mul(const Fp2& a, const Fp2& b) {
        const F t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
        const F s = F::add(a.c0, a.c1) * F::add(b.c0, b.c1);
        return {F::sub(t0, t1), F::sub(F::sub(s, t0), t1)};
    }
    static Fp2 sqr(const Fp2& a) { return mul(a, a); }
    static Fp2 mul_fp(const Fp2& a, const F& k) { return {a.c0 * k, a.c1 * k}; }
    static Fp2 inv(const Fp2& a) {
        const F n = F::inv(F::add(F::sqr(a.c0), F::sqr(a.c1)));
        return {a.c0 * n, F::neg(a.c1 * n)};
    }
    // a * xi, xi = XI0 + u
    static Fp2 mul_xi(const Fp2& a) {
        F x0a0 = F::zero(), x0a1 = F::zero();
        for (uint32_t i = 0; i < PP::XI0; i++) { x0a0 = F::add(x0a0, a.c0); x0a1 = F::add(x0a1, a.c1); }
        return {F::sub(x0a0, a.c1), F::add(x0a1, a.c0)};
    }
};

template <class FP, class PP>
struct Fp6 {
    using F2 = Fp2<FP, PP>;
    F2 c0, c1, c2;
    static Fp6 zero() { return {F2::zero(), F2::zero(), F2::zero()}; }
    static Fp6 one() { return {F2::one(), F2::zero(), F2::zero()}; }
    static Fp6 add(const Fp6& a, const Fp6& b) { return {F2::add(a.c0, b.c0), F2::add(a.c1, b.c1), F2::add(a.c2, b.c2)}; }
    static Fp6 sub(const Fp6& a, const Fp6& b) { return {F2::sub(a.c0, b.c0), F2::sub(a.c1, b.c1), F2::sub(a.c2, b.c2)}; }
    static Fp6 neg(const Fp6& a) { return {F2::neg(a.c0), F2::neg(a.c1), F2::neg(a.c2)}; }
    static Fp6 mul(const Fp6& a, const Fp6& b) {
        const F2 t0 = F2::mul(a.c0, b.c0), t1 = F2::mul(a.c1, b.c1), t2 = F2::mul(a.c2, b.c2);
        const F2 m12 = F2::sub(F2::sub(F2::mul(F2::add(a.c1, a.c2), F2::add(b.c1, b.c2)), t1), t2);
        const F2 m01 = F2::sub(F2::sub(F2::mul(F2::add(a.c0, a.c1), F2::add(b.c0, b.c1)), t0), t1);
        const F2 m02 = F2::sub(F2::sub(F2::mul(F2::add(a.c0, a.c2), F2::add(b.c0, b.c2)), t0), t2);
        return {F2::add(t0, F2::mul_xi(m12)), F2::add(m01, F2::mul_xi(t2)), F2::add(m02, t1)};
    }
    // a * v
    static Fp6 mul_v(const Fp6& a) { return {F2::mul_xi(a.c2), a.c0, a.c1}; }
    static Fp6 inv(const Fp6& a) {
        const F2 A = F2::sub(F2::sqr(a.c0), F2::mul_xi(F2::mul(a.c1, a.c2)));
        const F2 B = F2::sub(F2::mul_xi(F2::sqr(a.c2)), F2::mul(a.c0, a.c1));
        const F2 Cc = F2::sub(F2::sqr(a.c1), F2::mul(a.c0, a.c2));
        const F2 Fd = F2::add(F2::mul(a.c0, A), F2::mul_xi(F2::add(F2::mul(a.c2, B), F2::mul(a.c1, Cc))));
        const F2 fi = F2::inv(Fd);
        return {F2::mul(A, fi), F2::mul(B, fi), F2::mul(Cc, fi)};
    }
};

template <class FP, class PP>
struct Fp12 {
    using F6 = Fp6<FP, PP>;
    using F2 = Fp2<FP, PP>;
    F6 a0, a1;
    static Fp12 one() { return {F6::one(), F6::zero()}; }
    bool is_one() const {
        return a0.c0 == F2::one() && a0.c1.is_zero() && a0.c2.is_zero() && a1.c0.is_zero() && a1.c1.is_zero() && a1.c2.is_zero();
    }
    static Fp12 mul(const Fp12& x, const Fp12& y) {
        const F6 t0 = F6::mul(x.a0, y.a0), t1 = F6::mul(x.a1, y.a1);
        const F6 c1 = F6::sub(F6::sub(F6::mul(F6::add(x.a0, x.a1), F6::add(y.a0, y.a1)), t0), t1);
        return {F6::add(t0, F6::mul_v(t1)), c1};
    }
    static Fp12 conj(const Fp12& x) { return {x.a0, F6::neg(x.a1)}; }   // x^(p^6)
    static Fp12 inv(const Fp12& x) {
        const F6 t = F6::inv(F6::sub(F6::mul(x.a0, x.a0), F6::mul_v(F6::mul(x.a1, x.a1))));
        return {F6::mul(x.a0, t), F6::neg(F6::mul(x.a1, t))};
    }
};

// affine point of the twist E'(Fp2): y^2 = x^3 + b'; gnark's in-memory G2Affine = X.A0 || X.A1 || Y.A0 || Y.A1 (Montgomery)
template <class FP, class PP>
struct G2Aff {
    using F2 = Fp2<FP, PP>;
    F2 x, y;
    bool inf;
    static F2 btwist() {
        Fe<FP> b0, b1;
        for (int i = 0; i < FP::N; i++) { b0.l[i] = PP::bt0(i); b1.l[i] = PP::bt1(i); }
        return {Fe<FP>::to_mont(b0), Fe<FP>::to_mont(b1)};
    }
    static G2Aff generator() {
        Fe<FP> a, b, c, d;
        for (int i = 0; i < FP::N; i++) { a.l[i] = PP::g2x0(i); b.l[i] = PP::g2x1(i); c.l[i] = PP::g2y0(i); d.l[i] = PP::g2y1(i); }
        return {{Fe<FP>::to_mont(a), Fe<FP>::to_mont(b)}, {Fe<FP>::to_mont(c), Fe<FP>::to_mont(d)}, false};
    }
    bool on_curve() const { return inf || F2::sqr(y) == F2::add(F2::mul(F2::sqr(x), x), btwist()); }
    // slope of the chord / tangent; *this != -o (callers guarantee it)
    static G2Aff add(const G2Aff& p, const G2Aff& q, F2* slope = nullptr) {
        if (p.inf) return q;
        if (q.inf) return p;
        F2 lam;
        if (p.x == q.x) {
            if (!(p.y == q.y) || p.y.is_zero()) return {F2::zero(), F2::zero(), true};
            const F2 xx = F2::sqr(p.x);
            lam = F2::mul(F2::add(F2::dbl(xx), xx), F2::inv(F2::dbl(p.y)));
        } else {
            lam = F2::mul(F2::sub(q.y, p.y), F2::inv(F2::sub(q.x, p.x)));
        }
        if (slope) *slope = lam;
        const F2 x3 = F2::sub(F2::sub(F2::sqr(lam), p.x), q.x);
        return {x3, F2::sub(F2::mul(lam, F2::sub(p.x, x3)), p.y), false};
    }
    template <class FR>
    static G2Aff mul(const G2Aff& p, const Fe<FR>& k_canonical) {
        G2Aff acc{F2::zero(), F2::zero(), true};
        for (int w = Fe<FR>::N - 1; w >= 0; w--)
            for (int b = 31; b >= 0; b--) {
                acc = add(acc, acc);
                if ((k_canonical.l[w] >> b) & 1u) acc = add(acc, p);
            }
        return acc;
    }
};

// f_{T,Q}(P) (vertical lines dropped: they die in the final exponentiation), multiplied into `f`
template <class FP, class PP>
void miller_loop(const Affine<FP>& P, const G2Aff<FP, PP>& Q, Fp12<FP, PP>& f_acc) {
    using F = Fe<FP>;
    using F2 = Fp2<FP, PP>;
    using F12 = Fp12<FP, PP>;
    if (P.is_inf() || Q.inf) return;
    auto line = [&](const F2& lam, const G2Aff<FP, PP>& T) {
        // D-type twist (x, y) -> (x w^2, y w^3):  l(P) = yP - lam xP w + (lam xT - yT) w^3
        // M-type twist (x, y) -> (x / w^2, y / w^3), scaled by w^3 (a factor from a proper subfield):
        //                                         l(P) = (lam xT - yT) - lam xP v + yP v w            (w^2 = v, w^3 = v w)
        const F2 c = F2::sub(F2::mul(lam, T.x), T.y), m = F2::neg(F2::mul_fp(lam, P.x)), yp = F2::from_fp(P.y);
        F12 l{{F2::zero(), F2::zero(), F2::zero()}, {F2::zero(), F2::zero(), F2::zero()}};
        if (PP::TWIST_M) { l.a0.c0 = c; l.a0.c1 = m; l.a1.c1 = yp; }
        else { l.a0.c0 = yp; l.a1.c0 = m; l.a1.c1 = c; }
        return l;
    };
    F12 f = F12::one();
    G2Aff<FP, PP> T = Q;
    for (int bit = PP::ATE_BITS - 2; bit >= 0; bit--) {
        F2 lam;
        const G2Aff<FP, PP> T2 = G2Aff<FP, PP>::add(T, T, &lam);
        f = F12::mul(F12::mul(f, f), line(lam, T));
        T = T2;
        if ((PP::ate(bit >> 5) >> (bit & 31)) & 1u) {
            const G2Aff<FP, PP> TQ = G2Aff<FP, PP>::add(T, Q, &lam);
            f = F12::mul(f, line(lam, T));
            T = TQ;
        }
    }
    (void)sizeof(F);
    f_acc = F12::mul(f_acc, f);
}

template <class FP, class PP>
bool final_exp_is_one(const Fp12<FP, PP>& f) {
    using F12 = Fp12<FP, PP>;
    const F12 g = F12::mul(F12::conj(f), F12::inv(f));     // f^(p^6 - 1)
    F12 acc = F12::one();
    for (int bit = PP::FEXP_BITS - 1; bit >= 0; bit--) {   // ^((p^6 + 1) / r)
        acc = F12::mul(acc, acc);
        if ((PP::fexp(bit >> 5) >> (bit & 31)) & 1u) acc = F12::mul(acc, g);
    }
    return acc.is_one();
}

// e(a0, q0) * e(a1, q1) == 1
template <class FP, class PP>
bool pairing_check2(const Affine<FP>& a0, const G2Aff<FP, PP>& q0, const Affine<FP>& a1, const G2Aff<FP, PP>& q1) {
    Fp12<FP, PP> f = Fp12<FP, PP>::one();
    miller_loop<FP, PP>(a0, q0, f);
    miller_loop<FP, PP>(a1, q1, f);
    return final_exp_is_one<FP, PP>(f);
}

// ---- G2 encodings ------------------------------------------------------------------------------------------------------
// gnark compressed G2 (vk.bin: SURVEY.md App. A.5): X.A1 || X.A0 big-endian, flag bits in the top of byte 0 exactly as for G1
// (BN254 2 bits: 10 smaller y, 11 larger, 01 infinity; BLS12-381 3 bits: 100 / 101 / 110).  "Larger" for Fp2 is gnark's
// LexicographicallyLargest: decided on A1 unless it is zero, then on A0.
template <class FP, class PP, int CURVE_ID>
int g2_decompress(const uint8_t* in, G2Aff<FP, PP>& out) {
    using F = Fe<FP>;
    using F2 = Fp2<FP, PP>;
    constexpr int N = FP::N, NB = 4 * N;
    auto load = [&](const uint8_t* p, bool mask, F& x) {
        for (int w = 0; w < N; w++) {
            const uint8_t* q = p + NB - 4 * (w + 1);
            x.l[w] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
        }
        if (mask) x.l[N - 1] &= CURVE_ID == 0 ? 0x3fffffffu : 0x1fffffffu;
        const F m = F::modulus();
        for (int w = N - 1; w >= 0; w--)
            if (x.l[w] != m.l[w]) return x.l[w] < m.l[w];
        return false;
    };
    const uint32_t top = in[0];
    bool inf, largest;
    if (CURVE_ID == 0) { const uint32_t f = top >> 6; if (f == 0) return APK_ERR_ARG; inf = f == 1; largest = f == 3; }
    else { const uint32_t f = top >> 5; if (!(f == 4 || f == 5 || f == 6)) return APK_ERR_ARG; inf = f == 6; largest = f == 5; }
    F x1, x0;
    if (!load(in, true, x1) || !load(in + NB, false, x0)) return APK_ERR_ARG;
    if (inf) { if (!x1.is_zero() || !x0.is_zero()) return APK_ERR_ARG; out = {F2::zero(), F2::zero(), true}; return APK_OK; }
    const F2 X{F::to_mont(x0), F::to_mont(x1)};
    const F2 rhs = F2::add(F2::mul(F2::sqr(X), X), G2Aff<FP, PP>::btwist());
    // sqrt in Fp2 through the norm: y = y0 + y1 u with y0^2 = (a0 + sqrt(a0^2 + a1^2)) / 2 (or the other sign), y1 = a1 / (2 y0)
    uint32_t e[N];
    for (int w = 0; w < N; w++) e[w] = FP::sqrt_exp(w);
    auto fsqrt = [&](const F& a, F& r) { r = F::pow(a, e, N); return F::sqr(r) == a; };
    F2 Y;
    if (rhs.c1.is_zero()) {
        F r;
        if (fsqrt(rhs.c0, r)) Y = {r, F::zero()};
        else if (fsqrt(F::neg(rhs.c0), r)) Y = {F::zero(), r};      // (r u)^2 = -r^2
        else return APK_ERR_ARG;
    } else {
        F s;
        if (!fsqrt(F::add(F::sqr(rhs.c0), F::sqr(rhs.c1)), s)) return APK_ERR_ARG;
        F two = F::add(F::one(), F::one());
        const F half = F::inv(two);
        F y0;
        if (!fsqrt(F::add(rhs.c0, s) * half, y0) && !fsqrt(F::sub(rhs.c0, s) * half, y0)) return APK_ERR_ARG;
        Y = {y0, rhs.c1 * F::inv(F::add(y0, y0))};
    }
    if (!(F2::sqr(Y) == rhs)) return APK_ERR_ARG;
    auto fp_large = [&](const F& a) {
        const F c = F::from_mont(a);
        for (int w = N - 1; w >= 0; w--) { const uint32_t h = FP::half(w); if (c.l[w] != h) return c.l[w] > h; }
        return false;
    };
    const bool y_large = Y.c1.is_zero() ? fp_large(Y.c0) : fp_large(Y.c1);
    if (y_large != largest) Y = F2::neg(Y);
    out = {X, Y, false};
    return APK_OK;
}

// ---- the verifier ------------------------------------------------------------------------------------------------------
template <class FRP, class FPP, class PP, int CURVE_ID>
struct HostVerifier {
    using Fr = Fe<FRP>;
    using Fp = Fe<FPP>;
    using Aff = Affine<FPP>;
    using Pt = XYZZ<FPP>;
    using G2 = G2Aff<FPP, PP>;
    static constexpr int FPB = FPP::N * 4;

    // encodings, transcript, hash-to-field, challenges, PI(zeta) and the scalars of [lin]: plonk_protocol.h, shared with the prover
    using Proto = PlonkProtocol<FRP, FPP>;
    using Transcript = typename Proto::Transcript;
    static Aff load_pt(const uint8_t* slot) { Aff p; memcpy(&p, slot, sizeof p); return p; }
    static Fr load_fr(const uint8_t* slot) { Fr a; memcpy(&a, slot, sizeof a); return a; }
    static bool g1_on_curve(const Aff& p) {
        if (p.is_inf()) return true;
        Fp b = Fp::zero();
        b.l[0] = FPP::CURVE_B;
        return Fp::sqr(p.y) == Fp::sqr(p.x) * p.x + Fp::to_mont(b);
    }
    static bool fr_canonical(const Fr& m) {   // in-memory Montgomery limbs must be below r
        const Fr q = Fr::modulus();
        for (int w = Fr::N - 1; w >= 0; w--)
            if (m.l[w] != q.l[w]) return m.l[w] < q.l[w];
        return false;
    }
    static Pt smul(const Aff& p, const Fr& k_mont) {
        const Fr k = Fr::from_mont(k_mont);
        Pt acc = Pt::inf();
        bool started = false;
        for (int w = Fr::N - 1; w >= 0; w--)
            for (int b = 31; b >= 0; b--) {
                if (started) acc = Pt::dbl(acc);
                if ((k.l[w] >> b) & 1u) { acc.madd(p); started = true; }
            }
        return acc;
    }
    // [r]P == infinity.  BN254's G1 has cofactor 1; BLS12-381's has not (gnark's SetBytes rejects such points, the AVM's
    // pairing_check fails on them).
    static bool g1_in_subgroup(const Aff& p) {
        if (FPB != 48 || p.is_inf()) return true;
        Pt acc = Pt::inf();
        bool started = false;
        const Fr q = Fr::modulus();
        for (int w = Fr::N - 1; w >= 0; w--)
            for (int b = 31; b >= 0; b--) {
                if (started) acc = Pt::dbl(acc);
                if ((q.l[w] >> b) & 1u) { acc.madd(p); started = true; }
            }
        return acc.to_affine().is_inf();
    }
    static void put_fr(uint8_t* out, const Fr& v) { fe_to_be<FRP>(v, out); }
    static void put_pt(uint8_t* out, const Aff& p) {   // what the AVM's ec ops return: X || Y big-endian, all zero for infinity
        memset(out, 0, APK_G1_MAX_BYTES);
        if (!p.is_inf()) { fe_to_be<FPP>(p.x, out); fe_to_be<FPP>(p.y, out + FPB); }
    }

    // Kzg.G1 / Kzg.G2 of the key, and the once-per-key checks of every point the key holds
    static int key_check(const apk_verifying_key* vk, Aff& G1, G2* g2) {
        const uint32_t k = vk->nb_commitments;
        const Aff Ql = load_pt(vk->ql), Qr = load_pt(vk->qr), Qm = load_pt(vk->qm), Qo = load_pt(vk->qo), Qk = load_pt(vk->qk);
        const Aff S1 = load_pt(vk->s[0]), S2 = load_pt(vk->s[1]), S3 = load_pt(vk->s[2]);
        Aff Qcp[APK_MAX_COMMITMENTS];
        for (uint32_t i = 0; i < k && i < APK_MAX_COMMITMENTS; i++) Qcp[i] = load_pt(vk->qcp[i]);
        G1 = load_pt(vk->g1);
        if (!g1_on_curve(G1) || G1.is_inf()) { set_error("verifying key: Kzg.G1 is not a curve point"); return APK_ERR_ARG; }
        for (int j = 0; j < 2; j++) {
            memcpy(&g2[j].x, vk->g2[j], sizeof(g2[j].x));
            memcpy(&g2[j].y, vk->g2[j] + 2 * FPB, sizeof(g2[j].y));
            g2[j].inf = g2[j].x.is_zero() && g2[j].y.is_zero();
        }
        // The key's own points are constants of the circuit: checked ONCE per key (on the curve / the twist, in the prime-order
        // subgroups - gnark rejects such points when it decodes a key; the twists have large cofactors and the ate Miller loop is
        // a pairing only on the order-r subgroup), remembered by value.  Two G2 scalar multiplications by r per call were most of a
        // small verification's time.
        {
            std::vector<uint8_t> blob;
            auto put = [&](const void* p, size_t nb) { const uint8_t* b = (const uint8_t*)p; blob.insert(blob.end(), b, b + nb); };
            const int cid = CURVE_ID;
            put(&cid, sizeof cid);
            const Aff& G1c = G1;
            for (const Aff* p : {&Ql, &Qr, &Qm, &Qo, &Qk, &S1, &S2, &S3, &G1c}) put(p, sizeof(Aff));
            for (uint32_t i = 0; i < k; i++) put(&Qcp[i], sizeof(Aff));
            put(vk->g2[0], 4 * FPB); put(vk->g2[1], 4 * FPB);
            static std::mutex mu;
            static std::vector<std::vector<uint8_t>> seen;
            bool known = false;
            { std::lock_guard<std::mutex> lk(mu); for (const auto& b : seen) if (b == blob) { known = true; break; } }
            if (!known) {
                std::vector<Aff> kp = {Ql, Qr, Qm, Qo, Qk, S1, S2, S3, G1};
                for (uint32_t i = 0; i < k; i++) kp.push_back(Qcp[i]);
                for (const Aff& p : kp) if (!g1_on_curve(p)) { set_error("verifying key: a G1 point is not on the curve"); return APK_ERR_ARG; }
                for (const Aff& p : kp) if (!g1_in_subgroup(p)) { set_error("verifying key: a G1 point is not in the prime-order subgroup"); return APK_ERR_ARG; }
                for (int j = 0; j < 2; j++) {
                    if (g2[j].inf || !g2[j].on_curve()) { set_error("verifying key: Kzg.G2[%d] is not a point of the twist", j); return APK_ERR_ARG; }
                    if (!G2::template mul<FRP>(g2[j], Fr::modulus()).inf) { set_error("verifying key: Kzg.G2[%d] is not in the prime-order subgroup", j); return APK_ERR_ARG; }
                }
                std::lock_guard<std::mutex> lk(mu);
                if (seen.size() >= 16) seen.erase(seen.begin());
                seen.push_back(std::move(blob));
            }
        }
        return APK_OK;
    }

    static bool key_shape_ok(const apk_verifying_key* vk) {
        if (vk->n < 2 || (vk->n & (vk->n - 1)) || vk->n > (1ull << 30)) { set_error("verifying key: n must be a power of two"); return false; }
        return true;
    }

    // One proof's verification, cut into the phases apk_verify_ex and apk_verify_batch share:
    //   load_and_check   key and proof material, everything the proof supplies range / curve checked
    //   challenges       Fiat-Shamir gamma, beta, alpha, zeta
    //   lin_scalars      PI(zeta), the expected opening of the linearised polynomial, the scalars of [lin]
    //   lin_terms        [lin] as 11 + k scalar x point terms (the sum itself is the caller's: smul here, a kernel in a batch)
    //   fold_scalars     gamma' (which hashes [lin] in affine form) and the folded claim at zeta
    struct Job {
        const apk_verifying_key* vk;
        uint32_t k;
        uint64_t n;
        const Fr* pub;
        Fr omega, n_inv, u;
        typename Proto::KeyPoints key;
        Aff Bsb[APK_MAX_COMMITMENTS];
        Aff L, R, O, Z, H[3], Wz, Wzw;
        typename Proto::Evals ev;
        Fr gamma, beta, alpha, zeta;
        typename Proto::AtZeta at;
        typename Proto::LinScalars lin;
        Fr gk, c, gpow[5 + APK_MAX_COMMITMENTS];   // gamma'^(i+1) for L, R, O, S1, S2, Qcp_i
        uint8_t gk_raw[32];

        // the 9 + k points the proof supplies, in the order they are checked
        int proof_points(Aff* out) const {
            const Aff fixed[9] = {L, R, O, Z, H[0], H[1], H[2], Wz, Wzw};
            for (int i = 0; i < 9; i++) out[i] = fixed[i];
            for (uint32_t i = 0; i < k; i++) out[9 + i] = Bsb[i];
            return 9 + (int)k;
        }

    // every caller gets the same checks, unconditionally: on the curve, in the subgroup, canonical scalars
    int load_and_check(const apk_verifying_key* vk_, const apk_proof* pr, const void* public_inputs) {
        vk = vk_;
        k = vk->nb_commitments;
        if (k > APK_MAX_COMMITMENTS || pr->nb_commitments != k || pr->curve != (uint32_t)CURVE_ID) {
            set_error("proof does not match the verifying key (curve / number of commitments)");
            return APK_ERR_VERIFY;
        }
        n = vk->n;
        int log_n = 0;
        while ((1ull << log_n) < n) log_n++;
        // domain constants as gnark's fft.NewDomain derives them (= VK Generator / SizeInv / CosetShift, :57,:68)
        Fr root;
        for (int i = 0; i < Fr::N; i++) root.l[i] = FRP::root(i);
        omega = Fr::to_mont(root);
        for (int i = 0; i < FRP::ADICITY - log_n; i++) omega = Fr::sqr(omega);
        Fr nf = Fr::zero();
        nf.l[0] = (uint32_t)n;
        n_inv = Fr::inv(Fr::to_mont(nf));
        Fr sh = Fr::zero();
        sh.l[0] = FRP::COSET_SHIFT;
        u = Fr::to_mont(sh);

        // proof and key material; everything the proof supplies is range / curve checked (templateLogicSigBN254.go:110-120)
        key.ql = load_pt(vk->ql); key.qr = load_pt(vk->qr); key.qm = load_pt(vk->qm); key.qo = load_pt(vk->qo); key.qk = load_pt(vk->qk);
        key.s1 = load_pt(vk->s[0]); key.s2 = load_pt(vk->s[1]); key.s3 = load_pt(vk->s[2]);
        key.k = k;
        L = load_pt(pr->lro[0]); R = load_pt(pr->lro[1]); O = load_pt(pr->lro[2]); Z = load_pt(pr->z);
        for (int j = 0; j < 3; j++) H[j] = load_pt(pr->h[j]);
        Wz = load_pt(pr->batched_h); Wzw = load_pt(pr->zshift_h);
        std::vector<Aff> pts = {L, R, O, Z, H[0], H[1], H[2], Wz, Wzw};
        for (uint32_t i = 0; i < k; i++) { key.qcp[i] = load_pt(vk->qcp[i]); Bsb[i] = load_pt(pr->bsb22[i]); pts.push_back(Bsb[i]); }
        for (const Aff& p : pts) if (!g1_on_curve(p)) { set_error("proof point is not on the curve"); return APK_ERR_VERIFY; }
        for (const Aff& p : pts) if (!g1_in_subgroup(p)) { set_error("proof point is not in the prime-order subgroup"); return APK_ERR_VERIFY; }
        ev.l = load_fr(pr->claimed_values[1]); ev.r = load_fr(pr->claimed_values[2]); ev.o = load_fr(pr->claimed_values[3]);
        ev.s1 = load_fr(pr->claimed_values[4]); ev.s2 = load_fr(pr->claimed_values[5]); ev.zw = load_fr(pr->zshift_value);
        std::vector<Fr> vals = {ev.l, ev.r, ev.o, ev.s1, ev.s2, ev.zw};
        for (uint32_t i = 0; i < k; i++) { ev.qcp[i] = load_fr(pr->claimed_values[6 + i]); vals.push_back(ev.qcp[i]); }
        pub = reinterpret_cast<const Fr*>(public_inputs);
        for (uint32_t i = 0; i < vk->nb_public; i++) vals.push_back(pub[i]);
        for (const Fr& v : vals) if (!fr_canonical(v)) { set_error("scalar is not below the field modulus"); return APK_ERR_VERIFY; }
        return APK_OK;
    }

    void challenges(apk_verify_trace* tr) {
        uint8_t gamma_raw[32], beta_raw[32], alpha_raw[32], zeta_raw[32];
        gamma = Proto::gamma(key, pub, vk->nb_public, L, R, O, gamma_raw);
        beta = Proto::beta(gamma_raw, beta_raw);
        alpha = Proto::alpha(beta_raw, Bsb, k, Z, alpha_raw);
        zeta = Proto::zeta(alpha_raw, H, zeta_raw);
        if (tr) { put_fr(tr->gamma, gamma); put_fr(tr->beta, beta); put_fr(tr->alpha, alpha); put_fr(tr->zeta, zeta); }
    }

    int lin_scalars(apk_verify_trace* tr) {
        Fr cval[APK_MAX_COMMITMENTS];
        for (uint32_t i = 0; i < k; i++) cval[i] = Proto::hash_fr(Bsb[i]);
        at = Proto::at_zeta(zeta, n, omega, n_inv, pub, vk->nb_public, cval, vk->commitment_constraint_index, k);
        if (!at.ok) { set_error("zeta lies on the domain"); return APK_ERR_VERIFY; }   // probability ~ n / r
        lin = Proto::lin_scalars(gamma, beta, alpha, zeta, u, at, ev);
        if (tr) { put_fr(tr->pi, at.pi); put_fr(tr->lin_at_zeta, lin.lin_z); }
        return APK_OK;
    }

    // [lin] = sum of these 11 + k terms: Proto::lin_coefs says which scalar goes with which point, the order is the batch kernels'
    int lin_terms(Aff* pts, Fr* sc) const {
        const typename Proto::LinCoefs lc = Proto::lin_coefs(ev, at, lin, k);
        int m = 0;
        auto term = [&](const Aff& p, const Fr& s) { pts[m] = p; sc[m] = s; m++; };
        term(key.ql, lc.ql); term(key.qr, lc.qr); term(key.qm, lc.qm); term(key.qo, lc.qo); term(key.qk, Fr::one());
        for (uint32_t i = 0; i < k; i++) term(Bsb[i], lc.bsb[i]);
        term(key.s3, lc.s3); term(Z, lc.z);
        for (int j = 0; j < 3; j++) term(H[j], lc.h[j]);
        return m;
    }

    void fold_scalars(const Aff& lin_com, apk_verify_trace* tr) {
        // ---- gamma' and the folded opening at zeta (:280-321)
        gk = Proto::gamma_kzg(zeta, lin_com, L, R, O, key, lin.lin_z, ev, gk_raw);
        if (tr) put_fr(tr->gamma_kzg, gk);
        c = Proto::fold(gk, lin.lin_z, ev, k, gpow);
        if (tr) put_fr(tr->folded_claim, c);
    }
    };   // struct Job

    static int verify(const apk_verifying_key* vk, const apk_proof* pr, const void* public_inputs, apk_verify_trace* tr) {
        if (tr) memset(tr, 0, sizeof *tr);
        if (!key_shape_ok(vk)) return APK_ERR_ARG;
        Job J;
        int rc = J.load_and_check(vk, pr, public_inputs);
        if (rc != APK_OK) return rc;
        J.challenges(tr);
        rc = J.lin_scalars(tr);
        if (rc != APK_OK) return rc;
        const uint32_t k = J.k;
        const Aff &L = J.L, &R = J.R, &O = J.O, &Z = J.Z, &Wz = J.Wz, &Wzw = J.Wzw, &S1 = J.key.s1, &S2 = J.key.s2;
        const Fr &zeta = J.zeta, &zw_z = J.ev.zw, &omega = J.omega;

        // ---- [lin] (App. E "lin(X)")
        Aff lin_pts[11 + APK_MAX_COMMITMENTS];
        Fr lin_sc[11 + APK_MAX_COMMITMENTS];
        const int nb_lin = J.lin_terms(lin_pts, lin_sc);
        Pt lin = Pt::inf();
        for (int i = 0; i < nb_lin; i++) {
            if (lin_sc[i] == Fr::one()) lin.madd(lin_pts[i]); else lin.add(smul(lin_pts[i], lin_sc[i]));   // (Qk's scalar is 1)
        }
        const Aff lin_com = lin.to_affine();
        if (tr) put_pt(tr->lin_commitment, lin_com);

        J.fold_scalars(lin_com, tr);
        const Fr& c = J.c;
        const uint8_t* gk_raw = J.gk_raw;
        Pt F = Pt::from_affine(lin_com);
        const Aff fold_pts[5] = {L, R, O, S1, S2};
        for (int i = 0; i < 5; i++) F.add(smul(fold_pts[i], J.gpow[i]));
        for (uint32_t i = 0; i < k; i++) F.add(smul(J.key.qcp[i], J.gpow[5 + i]));
        if (tr) put_pt(tr->folded_digest, F.to_affine());

        // ---- batch the two openings with verifier-side randomness r' (any value unpredictable to the prover: a hash of
        // everything above; :322-345), then e(F - c G1 + zeta W_z + r' (Z - Zw G1 + w zeta W_zw), G2_0) e(-(W_z + r' W_zw), G2_1) = 1
        uint8_t rr_raw[32];
        {
            Transcript t("random");
            t.bytes(gk_raw, 32); t.point(F.to_affine()); t.point(Z); t.point(Wz); t.point(Wzw); t.scalar(c); t.scalar(zw_z);
            t.done(rr_raw);
        }
        const Fr rr = fr_from_be<FRP>(rr_raw);
        Aff G1;
        G2 g2[2];
        rc = key_check(vk, G1, g2);
        if (rc != APK_OK) return rc;
        Pt A = F;
        A.add(smul(Z, rr));
        Pt cg = smul(G1, c + rr * zw_z);
        cg.neg_inplace();
        A.add(cg);
        A.add(smul(Wz, zeta));
        A.add(smul(Wzw, rr * zeta * omega));
        Pt B = Pt::from_affine(Wz);
        B.add(smul(Wzw, rr));
        B.neg_inplace();
        if (!pairing_check2<FPP, PP>(A.to_affine(), g2[0], B.to_affine(), g2[1])) {
            set_error("plonk verification failed: pairing check");
            return APK_ERR_VERIFY;
        }
        return APK_OK;
    }

    // ---- segmented sums out[s] = sum_{i in [seg[s], seg[s+1])} k_i P_i: on the host here, on a device in kernels_lincomb.h ----
    // The host side of a batch is N independent pieces of work (a proof's checks and challenges, a term's scalar multiplication):
    // they are spread over the host threads a service has anyway - APK_VERIFY_THREADS, default min(16, the machine's) - instead of
    // the calling thread alone.  fn(i) runs once for every i < n; no two calls share an i.
    template <class Fn>
    static void parallel_for(uint64_t n, Fn fn) {
        static const int want = env_int("APK_VERIFY_THREADS", (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())), 1, 64);
        const uint64_t nt = std::min<uint64_t>((uint64_t)want, n);
        if (nt <= 1) { for (uint64_t i = 0; i < n; i++) fn(i); return; }
        std::atomic<uint64_t> next{0};
        auto work = [&] { for (uint64_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i); };
        std::vector<std::thread> th;
        for (uint64_t t = 1; t < nt; t++) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    static void lincomb_host(const Aff* pts, const Fr* sc, const uint64_t* seg, uint32_t nb_segments, Aff* out) {
        std::vector<Pt> prod(seg[nb_segments]);
        parallel_for(prod.size(), [&](uint64_t i) { prod[i] = smul(pts[i], sc[i]); });
        parallel_for(nb_segments, [&](uint64_t s) {
            Pt acc = Pt::inf();
            for (uint64_t i = seg[s]; i < seg[s + 1]; i++) acc.add(prod[i]);
            out[s] = acc.to_affine();
        });
    }
    static int lincomb(int device, const Aff* pts, const Fr* sc, const uint64_t* seg, uint32_t nb_segments, Aff* out) {
        if (device < 0) { lincomb_host(pts, sc, seg, nb_segments, out); return APK_OK; }
        return CURVE_ID == APK_BN254 ? g1_lincomb_segments_bn254(device, pts, sc, seg, nb_segments, out)
                                     : g1_lincomb_segments_bls12381(device, pts, sc, seg, nb_segments, out);
    }

    // ---- the batch: `count` proofs under ONE key, one pairing check when nothing is wrong (DESIGN.md "Batch verification") ----
    //   per proof, first and by itself: sizes, canonical scalars, points on the curve / in the subgroup, zeta off the domain
    //   stage 1   [lin]_j for every surviving proof: N segments of 11 + k terms (gamma'_j hashes [lin]_j in affine form)
    //   weights   D = sha256(key points, N, every proof's points, claimed values, public inputs); rho_0 = 1,
    //             rho_j = low 128 bits of sha256("apk-batch" || D || be32(j))
    //   stage 2   A = sum rho_j A_j, B = sum rho_j B_j as ONE call of two segments; e(A, G2_0) e(B, G2_1) = 1
    //   a failed fold is bisected (the stage-1 points are kept) down to the proofs that cause it
    static int verify_batch(int device, const apk_verifying_key* vk, const apk_proof* proofs, const void* const* public_inputs,
                            const uint32_t* nb_public_inputs, uint32_t count, int* status, apk_verify_batch_trace* tr) {
        if (tr) memset(tr, 0, sizeof *tr);
        if (!key_shape_ok(vk)) return APK_ERR_ARG;
        const uint32_t k = vk->nb_commitments;
        Aff G1 = Aff::inf();
        G2 g2[2];
        if (count == 0) {
            if (k <= APK_MAX_COMMITMENTS) return key_check(vk, G1, g2);
            return APK_OK;
        }
        std::vector<Job> jobs(count);
        std::vector<uint8_t> readable(count, 0), live(count, 0);
        std::vector<std::string> why(count);
        for (uint32_t j = 0; j < count; j++) {
            status[j] = APK_ERR_VERIFY;
            if (k > APK_MAX_COMMITMENTS || proofs[j].nb_commitments != k || proofs[j].curve != (uint32_t)CURVE_ID) {
                why[j] = "proof does not match the verifying key (curve / number of commitments)";
                continue;
            }
            if (nb_public_inputs[j] != vk->nb_public) {
                char buf[96];
                snprintf(buf, sizeof buf, "invalid witness size, got %u, expected %u (public)", nb_public_inputs[j], vk->nb_public);
                why[j] = buf;
                continue;
            }
            if (vk->nb_public && (!public_inputs || !public_inputs[j])) { set_error("null argument"); return APK_ERR_ARG; }
            readable[j] = 1;
        }

        // the statement digest D and the weights: fixed before anything is folded, over every proof as it was handed in
        uint8_t D[32];
        {
            Sha256 h;
            auto hp = [&](const uint8_t* slot) { uint8_t b[2 * FPB]; g1_raw(load_pt(slot), b); h.update(b, 2 * FPB); };
            auto hs = [&](const Fr& s) { uint8_t b[32]; fe_to_be<FRP>(s, b); h.update(b, 32); };
            hp(vk->ql); hp(vk->qr); hp(vk->qm); hp(vk->qo); hp(vk->qk); hp(vk->s[0]); hp(vk->s[1]); hp(vk->s[2]);
            for (uint32_t i = 0; i < k && i < APK_MAX_COMMITMENTS; i++) hp(vk->qcp[i]);
            hp(vk->g1);
            const uint8_t nbe[4] = {(uint8_t)(count >> 24), (uint8_t)(count >> 16), (uint8_t)(count >> 8), (uint8_t)count};
            h.update(nbe, 4);
            for (uint32_t j = 0; j < count; j++) {
                const uint8_t mark = readable[j];
                h.update(&mark, 1);
                if (!mark) continue;
                const apk_proof& p = proofs[j];
                hp(p.lro[0]); hp(p.lro[1]); hp(p.lro[2]); hp(p.z); hp(p.h[0]); hp(p.h[1]); hp(p.h[2]); hp(p.batched_h); hp(p.zshift_h);
                for (uint32_t i = 0; i < k; i++) hp(p.bsb22[i]);
                for (uint32_t i = 1; i < 6 + k; i++) hs(load_fr(p.claimed_values[i]));
                hs(load_fr(p.zshift_value));
                const Fr* pub = reinterpret_cast<const Fr*>(public_inputs ? public_inputs[j] : nullptr);
                for (uint32_t i = 0; i < vk->nb_public; i++) hs(pub[i]);
            }
            h.final(D);
        }
        std::vector<Fr> rho(count);
        for (uint32_t j = 0; j < count; j++) {
            if (j == 0) { rho[j] = Fr::one(); continue; }
            uint8_t d[32], lo[32] = {0};
            const uint8_t jbe[4] = {(uint8_t)(j >> 24), (uint8_t)(j >> 16), (uint8_t)(j >> 8), (uint8_t)j};
            Sha256 h;
            h.update("apk-batch", 9); h.update(D, 32); h.update(jbe, 4); h.final(d);
            memcpy(lo + 16, d + 16, 16);
            rho[j] = fr_from_be<FRP>(lo);
        }
        if (tr) {
            memcpy(tr->d, D, 32);
            for (uint32_t j = 0; j < count && j < 4; j++) put_fr(tr->rho[j], rho[j]);
        }

        // a device also checks every point itself, in one kernel over the whole batch; the host checks below stay as they are
        if (device >= 0) {
            std::vector<Aff> pts;
            std::vector<uint32_t> owner;
            for (uint32_t j = 0; j < count; j++) {
                if (!readable[j]) continue;
                const apk_proof& p = proofs[j];
                const uint8_t* slots[9] = {p.lro[0], p.lro[1], p.lro[2], p.z, p.h[0], p.h[1], p.h[2], p.batched_h, p.zshift_h};
                for (const uint8_t* s : slots) { pts.push_back(load_pt(s)); owner.push_back(j); }
                for (uint32_t i = 0; i < k; i++) { pts.push_back(load_pt(p.bsb22[i])); owner.push_back(j); }
            }
            std::vector<uint8_t> flags(pts.size(), 0);
            const int rc = CURVE_ID == APK_BN254 ? g1_check_points_bn254(device, pts.data(), pts.size(), flags.data())
                                                 : g1_check_points_bls12381(device, pts.data(), pts.size(), flags.data());
            if (rc != APK_OK) return rc;
            for (size_t i = 0; i < flags.size(); i++) {
                if (!flags[i] || !readable[owner[i]]) continue;
                readable[owner[i]] = 0;
                why[owner[i]] = (flags[i] & 1) ? "proof point is not on the curve (device check)" : "proof point is not in the prime-order subgroup (device check)";
            }
        }
        // the host's own checks of every proof, the same in every mode; one proof is one piece of work (on BLS12-381 its 9 + k
        // multiplications by r are most of a verification's host time)
        parallel_for(count, [&](uint64_t j) {
            if (!readable[j]) return;
            Job& J = jobs[j];
            if (J.load_and_check(vk, &proofs[j], public_inputs ? public_inputs[j] : nullptr) != APK_OK) { why[j] = apk_last_error(); return; }
            J.challenges(nullptr);
            if (J.lin_scalars(nullptr) != APK_OK) { why[j] = apk_last_error(); return; }
            live[j] = 1;
        });
        std::vector<uint32_t> set;
        for (uint32_t j = 0; j < count; j++) if (live[j]) set.push_back(j);
        // the key is looked at where verify() looks at it: after the proof's own checks, before any sum - a batch of one gives
        // apk_verify's code in every corner (a bad key AND a malformed proof: APK_ERR_VERIFY)
        if (!set.empty()) {
            const int rc = key_check(vk, G1, g2);
            if (rc != APK_OK) return rc;
        }

        // ---- stage 1
        std::vector<Aff> lin(count, Aff::inf());
        if (!set.empty()) {
            std::vector<Aff> P(set.size() * (11 + k)), out(set.size());
            std::vector<Fr> S(P.size());
            std::vector<uint64_t> seg(set.size() + 1, 0);
            for (size_t i = 0; i < set.size(); i++) seg[i + 1] = seg[i] + (uint64_t)jobs[set[i]].lin_terms(&P[seg[i]], &S[seg[i]]);
            const int rc = lincomb(device, P.data(), S.data(), seg.data(), (uint32_t)set.size(), out.data());
            if (rc != APK_OK) return rc;
            for (size_t i = 0; i < set.size(); i++) lin[set[i]] = out[i];
        }
        std::vector<Fr> rr(count);
        for (uint32_t j : set) {
            Job& J = jobs[j];
            if (tr && j < 4) put_pt(tr->lin_commitment[j], lin[j]);
            J.fold_scalars(lin[j], nullptr);
            // verifier-side randomness of proof j's two openings: as in verify(), but from gamma' and the proof's own bytes - no
            // point has to come back from the device between stage 1 and the fold
            uint8_t raw[32];
            Transcript t("random");
            t.scalar(J.gk); t.point(J.Z); t.point(J.Wz); t.point(J.Wzw); t.scalar(J.c); t.scalar(J.ev.zw);
            t.done(raw);
            rr[j] = fr_from_be<FRP>(raw);
        }

        // ---- stage 2 + the pairing, over any subset of the live proofs
        uint32_t folds = 0;
        auto fold = [&](const std::vector<uint32_t>& sub, bool& ok) -> int {
            std::vector<Aff> P;
            std::vector<Fr> S;
            Fr kS1 = Fr::zero(), kS2 = Fr::zero(), kG1 = Fr::zero(), kQcp[APK_MAX_COMMITMENTS];
            for (uint32_t i = 0; i < k; i++) kQcp[i] = Fr::zero();
            auto term = [&](const Aff& p, const Fr& s) { P.push_back(p); S.push_back(s); };
            for (uint32_t j : sub) {
                const Job& J = jobs[j];
                const Fr& w = rho[j];
                term(lin[j], w); term(J.L, w * J.gpow[0]); term(J.R, w * J.gpow[1]); term(J.O, w * J.gpow[2]);
                term(J.Z, w * rr[j]); term(J.Wz, w * J.zeta); term(J.Wzw, w * rr[j] * J.zeta * J.omega);
                kS1 = kS1 + w * J.gpow[3];
                kS2 = kS2 + w * J.gpow[4];
                for (uint32_t i = 0; i < k; i++) kQcp[i] = kQcp[i] + w * J.gpow[5 + i];
                kG1 = kG1 + w * (J.c + rr[j] * J.ev.zw);
            }
            const Job& J0 = jobs[sub[0]];
            term(J0.key.s1, kS1); term(J0.key.s2, kS2);
            for (uint32_t i = 0; i < k; i++) term(J0.key.qcp[i], kQcp[i]);
            term(G1, Fr::neg(kG1));
            const uint64_t nA = P.size();
            for (uint32_t j : sub) { term(jobs[j].Wz, Fr::neg(rho[j])); term(jobs[j].Wzw, Fr::neg(rho[j] * rr[j])); }
            const uint64_t seg[3] = {0, nA, P.size()};
            Aff AB[2];
            const int rc = lincomb(device, P.data(), S.data(), seg, 2, AB);
            if (rc != APK_OK) return rc;
            if (tr && folds == 0) { put_pt(tr->a, AB[0]); put_pt(tr->b, AB[1]); }
            folds++;
            ok = pairing_check2<FPP, PP>(AB[0], g2[0], AB[1], g2[1]);
            return APK_OK;
        };
        int rc = APK_OK;
        // `sub` is known to hold a rejected proof: find it / them
        auto search = [&](auto&& self, const std::vector<uint32_t>& sub) -> void {
            if (rc != APK_OK) return;
            if (sub.size() == 1) { live[sub[0]] = 0; why[sub[0]] = "plonk verification failed: pairing check"; return; }
            const std::vector<uint32_t> left(sub.begin(), sub.begin() + sub.size() / 2), right(sub.begin() + sub.size() / 2, sub.end());
            bool ok_left = true, ok_right = false;
            rc = fold(left, ok_left);
            if (rc != APK_OK) return;
            if (!ok_left) {
                self(self, left);
                if (rc != APK_OK) return;
                rc = fold(right, ok_right);
                if (rc != APK_OK) return;
            }                                    // a good left half leaves the fault in the right one: no fold needed to know
            if (!ok_right) self(self, right);
        };
        if (!set.empty()) {
            bool ok = false;
            rc = fold(set, ok);
            if (rc != APK_OK) return rc;
            if (!ok) search(search, set);
            if (rc != APK_OK) return rc;
        }
        if (tr) tr->folds = folds;
        int first_bad = -1;
        for (uint32_t j = 0; j < count; j++) {
            if (live[j]) status[j] = APK_OK;
            else if (first_bad < 0) first_bad = (int)j;
        }
        if (first_bad < 0) return APK_OK;
        set_error("batch verification: proof %d rejected: %s", first_bad, why[first_bad].c_str());
        return APK_ERR_VERIFY;
    }
};

}  // namespace apk

// The rules of the KZG primitives (include/apk.h apk_kzg_*), stated ONCE for the opening calls (backend_impl.h) and the two
// verification calls (verify_api.cpp): the fold challenge, the fold itself and the pairing equation - and, for openings at several
// points (apk_kzg_batch_verify_multi) and for many coset openings (apk_kzg_batch_verify_cosets), the weights, the fold and the one
// pairing check.  Host only: no HIP include, builds with
// plain g++ against verify_host.h (pairing, point checks) and plonk_protocol.h (encodings).
//
// The shapes are gnark-crypto's kzg package: deriveGamma hashes "gamma", the point, the digests, the claimed values and the
// caller's data transcript; BatchVerifySinglePoint folds digests and values with the powers of that challenge and hands the
// result to Verify.  For the operands in the order PLONK uses them - digests [lin] [L] [R] [O] [S1] [S2] [Qcp_i], their claimed
// values, extra = the 32 bytes of Z(omega zeta) - the challenge is PlonkProtocol::gamma_kzg (tests/test_kzg_host.py holds it
// against the executed reference template's recorded value).
#pragma once
#include <chrono>
#include <mutex>
#include <string.h>
#include <utility>
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

    // ---- kzg.BatchVerifyMultiPoints: `count` openings (digest_i, z_i, v_i, H_i), one pairing check ------------------------------
    // gnark draws the fold's weights from crypto/rand; here they are hashed from the statement, the convention apk_verify_batch
    // has for its rho_j (verify_host.h), so that a verdict can be reproduced:
    //   D        = sha256(be32(curve) || g1 || g2[0] || g2[1] || be32(count) || per opening: digest, z, v, H) - G1 points in the
    //              transcript's raw encoding, scalars canonical big-endian, the G2 points in the key's in-memory bytes
    //   lambda_0 = 1, lambda_j = the low 128 bits of sha256("apk-kzg-multi" || D || be32(j))
    //   A = sum lambda_i digest_i + sum (lambda_i z_i) H_i - (sum lambda_i v_i) G1,  B = -sum lambda_i H_i
    //   e(A, G2_0) e(B, G2_1) == 1          (count == 1: kzg_check's equation)
    static void be32(uint32_t v, uint8_t out[4]) { out[0] = (uint8_t)(v >> 24); out[1] = (uint8_t)(v >> 16); out[2] = (uint8_t)(v >> 8); out[3] = (uint8_t)v; }
    static void multi_weights(const apk_kzg_vk* vk, const Aff& g1, uint32_t count, const Aff* digests, const Fr* points, const Fr* values,
                              const Aff* hs, Fr* lambda) {
        uint8_t D[32], w[4], b[2 * FPB];
        Sha256 h;
        auto hp = [&](const Aff& p) { g1_raw(p, b); h.update(b, 2 * FPB); };
        auto hs_ = [&](const Fr& s) { fe_to_be<FRP>(s, b); h.update(b, 32); };
        be32((uint32_t)CURVE_ID, w); h.update(w, 4);
        hp(g1);
        h.update(vk->g2[0], 4 * FPB); h.update(vk->g2[1], 4 * FPB);
        be32(count, w); h.update(w, 4);
        for (uint32_t i = 0; i < count; i++) { hp(digests[i]); hs_(points[i]); hs_(values[i]); hp(hs[i]); }
        h.final(D);
        for (uint32_t j = 0; j < count; j++) {
            if (j == 0) { lambda[0] = Fr::one(); continue; }
            uint8_t d[32], lo[32] = {0};
            Sha256 hj;
            be32(j, w);
            hj.update("apk-kzg-multi", 13); hj.update(D, 32); hj.update(w, 4); hj.final(d);
            memcpy(lo + 16, d + 16, 16);
            lambda[j] = fr_from_be<FRP>(lo);
        }
    }
    // every scalar below r?  (spread over the host threads, like the points' checks below)
    static bool multi_scalars_ok(uint32_t count, const Fr* points, const Fr* values) {
        std::vector<uint8_t> ok(2 * (size_t)count, 0);
        V::parallel_for(2 * (uint64_t)count, [&](uint64_t i) { ok[i] = kzg_fe_canonical<FRP>(i < count ? points[i] : values[i - count]) ? 1 : 0; });
        for (uint8_t o : ok) if (!o) return false;
        return true;
    }
    // The scalars are canonical (multi_scalars_ok).  device -1: the fold runs on the host, else on that GPU (kernels_lincomb.h).
    // APK_OK, APK_ERR_VERIFY (*why says what was rejected) or the device's error.
    static int multi_check(int device, const apk_kzg_vk* vk, const Aff& g1, const G2* g2, uint32_t count, const Aff* digests,
                           const Fr* points, const Fr* values, const Aff* hs, const char** why) {
        std::vector<uint8_t> ok(2 * (size_t)count, 0);
        V::parallel_for(2 * (uint64_t)count, [&](uint64_t i) { ok[i] = point_ok(i < count ? digests[i] : hs[i - count]) ? 1 : 0; });
        for (size_t i = 0; i < ok.size(); i++)
            if (!ok[i]) { *why = i < count ? "kzg: a digest is not a point of the group" : "kzg: an opening proof is not a point of the group"; return APK_ERR_VERIFY; }
        std::vector<Fr> lambda(count);
        multi_weights(vk, g1, count, digests, points, values, hs, lambda.data());
        // ONE segmented sum: [0, 2 count + 1) is A, the count terms behind it are -B
        std::vector<Aff> pts(3 * (size_t)count + 1);
        std::vector<Fr> sc(pts.size());
        Fr v = Fr::zero();
        for (uint32_t i = 0; i < count; i++) {
            pts[i] = digests[i]; sc[i] = lambda[i];
            pts[count + i] = hs[i]; sc[count + i] = lambda[i] * points[i];
            pts[2 * (size_t)count + 1 + i] = hs[i]; sc[2 * (size_t)count + 1 + i] = lambda[i];
            v = v + lambda[i] * values[i];
        }
        pts[2 * (size_t)count] = g1; sc[2 * (size_t)count] = Fr::neg(v);
        const uint64_t seg[3] = {0, 2 * (uint64_t)count + 1, 3 * (uint64_t)count + 1};
        Aff out[2];
        const int rc = V::lincomb(device, pts.data(), sc.data(), seg, 2, out);
        if (rc != APK_OK) return rc;
        Pt B = Pt::from_affine(out[1]);
        B.neg_inplace();
        if (!pairing_check2<FPP, PP>(out[0], g2[0], B.to_affine(), g2[1])) { *why = "kzg: the openings do not verify"; return APK_ERR_VERIFY; }
        return APK_OK;
    }

    // ---- a coset opening (apk_kzg_verify_coset): ONE proof for the l = 2^log_l points of coset `index` of the size-2^log_n domain ---
    // The points are x_j = w^(index + n' j), j < l (n' = n / l, w the domain's generator); all satisfy x^l = a = w^(index l).
    //   H = [(f - I) / (X^l - a)],  I = f mod (X^l - a): the polynomial of degree < l with I(x_j) = values[j]
    //   e(digest - [I(tau)]G1 + a H, G2_0) e(-H, [tau^l]G2) == 1
    // which is kzg_check's equation with [tau^l]G2 in place of G2_1, the shifted digest, value 0 and point a: there is no second
    // pairing routine.  I's coefficient c = w^(-index c) IDFT_l(values)_c, the IDFT over the generator w^(n') of the size-l domain.
    static Fr domain_root(int log_n) {      // the generator of the domain of 2^log_n points, Montgomery
        Fr a;
        for (int i = 0; i < Fr::N; i++) a.l[i] = FRP::root(i);
        Fr w = Fr::to_mont(a);
        for (int i = 0; i < FRP::ADICITY - log_n; i++) w = Fr::sqr(w);
        return w;
    }
    // v: the l values in the order j = 0 .. l-1, replaced by the l coefficients of I
    static void coset_interpolate(int log_n, int log_l, uint64_t index, std::vector<Fr>& v) {
        const uint32_t l = 1u << log_l;
        const Fr g_inv = Fr::inv(domain_root(log_l));
        for (uint32_t i = 0; i < l; i++) {
            uint32_t j = 0;
            for (int b = 0; b < log_l; b++) j |= ((i >> b) & 1u) << (log_l - 1 - b);
            if (i < j) std::swap(v[i], v[j]);
        }
        for (int t = 0; t < log_l; t++) {
            const uint32_t half = 1u << t;
            const Fr wt = Fr::pow_u64(g_inv, (uint64_t)(l >> (t + 1)));
            for (uint32_t base = 0; base < l; base += 2 * half) {
                Fr tw = Fr::one();
                for (uint32_t k = 0; k < half; k++) {
                    const Fr u = v[base + k], x = v[base + k + half] * tw;
                    v[base + k] = u + x;
                    v[base + k + half] = u - x;
                    tw = tw * wt;
                }
            }
        }
        Fr lf = Fr::zero();
        lf.l[0] = l;
        const Fr step = Fr::inv(Fr::pow_u64(domain_root(log_n), index));
        Fr cur = Fr::inv(Fr::to_mont(lf));
        for (uint32_t c = 0; c < l; c++) { v[c] = v[c] * cur; cur = cur * step; }
    }
    // g2 = (G2_0, [tau^l]G2); srs: the first l canonical SRS points; values canonical.  *why says what was rejected.
    static bool coset_check(const Aff& g1, const G2* g2, const Aff* srs, int log_n, int log_l, uint64_t index, const Aff& digest,
                            const Fr* values, const Aff& H, const char** why) {
        const uint32_t l = 1u << log_l;
        *why = "kzg: the digest or the proof is not a point of the group";
        if (!point_ok(digest) || !point_ok(H)) return false;
        std::vector<Fr> coeff(values, values + l);
        coset_interpolate(log_n, log_l, index, coeff);
        const uint64_t seg[2] = {0, l};
        Aff I;
        V::lincomb(-1, srs, coeff.data(), seg, 1, &I);
        Pt shifted = Pt::from_affine(I);
        shifted.neg_inplace();
        shifted.add(Pt::from_affine(digest));
        *why = "kzg: the coset opening does not verify";
        return kzg_check(g1, g2, shifted.to_affine(), Fr::pow_u64(domain_root(log_n), index << log_l), Fr::zero(), H);
    }

    // ---- many coset openings, one pairing check (apk_kzg_batch_verify_cosets) ----------------------------------------------------
    // `count` rows (digest_of[k] < nb_digests, index[k] < n / l, l values, H_k); a row may repeat a coset or a whole (commitment,
    // coset) pair.  a_k = w^(index[k] l), s_c = [tau^c]G1:
    //   q_c  = sum_k lambda_k w^(-index[k] c) IDFT_l(values_k)_c   (c < l; coset_interpolate's IDFT, 1 / l included)     cosets_fold
    //   mu_d = sum_{k : digest_of[k] = d} lambda_k
    //   A = sum_d mu_d C_d - sum_c q_c s_c + sum_k (lambda_k a_k) H_k,   B = sum_k lambda_k H_k        ONE two-segment V::lincomb
    //   e(A, G2_0) e(-B, [tau^l]G2) == 1                                  (count == 1: coset_check's equation)
    // The weights are hashed from the statement in two levels, the bulky rows under parallel_for:
    //   r_k = sha256(be32(digest_of[k]) || be64(index[k]) || the row's l values || H_k)
    //   D   = sha256(be32(curve) || g1 || g2[0] || g2_tau_l || be64(n) || be32(l) || be32(nb_digests) || the digests || be32(count)
    //                || r_0 .. r_(count-1))                                       - the encodings are multi_weights'
    //   lambda_0 = 1, lambda_j = the low 128 bits of sha256("apk-kzg-cosets" || D || be32(j))
    static constexpr int COSETS_FOLD_LOG_TILE = 10;       // coset sizes up to 2^10 fold on the device (kernels_kzg_cosets_fold.h)
    static void be64(uint64_t v, uint8_t out[8]) { for (int i = 0; i < 8; i++) out[i] = (uint8_t)(v >> (56 - 8 * i)); }
    // g2: (G2_0, [tau^l]G2) as apk_kzg_vk.g2 holds points
    static void cosets_weights(const Aff& g1, const uint8_t* g2_0, const uint8_t* g2_tau_l, uint64_t n, uint32_t l, uint32_t nb_digests,
                               const Aff* digests, uint32_t count, const uint32_t* digest_of, const uint64_t* index, const Fr* values,
                               const Aff* hs, Fr* lambda) {
        std::vector<uint8_t> rows(32 * (size_t)count);
        V::parallel_for(count, [&](uint64_t k) {
            uint8_t w[8], b[2 * FPB];
            Sha256 h;
            be32(digest_of[k], w); h.update(w, 4);
            be64(index[k], w); h.update(w, 8);
            for (uint32_t j = 0; j < l; j++) { fe_to_be<FRP>(values[k * l + j], b); h.update(b, 32); }
            g1_raw(hs[k], b); h.update(b, 2 * FPB);
            h.final(&rows[32 * k]);
        });
        uint8_t D[32], w[8], b[2 * FPB];
        Sha256 h;
        be32((uint32_t)CURVE_ID, w); h.update(w, 4);
        g1_raw(g1, b); h.update(b, 2 * FPB);
        h.update(g2_0, 4 * FPB); h.update(g2_tau_l, 4 * FPB);
        be64(n, w); h.update(w, 8);
        be32(l, w); h.update(w, 4);
        be32(nb_digests, w); h.update(w, 4);
        for (uint32_t d = 0; d < nb_digests; d++) { g1_raw(digests[d], b); h.update(b, 2 * FPB); }
        be32(count, w); h.update(w, 4);
        h.update(rows.data(), rows.size());
        h.final(D);
        lambda[0] = Fr::one();
        V::parallel_for(count, [&](uint64_t j) {
            if (j == 0) return;
            uint8_t d[32], lo[32] = {0}, jw[4];
            Sha256 hj;
            be32((uint32_t)j, jw);
            hj.update("apk-kzg-cosets", 14); hj.update(D, 32); hj.update(jw, 4); hj.final(d);
            memcpy(lo + 16, d + 16, 16);
            lambda[j] = fr_from_be<FRP>(lo);
        });
    }
    // every index below n / l and every value and weight below r?  null, or what is wrong
    static const char* cosets_scalars_ok(int log_n, int log_l, uint32_t count, const uint64_t* index, const Fr* weights, const Fr* values) {
        const uint32_t l = 1u << log_l;
        std::vector<uint8_t> bad(count, 0);
        V::parallel_for(count, [&](uint64_t k) {
            if (index[k] >> (log_n - log_l)) { bad[k] = 1; return; }
            if (weights && !kzg_fe_canonical<FRP>(weights[k])) { bad[k] = 2; return; }
            for (uint32_t j = 0; j < l; j++)
                if (!kzg_fe_canonical<FRP>(values[k * l + j])) { bad[k] = 2; return; }
        });
        for (uint8_t b : bad)
            if (b) return b == 1 ? "kzg: a coset index is not below n / l" : "scalar is not below the field modulus";
        return nullptr;
    }
    // q (l Fr) from canonical rows and weights.  device -1: coset_interpolate per row on the host threads, then the weighted sums;
    // device >= 0: the kernels, for l <= 2^10 - above that the device is only opened and the host path runs.  Same bytes either way.
    static int cosets_fold(int device, int log_n, int log_l, uint32_t count, const uint64_t* index, const Fr* weights, const Fr* values, Fr* q) {
        const uint32_t l = 1u << log_l;
        if (device >= 0 && log_l <= COSETS_FOLD_LOG_TILE) {
            std::vector<Fr> scale(count), step(count), tw((size_t)1 << (COSETS_FOLD_LOG_TILE - 1));
            Fr lf = Fr::zero();
            lf.l[0] = l;
            const Fr l_inv = Fr::inv(Fr::to_mont(lf)), w_inv = Fr::inv(domain_root(log_n)), g_inv = Fr::inv(domain_root(COSETS_FOLD_LOG_TILE));
            tw[0] = Fr::one();
            for (size_t j = 1; j < tw.size(); j++) tw[j] = tw[j - 1] * g_inv;
            V::parallel_for(count, [&](uint64_t k) { scale[k] = weights[k] * l_inv; step[k] = Fr::pow_u64(w_inv, index[k]); });
            return CURVE_ID == APK_BN254 ? kzg_cosets_fold_bn254(device, log_l, count, values, scale.data(), step.data(), tw.data(), q)
                                         : kzg_cosets_fold_bls12381(device, log_l, count, values, scale.data(), step.data(), tw.data(), q);
        }
        if (device >= 0) {
            const int rc = CURVE_ID == APK_BN254 ? kzg_cosets_fold_bn254(device, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr)
                                                 : kzg_cosets_fold_bls12381(device, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
            if (rc != APK_OK) return rc;
        }
        std::vector<Fr> co((size_t)count << log_l);
        V::parallel_for(count, [&](uint64_t k) {
            std::vector<Fr> v(values + k * l, values + (k + 1) * l);
            coset_interpolate(log_n, log_l, index[k], v);
            memcpy(&co[k * l], v.data(), (size_t)l * sizeof(Fr));
        });
        V::parallel_for(l, [&](uint64_t c) {
            Fr acc = Fr::zero();
            for (uint32_t k = 0; k < count; k++) acc = acc + weights[k] * co[(size_t)k * l + c];
            q[c] = acc;
        });
        return APK_OK;
    }
    // The point checks of a batch: coordinates below p on the host; on the curve and in the subgroup on the host (device -1) or
    // through g1_check_points_* (device >= 0).  pts: the digests, then the proofs.
    static int cosets_points_ok(int device, const Aff* pts, uint32_t nb_digests, uint32_t count, const char** why) {
        const size_t total = (size_t)nb_digests + count;
        std::vector<uint8_t> flags(total, 0), bad(total, 0);
        if (device >= 0) {
            const int rc = CURVE_ID == APK_BN254 ? g1_check_points_bn254(device, pts, total, flags.data())
                                                 : g1_check_points_bls12381(device, pts, total, flags.data());
            if (rc != APK_OK) return rc;
            V::parallel_for(total, [&](uint64_t i) { bad[i] = flags[i] || !kzg_fe_canonical<FPP>(pts[i].x) || !kzg_fe_canonical<FPP>(pts[i].y); });
        } else {
            V::parallel_for(total, [&](uint64_t i) { bad[i] = !point_ok(pts[i]); });
        }
        for (size_t i = 0; i < total; i++)
            if (bad[i]) { *why = i < nb_digests ? "kzg: a digest is not a point of the group" : "kzg: an opening proof is not a point of the group"; return APK_ERR_VERIFY; }
        return APK_OK;
    }
    // g2 = (G2_0, [tau^l]G2), g2_bytes the same two points as the caller holds them; srs: the first l canonical SRS points; indices,
    // digest_of and scalars checked (cosets_scalars_ok).  APK_OK, APK_ERR_VERIFY (*why says what was rejected) or the device's error.
    // ms (optional, 5 doubles): the milliseconds of the point checks, the weights, the fold, the segmented sum and the pairing.
    static int cosets_check(int device, const Aff& g1, const G2* g2, const uint8_t* g2_0, const uint8_t* g2_tau_l, const Aff* srs, int log_n,
                            int log_l, uint32_t nb_digests, const Aff* digests, uint32_t count, const uint32_t* digest_of,
                            const uint64_t* index, const Fr* values, const Aff* hs, const char** why, double* ms = nullptr) {
        const uint32_t l = 1u << log_l;
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto lap = [&](int slot, std::chrono::steady_clock::time_point& t0) {
            const auto t1 = now();
            if (ms) ms[slot] = std::chrono::duration<double, std::milli>(t1 - t0).count();
            t0 = t1;
        };
        auto t0 = now();
        std::vector<Aff> pts((size_t)nb_digests + l + 2 * (size_t)count);
        for (uint32_t d = 0; d < nb_digests; d++) pts[d] = digests[d];
        for (uint32_t k = 0; k < count; k++) pts[nb_digests + k] = hs[k];
        int rc = cosets_points_ok(device, pts.data(), nb_digests, count, why);
        if (rc != APK_OK) return rc;
        lap(0, t0);
        std::vector<Fr> lambda(count), q(l);
        cosets_weights(g1, g2_0, g2_tau_l, 1ull << log_n, l, nb_digests, digests, count, digest_of, index, values, hs, lambda.data());
        lap(1, t0);
        rc = cosets_fold(device, log_n, log_l, count, index, lambda.data(), values, q.data());
        if (rc != APK_OK) return rc;
        lap(2, t0);
        // ONE segmented sum: [0, nb_digests + l + count) is A, the count terms behind it are B
        std::vector<Fr> sc(pts.size());
        const size_t o_srs = nb_digests, o_ah = o_srs + l, o_b = o_ah + count;
        for (uint32_t d = 0; d < nb_digests; d++) sc[d] = Fr::zero();
        for (uint32_t k = 0; k < count; k++) sc[digest_of[k]] = sc[digest_of[k]] + lambda[k];
        for (uint32_t c = 0; c < l; c++) { pts[o_srs + c] = srs[c]; sc[o_srs + c] = Fr::neg(q[c]); }
        const Fr w_l = Fr::pow_u64(domain_root(log_n), l);
        V::parallel_for(count, [&](uint64_t k) {
            pts[o_ah + k] = hs[k]; sc[o_ah + k] = lambda[k] * Fr::pow_u64(w_l, index[k]);
            pts[o_b + k] = hs[k]; sc[o_b + k] = lambda[k];
        });
        const uint64_t seg[3] = {0, o_b, o_b + count};
        Aff out[2];
        rc = V::lincomb(device, pts.data(), sc.data(), seg, 2, out);
        if (rc != APK_OK) return rc;
        lap(3, t0);
        Pt B = Pt::from_affine(out[1]);
        B.neg_inplace();
        const bool ok = pairing_check2<FPP, PP>(out[0], g2[0], B.to_affine(), g2[1]);
        lap(4, t0);
        if (!ok) { *why = "kzg: the coset openings do not verify"; return APK_ERR_VERIFY; }
        return APK_OK;
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

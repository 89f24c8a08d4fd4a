// Host-only compile unit of libapk (plain g++, no HIP): apk_verify*, the readers of marshalled proofs and the G2 helpers of include/apk.h.  Kept apart from
// apk_api.cpp because the Fp12 tower templates take minutes to optimise and change rarely.
#include <string.h>

#include "backend.h"
#include "verify_host.h"
#include "verify_keys.h"
#include "proof_codec.h"
#include "runtime_env.h"
#include "kzg_protocol.h"
#include "kzg_recover_host.h"

namespace apk {

template <class FR, class FP, class PP, int CURVE_ID>
static int g2_decompress_t(const uint8_t* in, void* out) {
    G2Aff<FP, PP> q;
    if (g2_decompress<FP, PP, CURVE_ID>(in, q) != APK_OK) { set_error("not a valid compressed G2 point"); return APK_ERR_ARG; }
    // gnark's G2Affine.SetBytes also rejects points outside the order-r subgroup (the twists have large cofactors)
    if (!q.inf && !G2Aff<FP, PP>::template mul<FR>(q, Fe<FR>::modulus()).inf) { set_error("compressed G2 point is not in the prime-order subgroup"); return APK_ERR_ARG; }
    memset(out, 0, 4 * sizeof(Fe<FP>));
    if (!q.inf) { memcpy(out, &q.x, sizeof q.x); memcpy((uint8_t*)out + sizeof q.x, &q.y, sizeof q.y); }
    return APK_OK;
}
template <class FR, class FP, class PP>
static int g2_mul_gen_t(const void* scalar, void* out) {
    Fe<FR> k;
    memcpy(&k, scalar, sizeof k);
    const G2Aff<FP, PP> q = G2Aff<FP, PP>::template mul<FR>(G2Aff<FP, PP>::generator(), Fe<FR>::from_mont(k));
    memset(out, 0, 4 * sizeof(Fe<FP>));
    if (!q.inf) { memcpy(out, &q.x, sizeof q.x); memcpy((uint8_t*)out + sizeof q.x, &q.y, sizeof q.y); }
    return APK_OK;
}

// ---- apk_kzg_verify / apk_kzg_batch_verify / apk_kzg_fold_challenge (kzg_protocol.h) ----------------------------------------------
template <class FR, class FP>
static bool kzg_load_scalars(const void* in, uint32_t count, std::vector<Fe<FR>>& out) {
    out.resize(count);
    if (count) memcpy(out.data(), in, (size_t)count * sizeof(Fe<FR>));
    for (const Fe<FR>& v : out)
        if (!kzg_fe_canonical<FR>(v)) { set_error("scalar is not below the field modulus"); return false; }
    return true;
}
template <class FR, class FP>
static void kzg_load_points(const void* in, uint32_t count, std::vector<Affine<FP>>& out) {
    out.resize(count);
    if (count) memcpy(out.data(), in, (size_t)count * sizeof(Affine<FP>));
}
template <class FR, class FP, class PP, int CURVE_ID>
static int kzg_verify_t(const apk_kzg_vk* vk, uint32_t count, const void* digests, const void* values, const void* point,
                        const uint8_t* extra, size_t extra_len, const void* h, bool batch) {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    typename K::Aff g1, H;
    typename K::G2 g2[2];
    if (const char* bad = K::key_load(vk, g1, g2)) { set_error("%s", bad); return APK_ERR_ARG; }
    std::vector<Fe<FR>> vals, z;
    std::vector<Affine<FP>> digs;
    if (!kzg_load_scalars<FR, FP>(values, count, vals) || !kzg_load_scalars<FR, FP>(point, 1, z)) return APK_ERR_ARG;
    kzg_load_points<FR, FP>(digests, count, digs);
    memcpy(&H, h, sizeof H);
    typename K::Aff digest = digs[0];
    Fe<FR> value = vals[0];
    if (batch) {
        // (the challenge hashes what the caller sent; the fold multiplies points, so they are checked first)
        for (const auto& d : digs) if (!K::point_ok(d)) { set_error("kzg: a digest is not a point of the group"); return APK_ERR_VERIFY; }
        uint8_t raw[32];
        const Fe<FR> gamma = kzg_fold_challenge<FR, FP>(z[0], digs.data(), vals.data(), count, extra, extra_len, raw);
        K::kzg_fold(gamma, digs.data(), vals.data(), count, digest, value);
    }
    if (!K::kzg_check(g1, g2, digest, z[0], value, H)) { set_error("kzg: the opening does not verify"); return APK_ERR_VERIFY; }
    return APK_OK;
}
static int kzg_verify_dispatch(const apk_kzg_vk* vk, uint32_t count, const void* digests, const void* values, const void* point,
                               const uint8_t* extra, size_t extra_len, const void* h, bool batch) {
    if (!vk || !digests || !values || !point || !h || (extra_len && !extra)) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0 || count > APK_KZG_MAX_POLYS) { set_error("kzg: %u polynomials (1..%d)", count, APK_KZG_MAX_POLYS); return APK_ERR_ARG; }
    if (vk->curve == APK_BN254) return kzg_verify_t<FrBN254, FpBN254, PairBN254, APK_BN254>(vk, count, digests, values, point, extra, extra_len, h, batch);
    if (vk->curve == APK_BLS12_381) return kzg_verify_t<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(vk, count, digests, values, point, extra, extra_len, h, batch);
    set_error("unsupported curve: %d", vk->curve);
    return APK_ERR_ARG;
}
template <class FR, class FP>
static int kzg_challenge_t(uint32_t count, const void* digests, const void* values, const void* point, const uint8_t* extra,
                           size_t extra_len, void* out) {
    std::vector<Fe<FR>> vals, z;
    std::vector<Affine<FP>> digs;
    if (!kzg_load_scalars<FR, FP>(values, count, vals) || !kzg_load_scalars<FR, FP>(point, 1, z)) return APK_ERR_ARG;
    kzg_load_points<FR, FP>(digests, count, digs);
    uint8_t raw[32];
    const Fe<FR> gamma = kzg_fold_challenge<FR, FP>(z[0], digs.data(), vals.data(), count, extra, extra_len, raw);
    memcpy(out, &gamma, sizeof gamma);
    return APK_OK;
}
// ---- apk_kzg_batch_verify_multi / apk_kzg_multi_weights: the key, the scalars (APK_ERR_ARG), then the rule of kzg_protocol.h
template <class FR, class FP, class PP, int CURVE_ID>
static int kzg_multi_t(const apk_kzg_vk* vk, int device, uint32_t count, const void* digests, const void* points, const void* values,
                       const void* hs, void* out_weights) {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    typename K::Aff g1;
    typename K::G2 g2[2];
    if (const char* bad = K::key_load(vk, g1, g2)) { set_error("%s", bad); return APK_ERR_ARG; }
    std::vector<Fe<FR>> vals((size_t)count), zs((size_t)count);
    std::vector<Affine<FP>> digs, Hs;
    memcpy(vals.data(), values, (size_t)count * sizeof(Fe<FR>));
    memcpy(zs.data(), points, (size_t)count * sizeof(Fe<FR>));
    if (!K::multi_scalars_ok(count, zs.data(), vals.data())) { set_error("scalar is not below the field modulus"); return APK_ERR_ARG; }
    kzg_load_points<FR, FP>(digests, count, digs);
    kzg_load_points<FR, FP>(hs, count, Hs);
    if (out_weights) {
        K::multi_weights(vk, g1, count, digs.data(), zs.data(), vals.data(), Hs.data(), reinterpret_cast<Fe<FR>*>(out_weights));
        return APK_OK;
    }
    const char* why = "";
    const int rc = K::multi_check(device, vk, g1, g2, count, digs.data(), zs.data(), vals.data(), Hs.data(), &why);
    if (rc == APK_ERR_VERIFY) set_error("%s", why);
    return rc;
}
static int kzg_multi_dispatch(const apk_kzg_vk* vk, int device, uint32_t count, const void* digests, const void* points, const void* values,
                              const void* hs, void* out_weights, bool weights) {
    if (!vk || !digests || !points || !values || !hs || (weights && !out_weights)) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0 || count > APK_KZG_MAX_POLYS) { set_error("kzg: %u openings (1..%d)", count, APK_KZG_MAX_POLYS); return APK_ERR_ARG; }
    if (device < -1) { set_error("device %d out of range", device); return APK_ERR_ARG; }
    if (device >= 0) runtime_checkpoint();
    if (vk->curve == APK_BN254) return kzg_multi_t<FrBN254, FpBN254, PairBN254, APK_BN254>(vk, device, count, digests, points, values, hs, out_weights);
    if (vk->curve == APK_BLS12_381) return kzg_multi_t<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(vk, device, count, digests, points, values, hs, out_weights);
    set_error("unsupported curve: %d", vk->curve);
    return APK_ERR_ARG;
}
// ---- apk_kzg_verify_coset: the key and [tau^l]G2 (as a key whose second G2 point it is), the shape, the scalars (APK_ERR_ARG), then
// the rule of kzg_protocol.h
template <class FR, class FP, class PP, int CURVE_ID>
static int kzg_coset_t(const apk_kzg_vk* vk, const void* g2_tau_l, const void* srs_g1, int log_n, int log_l, uint64_t index,
                       const void* digest, const void* values, const void* h) {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    typename K::Aff g1, D, H;
    typename K::G2 g2[2];
    if (const char* bad = K::key_load(vk, g1, g2)) { set_error("%s", bad); return APK_ERR_ARG; }
    apk_kzg_vk at_l = *vk;
    memcpy(at_l.g2[1], g2_tau_l, 4 * K::FPB);
    if (const char* bad = K::key_load(&at_l, g1, g2)) { set_error("%s", bad); return APK_ERR_ARG; }
    if (log_n > FR::ADICITY) { set_error("kzg: the field has no domain of 2^%d points", log_n); return APK_ERR_ARG; }
    const uint32_t l = 1u << log_l;
    std::vector<Fe<FR>> vals;
    std::vector<Affine<FP>> srs;
    if (!kzg_load_scalars<FR, FP>(values, l, vals)) return APK_ERR_ARG;
    kzg_load_points<FR, FP>(srs_g1, l, srs);
    for (const auto& p : srs) if (!K::point_ok(p)) { set_error("kzg: an SRS point is not a point of the group"); return APK_ERR_ARG; }
    memcpy(&D, digest, sizeof D);
    memcpy(&H, h, sizeof H);
    const char* why = "";
    if (!K::coset_check(g1, g2, srs.data(), log_n, log_l, index, D, vals.data(), H, &why)) { set_error("%s", why); return APK_ERR_VERIFY; }
    return APK_OK;
}
static int kzg_coset_dispatch(const apk_kzg_vk* vk, const void* g2_tau_l, const void* srs_g1, uint64_t n, uint32_t l, uint64_t index,
                              const void* digest, const void* values, const void* h) {
    if (!vk || !g2_tau_l || !srs_g1 || !digest || !values || !h) { set_error("null argument"); return APK_ERR_ARG; }
    if (n < 4 || (n & (n - 1)) || l < 2 || (l & (l - 1)) || l > n / 2) {
        set_error("kzg: cosets of %u points in a domain of %llu (powers of two, 2 <= l <= n/2)", l, (unsigned long long)n);
        return APK_ERR_ARG;
    }
    if (index >= n / l) { set_error("kzg: coset %llu of %llu", (unsigned long long)index, (unsigned long long)(n / l)); return APK_ERR_ARG; }
    const int log_n = __builtin_ctzll(n), log_l = __builtin_ctz(l);
    if (vk->curve == APK_BN254) return kzg_coset_t<FrBN254, FpBN254, PairBN254, APK_BN254>(vk, g2_tau_l, srs_g1, log_n, log_l, index, digest, values, h);
    if (vk->curve == APK_BLS12_381) return kzg_coset_t<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(vk, g2_tau_l, srs_g1, log_n, log_l, index, digest, values, h);
    set_error("unsupported curve: %d", vk->curve);
    return APK_ERR_ARG;
}
// ---- apk_kzg_batch_verify_cosets / apk_kzg_cosets_weights / apk_kzg_cosets_fold: every argument check (APK_ERR_ARG) before the first
// point check or device call, then the rule of kzg_protocol.h
static bool kzg_cosets_shape_ok(uint64_t n, uint32_t l, uint32_t count) {
    if (n < 4 || (n & (n - 1)) || l < 2 || (l & (l - 1)) || l > n / 2) {
        set_error("kzg: cosets of %u points in a domain of %llu (powers of two, 2 <= l <= n/2)", l, (unsigned long long)n);
        return false;
    }
    if (count == 0 || count > APK_KZG_COSETS_MAX_ROWS) { set_error("kzg: %u coset openings (1..%u)", count, (unsigned)APK_KZG_COSETS_MAX_ROWS); return false; }
    return true;
}
// the calling thread's last apk_kzg_batch_verify_cosets: key and scalar checks, point checks, weights, fold, segmented sum, pairing
static thread_local double kzg_cosets_ms[6] = {0, 0, 0, 0, 0, 0};
template <class FR, class FP, class PP, int CURVE_ID>
static int kzg_cosets_t(const apk_kzg_vk* vk, int device, const void* g2_tau_l, const void* srs_g1, int log_n, int log_l, uint32_t nb_digests,
                        const void* digests, uint32_t count, const uint32_t* digest_of, const uint64_t* indices, const void* values,
                        const void* hs, void* out_weights) {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    const auto t0 = std::chrono::steady_clock::now();
    typename K::Aff g1;
    typename K::G2 g2[2];
    if (const char* bad = K::key_load(vk, g1, g2)) { set_error("%s", bad); return APK_ERR_ARG; }
    apk_kzg_vk at_l = *vk;
    memcpy(at_l.g2[1], g2_tau_l, 4 * K::FPB);
    if (const char* bad = K::key_load(&at_l, g1, g2)) { set_error("%s", bad); return APK_ERR_ARG; }
    if (log_n > FR::ADICITY) { set_error("kzg: the field has no domain of 2^%d points", log_n); return APK_ERR_ARG; }
    for (uint32_t k = 0; k < count; k++)
        if (digest_of[k] >= nb_digests) { set_error("kzg: row %u: digest_of = %u, but there are %u digests", k, digest_of[k], nb_digests); return APK_ERR_ARG; }
    const uint32_t l = 1u << log_l;
    // (the rows are read where they lie when they are aligned for it: 32 MiB at 2^20 rows of 2 values are not copied)
    std::vector<Fe<FR>> vals_copy;
    const Fe<FR>* vals = reinterpret_cast<const Fe<FR>*>(values);
    if ((uintptr_t)values % alignof(Fe<FR>)) {
        vals_copy.resize((size_t)count * l);
        memcpy(vals_copy.data(), values, vals_copy.size() * sizeof(Fe<FR>));
        vals = vals_copy.data();
    }
    if (const char* bad = K::cosets_scalars_ok(log_n, log_l, count, indices, nullptr, vals)) { set_error("%s", bad); return APK_ERR_ARG; }
    std::vector<Affine<FP>> digs, Hs, srs;
    kzg_load_points<FR, FP>(digests, nb_digests, digs);
    kzg_load_points<FR, FP>(hs, count, Hs);
    if (out_weights) {
        std::vector<Fe<FR>> lambda(count);
        K::cosets_weights(g1, vk->g2[0], at_l.g2[1], 1ull << log_n, l, nb_digests, digs.data(), count, digest_of, indices, vals, Hs.data(), lambda.data());
        memcpy(out_weights, lambda.data(), (size_t)count * sizeof(Fe<FR>));
        return APK_OK;
    }
    kzg_load_points<FR, FP>(srs_g1, l, srs);
    {
        std::vector<uint8_t> ok(l, 0);
        K::V::parallel_for(l, [&](uint64_t c) { ok[c] = K::point_ok(srs[c]) ? 1 : 0; });
        for (uint8_t o : ok) if (!o) { set_error("kzg: an SRS point is not a point of the group"); return APK_ERR_ARG; }
    }
    kzg_cosets_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const char* why = "";
    const int rc = K::cosets_check(device, g1, g2, vk->g2[0], at_l.g2[1], srs.data(), log_n, log_l, nb_digests, digs.data(), count, digest_of,
                                   indices, vals, Hs.data(), &why, kzg_cosets_ms + 1);
    if (rc == APK_ERR_VERIFY) set_error("%s", why);
    return rc;
}
static int kzg_cosets_dispatch(const apk_kzg_vk* vk, int device, const void* g2_tau_l, const void* srs_g1, uint64_t n, uint32_t l,
                               uint32_t nb_digests, const void* digests, uint32_t count, const uint32_t* digest_of, const uint64_t* indices,
                               const void* values, const void* hs, void* out_weights, bool weights) {
    if (!vk || !g2_tau_l || (!weights && !srs_g1) || !digests || !digest_of || !indices || !values || !hs || (weights && !out_weights)) {
        set_error("null argument");
        return APK_ERR_ARG;
    }
    if (!kzg_cosets_shape_ok(n, l, count)) return APK_ERR_ARG;
    if (nb_digests == 0 || nb_digests > count) { set_error("kzg: %u digests for %u coset openings (1..count)", nb_digests, count); return APK_ERR_ARG; }
    if (device < -1) { set_error("device %d out of range", device); return APK_ERR_ARG; }
    if (device >= 0) runtime_checkpoint();
    const int log_n = __builtin_ctzll(n), log_l = __builtin_ctz(l);
    if (vk->curve == APK_BN254)
        return kzg_cosets_t<FrBN254, FpBN254, PairBN254, APK_BN254>(vk, device, g2_tau_l, srs_g1, log_n, log_l, nb_digests, digests, count, digest_of, indices, values, hs, out_weights);
    if (vk->curve == APK_BLS12_381)
        return kzg_cosets_t<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(vk, device, g2_tau_l, srs_g1, log_n, log_l, nb_digests, digests, count, digest_of, indices, values, hs, out_weights);
    set_error("unsupported curve: %d", vk->curve);
    return APK_ERR_ARG;
}
template <class FR, class FP, class PP, int CURVE_ID>
static int kzg_cosets_fold_t(int device, int log_n, int log_l, uint32_t count, const uint64_t* indices, const void* weights, const void* values,
                             void* out) {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    if (log_n > FR::ADICITY) { set_error("kzg: the field has no domain of 2^%d points", log_n); return APK_ERR_ARG; }
    const uint32_t l = 1u << log_l;
    std::vector<Fe<FR>> vals((size_t)count * l), wts(count), q(l);
    memcpy(vals.data(), values, vals.size() * sizeof(Fe<FR>));
    memcpy(wts.data(), weights, wts.size() * sizeof(Fe<FR>));
    if (const char* bad = K::cosets_scalars_ok(log_n, log_l, count, indices, wts.data(), vals.data())) { set_error("%s", bad); return APK_ERR_ARG; }
    const int rc = K::cosets_fold(device, log_n, log_l, count, indices, wts.data(), vals.data(), q.data());
    if (rc == APK_OK) memcpy(out, q.data(), q.size() * sizeof(Fe<FR>));
    return rc;
}
}  // namespace apk

using namespace apk;

extern "C" {

int apk_verify_ex(const apk_verifying_key* vk, const apk_proof* proof, const void* public_inputs, uint32_t nb_public_inputs,
                  apk_verify_trace* trace) {
    if (!vk || !proof || (vk->nb_public && !public_inputs)) { set_error("null argument"); return APK_ERR_ARG; }
    // gnark's plonk.Verify: len(publicWitness) != vk.NbPublicVariables is an error, never a truncation or an over-read
    if (nb_public_inputs != vk->nb_public) {
        set_error("invalid witness size, got %u, expected %u (public)", nb_public_inputs, vk->nb_public);
        return APK_ERR_VERIFY;
    }
    if (vk->curve == APK_BN254) return HostVerifier<FrBN254, FpBN254, PairBN254, APK_BN254>::verify(vk, proof, public_inputs, trace);
    if (vk->curve == APK_BLS12_381) return HostVerifier<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>::verify(vk, proof, public_inputs, trace);
    set_error("unsupported curve: %d", vk->curve);
    return APK_ERR_ARG;
}

int apk_verify(const apk_verifying_key* vk, const apk_proof* proof, const void* public_inputs) {
    if (!vk) { set_error("null argument"); return APK_ERR_ARG; }
    return apk_verify_ex(vk, proof, public_inputs, vk->nb_public, nullptr);
}

int apk_verify_batch(int device, const apk_verifying_key* vk, const apk_proof* proofs, const void* const* public_inputs,
                     const uint32_t* nb_public_inputs, uint32_t count, int* status, apk_verify_batch_trace* trace) {
    if (!vk || (count && (!proofs || !nb_public_inputs || !status))) { set_error("null argument"); return APK_ERR_ARG; }
    if (device < -1) { set_error("device %d out of range", device); return APK_ERR_ARG; }
    if (device >= 0) runtime_checkpoint();
    if (vk->curve == APK_BN254)
        return HostVerifier<FrBN254, FpBN254, PairBN254, APK_BN254>::verify_batch(device, vk, proofs, public_inputs, nb_public_inputs, count, status, trace);
    if (vk->curve == APK_BLS12_381)
        return HostVerifier<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>::verify_batch(device, vk, proofs, public_inputs, nb_public_inputs, count, status, trace);
    set_error("unsupported curve: %d", vk->curve);
    return APK_ERR_ARG;
}

int apk_verify_batch_keys(int device, const apk_verifying_key* keys, uint32_t nb_keys, const uint32_t* key_of, const apk_proof* proofs,
                          const void* const* public_inputs, const uint32_t* nb_public_inputs, uint32_t count, int* status,
                          apk_verify_keys_trace* trace) {
    if ((nb_keys && !keys) || (count && (!key_of || !proofs || !nb_public_inputs || !status))) { set_error("null argument"); return APK_ERR_ARG; }
    if (count && !nb_keys) { set_error("%u proofs and no key", count); return APK_ERR_ARG; }
    if (device < -1) { set_error("device %d out of range", device); return APK_ERR_ARG; }
    if (device >= 0) runtime_checkpoint();
    KeysBatch b{device, keys, nb_keys, key_of, proofs, public_inputs, nb_public_inputs, count, status, trace, nullptr};
    return b.run();
}

size_t apk_proof_blob_len(int curve, uint32_t nb_commitments) { return proof_blob_len(curve, nb_commitments); }

int apk_unmarshal_proof(int curve, const uint8_t* blob, size_t len, apk_proof* out) {
    if (!out || (len && !blob)) { set_error("null argument"); return APK_ERR_ARG; }
    CodecError err;
    const int rc = unmarshal_proof(curve, blob, len, out, &err);
    if (rc != APK_OK) set_error("%s", err.msg);
    return rc;
}

int apk_unmarshal_public_inputs(int curve, const uint8_t* blob, size_t len, void* out_fr, uint32_t cap, uint32_t* nb_public) {
    if (!nb_public || (len && !blob) || (len >= 32 && !out_fr)) { set_error("null argument"); return APK_ERR_ARG; }
    CodecError err;
    const int rc = unmarshal_public_inputs(curve, blob, len, out_fr, cap, nb_public, &err);
    if (rc != APK_OK) set_error("%s", err.msg);
    return rc;
}

int apk_verify_blob(const apk_verifying_key* vk, const uint8_t* proof, size_t proof_len, const uint8_t* public_inputs, size_t public_len,
                    apk_verify_trace* trace) {
    if (trace) memset(trace, 0, sizeof *trace);
    if (!vk || (proof_len && !proof) || (public_len && !public_inputs)) { set_error("null argument"); return APK_ERR_ARG; }
    if (!codec_fp_bytes(vk->curve)) { set_error("unsupported curve: %d", vk->curve); return APK_ERR_ARG; }
    CodecError err;
    apk_proof pr;
    int rc = unmarshal_proof(vk->curve, proof, proof_len, &pr, &err);
    if (rc != APK_OK) { set_error("%s", err.msg); return rc; }
    // (the length first: the buffer below is sized by the key, never by the blob)
    if (public_len != (size_t)vk->nb_public * 32) {
        set_error("public inputs blob: %zu bytes, the key has %u public inputs (%zu bytes)", public_len, vk->nb_public, (size_t)vk->nb_public * 32);
        return APK_ERR_VERIFY;
    }
    std::vector<uint8_t> pub((size_t)vk->nb_public * APK_FR_BYTES + 1);
    uint32_t nb = 0;
    rc = unmarshal_public_inputs(vk->curve, public_inputs, public_len, pub.data(), vk->nb_public, &nb, &err);
    if (rc != APK_OK) { set_error("%s", err.msg); return rc; }
    return apk_verify_ex(vk, &pr, pub.data(), nb, trace);     // (a k that is not the key's is rejected there, with every other size)
}

int apk_verify_blobs(int device, const apk_verifying_key* keys, uint32_t nb_keys, const uint32_t* key_of, const uint8_t* const* proofs,
                     const size_t* proof_lens, const uint8_t* const* public_inputs, const size_t* public_lens, uint32_t count, int* status,
                     apk_verify_keys_trace* trace) {
    if ((nb_keys && !keys) || (count && (!key_of || !proofs || !proof_lens || !public_inputs || !public_lens || !status))) { set_error("null argument"); return APK_ERR_ARG; }
    if (count && !nb_keys) { set_error("%u proofs and no key", count); return APK_ERR_ARG; }
    if (device < -1) { set_error("device %d out of range", device); return APK_ERR_ARG; }
    if (device >= 0) runtime_checkpoint();
    std::vector<apk_proof> prs(count);
    std::vector<std::vector<uint8_t>> pubs(count);
    std::vector<const void*> pub_ptrs(count, nullptr);
    std::vector<uint32_t> nbs(count, 0);
    std::vector<std::string> prebad(count);
    for (uint32_t j = 0; j < count; j++) {
        if (key_of[j] >= nb_keys) { set_error("proof %u: key_of = %u, but there are %u keys", j, key_of[j], nb_keys); return APK_ERR_ARG; }
        if ((proof_lens[j] && !proofs[j]) || (public_lens[j] && !public_inputs[j])) { set_error("null argument"); return APK_ERR_ARG; }
        const int curve = keys[key_of[j]].curve;
        if (!codec_fp_bytes(curve)) { set_error("key %u: unsupported curve: %d", key_of[j], curve); return APK_ERR_ARG; }
        CodecError err;
        memset(&prs[j], 0, sizeof prs[j]);
        pubs[j].resize(public_lens[j] / 32 * APK_FR_BYTES + 1);
        pub_ptrs[j] = pubs[j].data();
        if (unmarshal_proof(curve, proofs[j], proof_lens[j], &prs[j], &err) != APK_OK ||
            unmarshal_public_inputs(curve, public_inputs[j], public_lens[j], pubs[j].data(), (uint32_t)(public_lens[j] / 32), &nbs[j], &err) != APK_OK)
            prebad[j] = err.msg;
    }
    KeysBatch b{device, keys, nb_keys, key_of, prs.data(), pub_ptrs.data(), nbs.data(), count, status, trace, &prebad};
    return b.run();
}

int apk_g1_lincomb_segments(int curve, int device, const void* points, const void* scalars, const uint64_t* seg, uint32_t nb_segments,
                            void* out_points) {
    if (nb_segments == 0) return APK_OK;
    if (!seg || !out_points) { set_error("null argument"); return APK_ERR_ARG; }
    if (device < -1) { set_error("device %d out of range", device); return APK_ERR_ARG; }
    if (device >= 0) runtime_checkpoint();
    if (seg[0] != 0) { set_error("segment offsets must start at 0"); return APK_ERR_ARG; }
    for (uint32_t s = 0; s < nb_segments; s++)
        if (seg[s + 1] < seg[s]) { set_error("segment offsets must not decrease"); return APK_ERR_ARG; }
    if (seg[nb_segments] > (1ull << 26)) { set_error("too many terms"); return APK_ERR_ARG; }
    if (seg[nb_segments] && (!points || !scalars)) { set_error("null argument"); return APK_ERR_ARG; }
    if (curve == APK_BN254) {
        using V = HostVerifier<FrBN254, FpBN254, PairBN254, APK_BN254>;
        return V::lincomb(device, (const V::Aff*)points, (const V::Fr*)scalars, seg, nb_segments, (V::Aff*)out_points);
    }
    if (curve == APK_BLS12_381) {
        using V = HostVerifier<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>;
        return V::lincomb(device, (const V::Aff*)points, (const V::Fr*)scalars, seg, nb_segments, (V::Aff*)out_points);
    }
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_kzg_verify(const apk_kzg_vk* vk, const void* digest, const void* point_fr, const void* value_fr, const void* h) {
    return kzg_verify_dispatch(vk, 1, digest, value_fr, point_fr, nullptr, 0, h, /*batch=*/false);
}

int apk_kzg_verify_coset(const apk_kzg_vk* vk, const void* g2_tau_l, const void* srs_g1, uint64_t n, uint32_t coset_size, uint64_t index,
                         const void* digest, const void* values, const void* h) {
    return kzg_coset_dispatch(vk, g2_tau_l, srs_g1, n, coset_size, index, digest, values, h);
}

int apk_kzg_batch_verify_cosets(const apk_kzg_vk* vk, int device, const void* g2_tau_l, const void* srs_g1, uint64_t n, uint32_t coset_size,
                                uint32_t nb_digests, const void* digests, uint32_t count, const uint32_t* digest_of, const uint64_t* indices,
                                const void* values, const void* hs) {
    return kzg_cosets_dispatch(vk, device, g2_tau_l, srs_g1, n, coset_size, nb_digests, digests, count, digest_of, indices, values, hs, nullptr,
                               /*weights=*/false);
}

int apk_kzg_cosets_weights(const apk_kzg_vk* vk, const void* g2_tau_l, uint64_t n, uint32_t coset_size, uint32_t nb_digests, const void* digests,
                           uint32_t count, const uint32_t* digest_of, const uint64_t* indices, const void* values, const void* hs,
                           void* out_weights) {
    return kzg_cosets_dispatch(vk, -1, g2_tau_l, nullptr, n, coset_size, nb_digests, digests, count, digest_of, indices, values, hs, out_weights,
                               /*weights=*/true);
}

int apk_kzg_cosets_fold(int curve, int device, uint64_t n, uint32_t coset_size, uint32_t count, const uint64_t* indices, const void* weights,
                        const void* values, void* out_coeffs) {
    if (!indices || !weights || !values || !out_coeffs) { set_error("null argument"); return APK_ERR_ARG; }
    if (!kzg_cosets_shape_ok(n, coset_size, count)) return APK_ERR_ARG;
    if (device < -1) { set_error("device %d out of range", device); return APK_ERR_ARG; }
    if (curve != APK_BN254 && curve != APK_BLS12_381) { set_error("unsupported curve: %d", curve); return APK_ERR_ARG; }
    if (device >= 0) runtime_checkpoint();
    const int log_n = __builtin_ctzll(n), log_l = __builtin_ctz(coset_size);
    if (curve == APK_BN254) return kzg_cosets_fold_t<FrBN254, FpBN254, PairBN254, APK_BN254>(device, log_n, log_l, count, indices, weights, values, out_coeffs);
    return kzg_cosets_fold_t<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(device, log_n, log_l, count, indices, weights, values, out_coeffs);
}

// the polynomial back from a sufficient set of its cells, on the calling thread (kzg_recover_host.h): null pointers, then the
// rules of kzg_recover_plan.h in apk_kzg_recover_cosets' order
int apk_kzg_recover_cosets_host(int curve, uint64_t n, uint32_t coset_size, uint32_t count, const uint64_t* indices, const void* values,
                                uint64_t len, void* out_poly) {
    if (!indices || !values || !out_poly) { set_error("null argument"); return APK_ERR_ARG; }
    RecoverVerdict v;
    if (curve == APK_BN254) v = kzg_recover_host<FrBN254>(n, coset_size, count, indices, values, len, out_poly);
    else if (curve == APK_BLS12_381) v = kzg_recover_host<FrBLS12381>(n, coset_size, count, indices, values, len, out_poly);
    else { set_error("unsupported curve: %d", curve); return APK_ERR_ARG; }
    if (v.rc != APK_OK) set_error("%s", v.message);
    return v.rc;
}

int apk_kzg_cosets_phase_ms(double* out_ms) {
    if (!out_ms) { set_error("null argument"); return APK_ERR_ARG; }
    memcpy(out_ms, kzg_cosets_ms, sizeof kzg_cosets_ms);
    return APK_OK;
}

int apk_kzg_batch_verify(const apk_kzg_vk* vk, uint32_t count, const void* digests, const void* values, const void* point_fr,
                         const uint8_t* extra, size_t extra_len, const void* h) {
    return kzg_verify_dispatch(vk, count, digests, values, point_fr, extra, extra_len, h, /*batch=*/true);
}

int apk_kzg_fold_challenge(int curve, uint32_t count, const void* digests, const void* values, const void* point_fr,
                           const uint8_t* extra, size_t extra_len, void* out_gamma) {
    if (!digests || !values || !point_fr || !out_gamma || (extra_len && !extra)) { set_error("null argument"); return APK_ERR_ARG; }
    if (count == 0 || count > APK_KZG_MAX_POLYS) { set_error("kzg: %u polynomials (1..%d)", count, APK_KZG_MAX_POLYS); return APK_ERR_ARG; }
    if (curve == APK_BN254) return kzg_challenge_t<FrBN254, FpBN254>(count, digests, values, point_fr, extra, extra_len, out_gamma);
    if (curve == APK_BLS12_381) return kzg_challenge_t<FrBLS12381, FpBLS12381>(count, digests, values, point_fr, extra, extra_len, out_gamma);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_kzg_batch_verify_multi(const apk_kzg_vk* vk, int device, uint32_t count, const void* digests, const void* points,
                               const void* values, const void* hs) {
    return kzg_multi_dispatch(vk, device, count, digests, points, values, hs, nullptr, /*weights=*/false);
}

int apk_kzg_multi_weights(const apk_kzg_vk* vk, uint32_t count, const void* digests, const void* points, const void* values,
                          const void* hs, void* out_weights) {
    return kzg_multi_dispatch(vk, -1, count, digests, points, values, hs, out_weights, /*weights=*/true);
}

int apk_g2_decompress(int curve, const uint8_t* compressed, void* out) {
    if (!compressed || !out) { set_error("null argument"); return APK_ERR_ARG; }
    if (curve == APK_BN254) return g2_decompress_t<FrBN254, FpBN254, PairBN254, APK_BN254>(compressed, out);
    if (curve == APK_BLS12_381) return g2_decompress_t<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(compressed, out);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

int apk_g2_mul_generator(int curve, const void* scalar_fr, void* out) {
    if (!scalar_fr || !out) { set_error("null argument"); return APK_ERR_ARG; }
    if (curve == APK_BN254) return g2_mul_gen_t<FrBN254, FpBN254, PairBN254>(scalar_fr, out);
    if (curve == APK_BLS12_381) return g2_mul_gen_t<FrBLS12381, FpBLS12381, PairBLS12381>(scalar_fr, out);
    set_error("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}

}  // extern "C"

// Batch verification ACROSS circuits (include/apk.h apk_verify_batch_keys / apk_verify_blobs; DESIGN.md "Batch verification"):
// `count` proofs, each under one of `nb_keys` verifying keys.  Host only, plain g++; the sums go through HostVerifier::lincomb - the
// kernels of kernels_lincomb.h when a device is named, the host otherwise.
//
// Every pairing equation of every circuit has the form e(A_j, [1]G2) e(B_j, [tau]G2) = 1, so what decides whether two proofs can be
// folded together is the SRS, not the circuit: keys are grouped by curve and the bytes of g1, g2[0], g2[1], and a group is what
// verify_host.h's verify_batch calls a batch - one stage 1, one stage 2, one pairing check, bisected when it fails.  The phases of a
// proof (HostVerifier::Job) are the ones apk_verify_ex and apk_verify_batch run, made against the proof's own key.  What differs from
// verify_batch: stage 2 keeps one accumulator of the scalars of S1, S2, Qcp_i PER KEY, and the weights come from one digest over
// the whole call - all keys, all proofs, every rho_j hashed (apk_verify_batch's D, rho_0 = 1 and trace bytes are pinned by its own
// tests and stay as they are, which is why the two do not share their digest and fold code).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "verify_host.h"

namespace apk {

struct KeysBatch {
    int device;
    const apk_verifying_key* keys;
    uint32_t nb_keys;
    const uint32_t* key_of;
    const apk_proof* proofs;
    const void* const* public_inputs;
    const uint32_t* nb_public_inputs;
    uint32_t count;
    int* status;
    apk_verify_keys_trace* tr;
    const std::vector<std::string>* prebad;   // apk_verify_blobs: why proof j could not be read ("" = it could); may be null

    std::vector<uint8_t> readable, live;
    std::vector<std::string> why;
    std::vector<uint8_t> rho_be;              // 32 bytes per proof, canonical big-endian (below 2^128: the same value on both curves)
    std::vector<uint32_t> group_of_key;
    uint32_t folds = 0;

    static void be32(Sha256& h, uint32_t v) { const uint8_t b[4] = {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v}; h.update(b, 4); }
    static void be64(Sha256& h, uint64_t v) { be32(h, (uint32_t)(v >> 32)); be32(h, (uint32_t)v); }
    static uint32_t key_qcp(const apk_verifying_key& vk) { return vk.nb_commitments < APK_MAX_COMMITMENTS ? vk.nb_commitments : APK_MAX_COMMITMENTS; }
    const void* pub_of(uint32_t j) const { return public_inputs ? public_inputs[j] : nullptr; }

    // ---- the digest's per-key and per-proof parts, in the key's curve's encodings (layout: include/apk.h) ----
    template <class V>
    static void hash_key(Sha256& h, const apk_verifying_key& vk) {
        auto hp = [&](const uint8_t* slot) { uint8_t b[2 * V::FPB]; g1_raw(V::load_pt(slot), b); h.update(b, 2 * V::FPB); };
        const uint32_t k = key_qcp(vk);
        be32(h, (uint32_t)vk.curve);
        hp(vk.ql); hp(vk.qr); hp(vk.qm); hp(vk.qo); hp(vk.qk); hp(vk.s[0]); hp(vk.s[1]); hp(vk.s[2]);
        for (uint32_t i = 0; i < k; i++) hp(vk.qcp[i]);
        hp(vk.g1);
        be64(h, vk.n); be32(h, vk.nb_public); be32(h, vk.nb_commitments);
        for (uint32_t i = 0; i < k; i++) be32(h, vk.commitment_constraint_index[i]);
        h.update(vk.g2[0], 4 * V::FPB); h.update(vk.g2[1], 4 * V::FPB);
    }
    template <class V>
    static void hash_proof(Sha256& h, const apk_proof& p, const apk_verifying_key& vk, const void* public_inputs) {
        using Fr = typename V::Fr;
        auto hp = [&](const uint8_t* slot) { uint8_t b[2 * V::FPB]; g1_raw(V::load_pt(slot), b); h.update(b, 2 * V::FPB); };
        auto hs = [&](const uint8_t* slot) { uint8_t b[32]; V::put_fr(b, V::load_fr(slot)); h.update(b, 32); };
        const uint32_t k = vk.nb_commitments;
        hp(p.lro[0]); hp(p.lro[1]); hp(p.lro[2]); hp(p.z); hp(p.h[0]); hp(p.h[1]); hp(p.h[2]); hp(p.batched_h); hp(p.zshift_h);
        for (uint32_t i = 0; i < k; i++) hp(p.bsb22[i]);
        for (uint32_t i = 1; i < 6 + k; i++) hs(p.claimed_values[i]);
        hs(p.zshift_value);
        for (uint32_t i = 0; i < vk.nb_public; i++) hs((const uint8_t*)public_inputs + sizeof(Fr) * i);
    }

    // the additional device check of every readable proof's points, one kernel per curve over the whole call
    template <class V>
    int device_check(int curve) {
        using Aff = typename V::Aff;
        std::vector<Aff> pts;
        std::vector<uint32_t> owner;
        for (uint32_t j = 0; j < count; j++) {
            if (!readable[j] || keys[key_of[j]].curve != curve) continue;
            const apk_proof& p = proofs[j];
            const uint8_t* slots[9] = {p.lro[0], p.lro[1], p.lro[2], p.z, p.h[0], p.h[1], p.h[2], p.batched_h, p.zshift_h};
            for (const uint8_t* s : slots) { pts.push_back(V::load_pt(s)); owner.push_back(j); }
            for (uint32_t i = 0; i < p.nb_commitments; i++) { pts.push_back(V::load_pt(p.bsb22[i])); owner.push_back(j); }
        }
        if (pts.empty()) return APK_OK;
        std::vector<uint8_t> flags(pts.size(), 0);
        const int rc = curve == APK_BN254 ? g1_check_points_bn254(device, pts.data(), pts.size(), flags.data())
                                          : g1_check_points_bls12381(device, pts.data(), pts.size(), flags.data());
        if (rc != APK_OK) return rc;
        for (size_t i = 0; i < flags.size(); i++) {
            if (!flags[i] || !readable[owner[i]]) continue;
            readable[owner[i]] = 0;
            why[owner[i]] = (flags[i] & 1) ? "proof point is not on the curve (device check)" : "proof point is not in the prime-order subgroup (device check)";
        }
        return APK_OK;
    }

    // One group: the readable proofs `members` (ascending) of keys that share g1 and g2.
    template <class FRP, class FPP, class PP, int CURVE_ID>
    int run_group(const std::vector<uint32_t>& members) {
        using V = HostVerifier<FRP, FPP, PP, CURVE_ID>;
        using Fr = typename V::Fr;
        using Aff = typename V::Aff;
        using Job = typename V::Job;
        const size_t m = members.size();
        std::vector<Job> jobs(m);
        std::vector<uint8_t> ok(m, 0);
        // the host's own checks of every proof against ITS key, the same in every mode; one proof is one piece of work
        V::parallel_for(m, [&](uint64_t i) {
            const uint32_t j = members[i];
            Job& J = jobs[i];
            if (J.load_and_check(&keys[key_of[j]], &proofs[j], pub_of(j)) != APK_OK) { why[j] = apk_last_error(); return; }
            J.challenges(nullptr);
            if (J.lin_scalars(nullptr) != APK_OK) { why[j] = apk_last_error(); return; }
            ok[i] = 1;
        });
        std::vector<uint32_t> set;            // indices into members / jobs
        for (size_t i = 0; i < m; i++) if (ok[i]) set.push_back((uint32_t)i);
        if (set.empty()) return APK_OK;
        // a key is looked at where verify() looks at it: after the proofs' own checks, before any sum
        Aff G1 = Aff::inf();
        typename V::G2 g2[2];
        {
            std::vector<uint8_t> checked(nb_keys, 0);
            for (uint32_t i : set) {
                const uint32_t kk = key_of[members[i]];
                if (checked[kk]) continue;
                checked[kk] = 1;
                const int rc = V::key_check(&keys[kk], G1, g2);   // (G1, g2: the same bytes for every key of the group)
                if (rc != APK_OK) return rc;
            }
        }

        // ---- stage 1: [lin]_j, segments of 11 + k_j terms
        std::vector<Aff> lin(m, Aff::inf());
        {
            std::vector<uint64_t> seg(set.size() + 1, 0);
            for (size_t i = 0; i < set.size(); i++) seg[i + 1] = seg[i] + 11 + jobs[set[i]].k;
            std::vector<Aff> P(seg[set.size()]), out(set.size());
            std::vector<Fr> S(P.size());
            for (size_t i = 0; i < set.size(); i++) jobs[set[i]].lin_terms(&P[seg[i]], &S[seg[i]]);
            const int rc = V::lincomb(device, P.data(), S.data(), seg.data(), (uint32_t)set.size(), out.data());
            if (rc != APK_OK) return rc;
            for (size_t i = 0; i < set.size(); i++) lin[set[i]] = out[i];
        }
        std::vector<Fr> rr(m), rho(m);
        for (uint32_t i : set) {
            Job& J = jobs[i];
            const uint32_t j = members[i];
            if (tr && j < 4) V::put_pt(tr->lin_commitment[j], lin[i]);
            J.fold_scalars(lin[i], nullptr);
            uint8_t raw[32];                  // the randomness of proof j's two openings, as verify_batch draws it
            typename V::Transcript t("random");
            t.scalar(J.gk); t.point(J.Z); t.point(J.Wz); t.point(J.Wzw); t.scalar(J.c); t.scalar(J.ev.zw);
            t.done(raw);
            rr[i] = fr_from_be<FRP>(raw);
            rho[i] = fr_from_be<FRP>(&rho_be[32 * (size_t)j]);
        }

        // ---- stage 2 + the pairing, over any subset of the live proofs
        struct KeyAcc { const Job* job; Fr s1, s2, qcp[APK_MAX_COMMITMENTS]; };
        auto fold = [&](const std::vector<uint32_t>& sub, bool& good) -> int {
            std::vector<Aff> P;
            std::vector<Fr> S;
            std::map<uint32_t, KeyAcc> acc;   // by key index: the scalars of the key's own points, summed over its proofs
            Fr kG1 = Fr::zero();
            auto term = [&](const Aff& p, const Fr& s) { P.push_back(p); S.push_back(s); };
            for (uint32_t i : sub) {
                const Job& J = jobs[i];
                const Fr& w = rho[i];
                term(lin[i], w); term(J.L, w * J.gpow[0]); term(J.R, w * J.gpow[1]); term(J.O, w * J.gpow[2]);
                term(J.Z, w * rr[i]); term(J.Wz, w * J.zeta); term(J.Wzw, w * rr[i] * J.zeta * J.omega);
                auto it = acc.find(key_of[members[i]]);
                if (it == acc.end()) {
                    KeyAcc a{&J, Fr::zero(), Fr::zero(), {}};
                    for (uint32_t c = 0; c < APK_MAX_COMMITMENTS; c++) a.qcp[c] = Fr::zero();
                    it = acc.emplace(key_of[members[i]], a).first;
                }
                KeyAcc& a = it->second;
                a.s1 = a.s1 + w * J.gpow[3];
                a.s2 = a.s2 + w * J.gpow[4];
                for (uint32_t c = 0; c < J.k; c++) a.qcp[c] = a.qcp[c] + w * J.gpow[5 + c];
                kG1 = kG1 + w * (J.c + rr[i] * J.ev.zw);
            }
            for (const auto& kv : acc) {
                const KeyAcc& a = kv.second;
                term(a.job->key.s1, a.s1); term(a.job->key.s2, a.s2);
                for (uint32_t c = 0; c < a.job->k; c++) term(a.job->key.qcp[c], a.qcp[c]);
            }
            term(G1, Fr::neg(kG1));
            const uint64_t nA = P.size();
            for (uint32_t i : sub) { term(jobs[i].Wz, Fr::neg(rho[i])); term(jobs[i].Wzw, Fr::neg(rho[i] * rr[i])); }
            const uint64_t seg[3] = {0, nA, P.size()};
            Aff AB[2];
            const int rc = V::lincomb(device, P.data(), S.data(), seg, 2, AB);
            if (rc != APK_OK) return rc;
            if (tr && folds == 0) { V::put_pt(tr->a, AB[0]); V::put_pt(tr->b, AB[1]); }
            folds++;
            good = pairing_check2<FPP, PP>(AB[0], g2[0], AB[1], g2[1]);
            return APK_OK;
        };
        int rc = APK_OK;
        // `sub` is known to hold a rejected proof: find it / them
        auto search = [&](auto&& self, const std::vector<uint32_t>& sub) -> void {
            if (rc != APK_OK) return;
            if (sub.size() == 1) { ok[sub[0]] = 0; why[members[sub[0]]] = "plonk verification failed: pairing check"; return; }
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
        bool good = false;
        rc = fold(set, good);
        if (rc != APK_OK) return rc;
        if (!good) search(search, set);
        if (rc != APK_OK) return rc;
        for (uint32_t i : set) if (ok[i]) live[members[i]] = 1;
        return APK_OK;
    }

    int run() {
        using VN = HostVerifier<FrBN254, FpBN254, PairBN254, APK_BN254>;
        using VL = HostVerifier<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>;
        if (tr) memset(tr, 0, sizeof *tr);
        for (uint32_t i = 0; i < nb_keys; i++) {
            if (keys[i].curve != APK_BN254 && keys[i].curve != APK_BLS12_381) { set_error("key %u: unsupported curve: %d", i, keys[i].curve); return APK_ERR_ARG; }
            if (!VN::key_shape_ok(&keys[i])) return APK_ERR_ARG;
        }
        for (uint32_t j = 0; j < count; j++)
            if (key_of[j] >= nb_keys) { set_error("proof %u: key_of = %u, but there are %u keys", j, key_of[j], nb_keys); return APK_ERR_ARG; }
        readable.assign(count, 0); live.assign(count, 0); why.assign(count, std::string());
        for (uint32_t j = 0; j < count; j++) {
            status[j] = APK_ERR_VERIFY;
            if (prebad && !(*prebad)[j].empty()) { why[j] = (*prebad)[j]; continue; }
            const apk_verifying_key& vk = keys[key_of[j]];
            if (vk.nb_commitments > APK_MAX_COMMITMENTS || proofs[j].nb_commitments != vk.nb_commitments || proofs[j].curve != (uint32_t)vk.curve) {
                why[j] = "proof does not match the verifying key (curve / number of commitments)";
                continue;
            }
            if (nb_public_inputs[j] != vk.nb_public) {
                char buf[96];
                snprintf(buf, sizeof buf, "invalid witness size, got %u, expected %u (public)", nb_public_inputs[j], vk.nb_public);
                why[j] = buf;
                continue;
            }
            if (vk.nb_public && !pub_of(j)) { set_error("null argument"); return APK_ERR_ARG; }
            readable[j] = 1;
        }

        // the statement digest D and the weights: fixed before anything is folded, over every key and every proof as handed in
        uint8_t D[32];
        {
            Sha256 h;
            be32(h, nb_keys);
            for (uint32_t i = 0; i < nb_keys; i++) {
                if (keys[i].curve == APK_BN254) hash_key<VN>(h, keys[i]); else hash_key<VL>(h, keys[i]);
            }
            be32(h, count);
            for (uint32_t j = 0; j < count; j++) {
                const uint8_t mark = readable[j];
                h.update(&mark, 1);
                be32(h, key_of[j]);
                if (!mark) continue;
                const apk_verifying_key& vk = keys[key_of[j]];
                if (vk.curve == APK_BN254) hash_proof<VN>(h, proofs[j], vk, pub_of(j)); else hash_proof<VL>(h, proofs[j], vk, pub_of(j));
            }
            h.final(D);
        }
        rho_be.assign(32 * (size_t)count, 0);
        for (uint32_t j = 0; j < count; j++) {
            uint8_t d[32];
            Sha256 h;
            h.update("apk-batch-keys", 14); h.update(D, 32); be32(h, j); h.final(d);
            memcpy(&rho_be[32 * (size_t)j + 16], d + 16, 16);
        }
        // groups: keys that share the curve and the bytes of g1, g2[0], g2[1], numbered in the order of their first key
        group_of_key.assign(nb_keys, 0);
        uint32_t nb_groups = 0;
        for (uint32_t i = 0; i < nb_keys; i++) {
            uint32_t g = nb_groups;
            for (uint32_t o = 0; o < i; o++)
                if (keys[o].curve == keys[i].curve && !memcmp(keys[o].g1, keys[i].g1, sizeof keys[i].g1) && !memcmp(keys[o].g2, keys[i].g2, sizeof keys[i].g2)) { g = group_of_key[o]; break; }
            group_of_key[i] = g;
            if (g == nb_groups) nb_groups++;
        }
        if (tr) {
            memcpy(tr->d, D, 32);
            for (uint32_t j = 0; j < count && j < 4; j++) memcpy(tr->rho[j], &rho_be[32 * (size_t)j], 32);
            tr->groups = nb_groups;
        }
        if (count == 0) {                 // nothing to verify: the keys are checked
            for (uint32_t i = 0; i < nb_keys; i++) {
                if (keys[i].nb_commitments > APK_MAX_COMMITMENTS) continue;
                int rc;
                if (keys[i].curve == APK_BN254) { VN::Aff G1; VN::G2 g2[2]; rc = VN::key_check(&keys[i], G1, g2); }
                else { VL::Aff G1; VL::G2 g2[2]; rc = VL::key_check(&keys[i], G1, g2); }
                if (rc != APK_OK) return rc;
            }
            return APK_OK;
        }

        // a device also checks every point itself; the host checks of run_group stay as they are
        if (device >= 0) {
            int rc = device_check<VN>(APK_BN254);
            if (rc == APK_OK) rc = device_check<VL>(APK_BLS12_381);
            if (rc != APK_OK) return rc;
        }
        for (uint32_t g = 0; g < nb_groups; g++) {
            std::vector<uint32_t> members;
            int curve = APK_BN254;
            for (uint32_t j = 0; j < count; j++)
                if (readable[j] && group_of_key[key_of[j]] == g) { members.push_back(j); curve = keys[key_of[j]].curve; }
            if (members.empty()) continue;
            const int rc = curve == APK_BN254 ? run_group<FrBN254, FpBN254, PairBN254, APK_BN254>(members)
                                              : run_group<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(members);
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

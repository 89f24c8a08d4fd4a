// The wire formats of a proof and of its public inputs, stated ONCE for the writers (apk_marshal_proof,
// apk_marshal_public_inputs) and the readers (apk_unmarshal_proof, apk_unmarshal_public_inputs, apk_verify_blob*): what the
// reference's MarshalProof (helper.go:13-24, marshalPlonkBls12381Proof :27-88) and MarshalPublicInputs (helper.go:91-110) write and
// what its generated AVM verifiers take apart again.  Host only: no HIP include, not the verifier; builds with plain g++ against
// plonk_protocol.h (the byte encodings) - tools/san/proof_codec_check.cpp drives it stand-alone under ASAN + UBSAN.
//
//   proof blob        [L][R][O] [H1][H2][H3] l r o s1 s2 [Z] z(zeta w) [W_zeta] [W_zeta_w] qcp_0.. [Bsb22_0]..
//                     = 9 points + 6 scalars + k (scalar + point): 768 + 96 k bytes on BN254, 1056 + 128 k on BLS12-381
//   public inputs     nb_public x 32 bytes
// Points are X || Y big-endian, scalars canonical big-endian.  A reader knows the curve and takes k from the length.  It refuses a
// coordinate that is not below p and a scalar that is not below r, and reads an all-zero point as infinity; whether a point lies on
// the curve and in the subgroup is the verifier's question (verify_host.h load_and_check), not the reader's.  The writer's BLS12-381
// infinity (0x40, then zeros: gnark's RawBytes) has a coordinate above p, so the reader refuses it like any other such value - no
// proof the prover makes holds the point at infinity.
//
// Return codes: APK_OK; APK_ERR_VERIFY - the bytes are not an acceptable proof (a rejected proof, as for the AVM, never an argument
// error); APK_ERR_ARG - the call itself is wrong (unknown curve, buffer too small).  `err` receives the field's name and byte offset.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/apk.h"
#include "plonk_protocol.h"

namespace apk {

struct CodecError {
    char msg[192];
    CodecError() { msg[0] = 0; }
    void set(const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
    }
};

inline size_t codec_fp_bytes(int curve) { return curve == APK_BN254 ? 32 : curve == APK_BLS12_381 ? 48 : 0; }

// 9 points + 6 scalars + k x (scalar + point); 0 for an unknown curve or k > APK_MAX_COMMITMENTS
inline size_t proof_blob_len(int curve, uint32_t k) {
    const size_t pt = 2 * codec_fp_bytes(curve);
    if (!pt || k > APK_MAX_COMMITMENTS) return 0;
    return 9 * pt + 6 * 32 + (size_t)k * (32 + pt);
}
// the k a blob of `len` bytes holds; -1 when no k in 0..APK_MAX_COMMITMENTS gives that length
inline int proof_blob_k(int curve, size_t len) {
    for (uint32_t k = 0; k <= APK_MAX_COMMITMENTS; k++)
        if (proof_blob_len(curve, k) == len && len) return (int)k;
    return -1;
}

// big-endian bytes -> canonical limbs; false when the value is not below the modulus
template <class P>
inline bool fe_load_be(const uint8_t* be, Fe<P>& a) {
    constexpr int N = P::N;
    for (int i = 0; i < N; i++) {
        const uint8_t* p = be + 4 * (N - 1 - i);
        a.l[i] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
    }
    for (int i = N - 1; i >= 0; i--)
        if (a.l[i] != P::mod(i)) return a.l[i] < P::mod(i);
    return false;
}

// The proof's fields in wire order.  PROOF = apk_proof (reading) or const apk_proof (writing); the visitor's point() / scalar()
// return false to stop the walk.
template <class PROOF, class V>
inline bool proof_fields(PROOF* p, uint32_t k, V& v) {
    static const char* const lro[3] = {"L", "R", "O"};
    static const char* const h[3] = {"H1", "H2", "H3"};
    static const char* const ev[5] = {"l(zeta)", "r(zeta)", "o(zeta)", "s1(zeta)", "s2(zeta)"};
    static const char* const qcp[APK_MAX_COMMITMENTS] = {"qcp_0(zeta)", "qcp_1(zeta)"};
    static const char* const bsb[APK_MAX_COMMITMENTS] = {"Bsb22_0", "Bsb22_1"};
    static_assert(APK_MAX_COMMITMENTS == 2, "name the fields of every commitment");
    for (int i = 0; i < 3; i++) if (!v.point(lro[i], p->lro[i])) return false;               // helper.go:33-37
    for (int i = 0; i < 3; i++) if (!v.point(h[i], p->h[i])) return false;                   // :42-45
    for (int i = 0; i < 5; i++) if (!v.scalar(ev[i], p->claimed_values[1 + i])) return false; // :53-56
    if (!v.point("Z", p->z)) return false;                                                   // :59-60
    if (!v.scalar("z(zeta w)", p->zshift_value)) return false;                               // :63-64
    if (!v.point("W_zeta", p->batched_h)) return false;                                      // :67-68
    if (!v.point("W_zeta_w", p->zshift_h)) return false;                                     // :71-72
    for (uint32_t i = 0; i < k; i++) if (!v.scalar(qcp[i], p->claimed_values[6 + i])) return false;   // :76-79
    for (uint32_t i = 0; i < k; i++) if (!v.point(bsb[i], p->bsb22[i])) return false;        // :80-83
    return true;
}

template <class FRP, class FPP>
struct ProofCodec {
    static constexpr int FPB = FPP::N * 4;

    struct Reader {
        const uint8_t* in;
        size_t off;
        CodecError* err;
        bool point(const char* name, uint8_t* slot) {
            Fe<FPP> x, y;
            memset(slot, 0, APK_G1_MAX_BYTES);
            if (!fe_load_be<FPP>(in + off, x)) { err->set("proof blob: %s at byte %zu: X is not below the field modulus", name, off); return false; }
            if (!fe_load_be<FPP>(in + off + FPB, y)) { err->set("proof blob: %s at byte %zu: Y is not below the field modulus", name, off + FPB); return false; }
            const Affine<FPP> pt{Fe<FPP>::to_mont(x), Fe<FPP>::to_mont(y)};       // (0, 0) stays (0, 0): infinity
            memcpy(slot, &pt, sizeof pt);
            off += 2 * FPB;
            return true;
        }
        bool scalar(const char* name, uint8_t* slot) {
            Fe<FRP> s;
            if (!fe_load_be<FRP>(in + off, s)) { err->set("proof blob: %s at byte %zu: scalar is not below r", name, off); return false; }
            s = Fe<FRP>::to_mont(s);
            memcpy(slot, &s, sizeof s);
            off += 32;
            return true;
        }
    };
    struct Writer {
        uint8_t* out;
        bool point(const char*, const uint8_t* slot) {
            Affine<FPP> pt;
            memcpy(&pt, slot, sizeof pt);
            g1_raw(pt, out);
            out += 2 * FPB;
            return true;
        }
        bool scalar(const char*, const uint8_t* slot) {
            Fe<FRP> s;
            memcpy(&s, slot, sizeof s);
            fe_to_be<FRP>(s, out);
            out += 32;
            return true;
        }
    };

    static int read_proof(int curve, const uint8_t* blob, size_t len, apk_proof* out, CodecError* err) {
        memset(out, 0, sizeof *out);
        const int k = proof_blob_k(curve, len);
        if (k < 0) {
            err->set("proof blob: %zu bytes; a proof is %zu + %d k bytes, k = 0..%d", len, proof_blob_len(curve, 0), 32 + 2 * FPB, APK_MAX_COMMITMENTS);
            return APK_ERR_VERIFY;
        }
        out->curve = (uint32_t)curve;
        out->nb_commitments = (uint32_t)k;
        Reader r{blob, 0, err};
        if (!proof_fields(out, (uint32_t)k, r)) {
            memset(out, 0, sizeof *out);
            return APK_ERR_VERIFY;
        }
        return APK_OK;
    }
    static void write_proof(const apk_proof* p, uint8_t* out) {
        Writer w{out};
        proof_fields(p, p->nb_commitments, w);
    }
    static int read_public(const uint8_t* blob, size_t len, void* out_fr, uint32_t cap, uint32_t* nb_public, CodecError* err) {
        *nb_public = 0;
        if (len % 32) { err->set("public inputs blob: %zu bytes is not a multiple of 32", len); return APK_ERR_VERIFY; }
        if (len / 32 > cap) { err->set("public inputs blob: %zu values do not fit %u", len / 32, cap); return APK_ERR_ARG; }
        for (size_t i = 0; i < len / 32; i++) {
            Fe<FRP> s;
            if (!fe_load_be<FRP>(blob + 32 * i, s)) { err->set("public inputs blob: value %zu at byte %zu: scalar is not below r", i, 32 * i); return APK_ERR_VERIFY; }
            s = Fe<FRP>::to_mont(s);
            memcpy((uint8_t*)out_fr + 32 * i, &s, sizeof s);
        }
        *nb_public = (uint32_t)(len / 32);
        return APK_OK;
    }
    static void write_public(const void* pub, uint32_t nb_public, uint8_t* out) {
        for (uint32_t i = 0; i < nb_public; i++) {
            Fe<FRP> s;
            memcpy(&s, (const uint8_t*)pub + 32 * i, sizeof s);
            fe_to_be<FRP>(s, out + 32 * i);
        }
    }
};

using ProofCodecBN254 = ProofCodec<FrBN254, FpBN254>;
using ProofCodecBLS12381 = ProofCodec<FrBLS12381, FpBLS12381>;

// ---- by curve id (pointers checked by the caller) ------------------------------------------------------------------------------------
inline int unmarshal_proof(int curve, const uint8_t* blob, size_t len, apk_proof* out, CodecError* err) {
    if (curve == APK_BN254) return ProofCodecBN254::read_proof(curve, blob, len, out, err);
    if (curve == APK_BLS12_381) return ProofCodecBLS12381::read_proof(curve, blob, len, out, err);
    err->set("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}
inline int unmarshal_public_inputs(int curve, const uint8_t* blob, size_t len, void* out_fr, uint32_t cap, uint32_t* nb_public, CodecError* err) {
    if (curve == APK_BN254) return ProofCodecBN254::read_public(blob, len, out_fr, cap, nb_public, err);
    if (curve == APK_BLS12_381) return ProofCodecBLS12381::read_public(blob, len, out_fr, cap, nb_public, err);
    err->set("unsupported curve: %d", curve);
    return APK_ERR_ARG;
}
// *len = the bytes needed, also when `cap` is too small
inline int marshal_proof(const apk_proof* p, uint8_t* out, size_t cap, size_t* len, CodecError* err) {
    const int curve = (int)p->curve;
    if (!codec_fp_bytes(curve)) { err->set("unrecognized proof type"); return APK_ERR_ARG; }   // helper.go:21 panics here
    if (p->nb_commitments > APK_MAX_COMMITMENTS) { err->set("too many commitments"); return APK_ERR_ARG; }
    const size_t need = proof_blob_len(curve, p->nb_commitments);
    *len = need;
    if (cap < need) { err->set("buffer too small: need %zu bytes", need); return APK_ERR_ARG; }
    if (curve == APK_BN254) ProofCodecBN254::write_proof(p, out); else ProofCodecBLS12381::write_proof(p, out);
    return APK_OK;
}
inline int marshal_public_inputs(int curve, const void* pub, uint32_t nb_public, uint8_t* out, size_t cap, CodecError* err) {
    if (!codec_fp_bytes(curve)) { err->set("unsupported curve: %d", curve); return APK_ERR_ARG; }
    if (cap < (size_t)nb_public * 32) { err->set("buffer too small"); return APK_ERR_ARG; }
    if (curve == APK_BN254) ProofCodecBN254::write_public(pub, nb_public, out); else ProofCodecBLS12381::write_public(pub, nb_public, out);
    return APK_OK;
}

}  // namespace apk

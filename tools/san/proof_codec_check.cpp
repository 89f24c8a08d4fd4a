// Sanitizer tier: algoplonk_amd/csrc/proof_codec.h (the readers and writers of marshalled proofs and public inputs) driven
// stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer - no libapk, no GPU, no interpreter:
//     make -C algoplonk_amd/csrc san-codec && tools/san/proof_codec_check blobs.txt
// One blob per line (tests/test_proof_blob.py writes the fixture's):   curve kind hex      curve 0 BN254 / 1 BLS12-381, kind P = proof,
// I = public inputs.  Every blob is copied into a heap buffer of exactly its length, so a read past its end is a report.  Tried on
// each: the blob itself (a proof must come back byte for byte from the writer), every truncation length 0..len-1, the first and the
// last byte of every field inverted (a point's X and Y are two fields), all bytes 0x00, all bytes 0xFF.  Prints how many attempts of
// each kind were accepted and rejected - the test holds the counts against libapk's own on the same attempts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../algoplonk_amd/csrc/proof_codec.h"

using namespace apk;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

struct Counts { long accept = 0, reject = 0; };
static Counts g_counts[2][5];     // [proof / public][whole, truncation, flip, zeros, ones]
static const char* const KINDS[5] = {"whole", "truncation", "flip", "zeros", "ones"};
static int g_bad = 0;

// first and last byte of every field of a proof with k commitments
struct Offsets {
    size_t off = 0, fpb;
    std::vector<size_t> edges;
    bool point(const char*, const uint8_t*) { for (int c = 0; c < 2; c++) { edges.push_back(off); edges.push_back(off + fpb - 1); off += fpb; } return true; }
    bool scalar(const char*, const uint8_t*) { edges.push_back(off); edges.push_back(off + 31); off += 32; return true; }
};

// one attempt on an exactly sized heap copy; returns the reader's code
static int attempt(int curve, bool proof, const uint8_t* data, size_t len, int kind, apk_proof* parsed = nullptr) {
    uint8_t* heap = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(heap, data, len);
    CodecError err;
    int rc;
    if (proof) {
        apk_proof pr;
        rc = unmarshal_proof(curve, heap, len, &pr, &err);
        if (rc == APK_OK) {
            if (proof_blob_len(curve, pr.nb_commitments) != len) { printf("accepted %zu bytes as k = %u\n", len, pr.nb_commitments); g_bad++; }
            if (parsed) *parsed = pr;
        }
    } else {
        std::vector<uint8_t> out(len / 32 * 32 + 1);
        uint32_t nb = 0;
        rc = unmarshal_public_inputs(curve, heap, len, out.data(), (uint32_t)(len / 32), &nb, &err);
        if (rc == APK_OK && nb != len / 32) { printf("public inputs: %zu bytes gave %u values\n", len, nb); g_bad++; }
    }
    free(heap);
    if (rc != APK_OK && rc != APK_ERR_VERIFY) { printf("unexpected code %d (%s)\n", rc, err.msg); g_bad++; }
    if (rc != APK_OK && !err.msg[0]) { printf("a rejection without a message\n"); g_bad++; }
    Counts& c = g_counts[proof ? 0 : 1][kind];
    if (rc == APK_OK) c.accept++; else c.reject++;
    return rc;
}

static void run_blob(int curve, bool proof, const std::vector<uint8_t>& blob) {
    const size_t len = blob.size();
    apk_proof pr;
    memset(&pr, 0, sizeof pr);
    const int rc = attempt(curve, proof, blob.data(), len, 0, &pr);
    std::vector<size_t> edges;
    if (proof && rc == APK_OK) {
        // the writer gives the bytes back (no fixture proof holds the point at infinity)
        std::vector<uint8_t> back(len);
        size_t wrote = 0;
        CodecError err;
        if (marshal_proof(&pr, back.data(), len, &wrote, &err) != APK_OK || wrote != len || memcmp(back.data(), blob.data(), len)) { printf("round trip differs\n"); g_bad++; }
        Offsets o;
        o.fpb = codec_fp_bytes(curve);
        const apk_proof* cp = &pr;
        proof_fields(cp, pr.nb_commitments, o);
        if (o.off != len) { printf("field walk covers %zu of %zu bytes\n", o.off, len); g_bad++; }
        edges = o.edges;
    } else if (!proof) {
        for (size_t i = 0; i + 32 <= len; i += 32) { edges.push_back(i); edges.push_back(i + 31); }
    }
    for (size_t cut = 0; cut < len; cut++) attempt(curve, proof, blob.data(), cut, 1);
    for (size_t e : edges) {
        std::vector<uint8_t> m = blob;
        m[e] ^= 0xff;
        attempt(curve, proof, m.data(), len, 2);
    }
    attempt(curve, proof, std::vector<uint8_t>(len, 0x00).data(), len, 3);
    attempt(curve, proof, std::vector<uint8_t>(len, 0xff).data(), len, 4);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: proof_codec_check blobs.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int nb = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        int curve;
        std::string kind, hex;
        if (!(ss >> curve >> kind >> hex) || (kind != "P" && kind != "I") || (curve != APK_BN254 && curve != APK_BLS12_381)) { fprintf(stderr, "blob %d: malformed line\n", nb); return 2; }
        run_blob(curve, kind == "P", unhex(hex));
        nb++;
    }
    // an unknown curve is an argument error, never a parse
    {
        CodecError err;
        apk_proof pr;
        uint8_t b[32] = {0}, out[32];
        uint32_t n = 0;
        if (unmarshal_proof(7, b, sizeof b, &pr, &err) != APK_ERR_ARG || unmarshal_public_inputs(7, b, sizeof b, out, 1, &n, &err) != APK_ERR_ARG ||
            unmarshal_public_inputs(APK_BN254, b, sizeof b, out, 0, &n, &err) != APK_ERR_ARG || proof_blob_len(7, 0) != 0 || proof_blob_len(APK_BN254, 3) != 0) { printf("argument errors\n"); g_bad++; }
    }
    for (int p = 0; p < 2; p++)
        for (int k = 0; k < 5; k++) printf("%s %s accept %ld reject %ld\n", p ? "public" : "proof", KINDS[k], g_counts[p][k].accept, g_counts[p][k].reject);
    if (nb == 0 || g_bad) { printf("PROOF CODEC CHECK FAILED: %d problems in %d blobs\n", g_bad, nb); return 1; }
    printf("PROOF CODEC CHECK OK: %d blobs\n", nb);
    return 0;
}

// Sanitizer tier: the multi-point rule of algoplonk_amd/csrc/kzg_protocol.h (the weights, the two-segment fold on the host and
// the pairing check of kzg.BatchVerifyMultiPoints) driven stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer - no
// libapk, no GPU, no interpreter:
//     make -C algoplonk_amd/csrc san-kzg-multi && tools/san/kzg_multi_check cases.txt
// One case per line (tests/test_kzg_multi_host.py writes them from its big-integer model), every field hex of the C-ABI's
// in-memory encodings:
//     curve expect g1 g2 count digests points values hs
// curve 0 BN254 / 1 BLS12-381; expect 1 = the batch verifies, 0 = it is rejected, 2 = the key is refused, 3 = a scalar is not
// below r.  Prints, per case, the verdict and the weights (count Fr, Montgomery, hex) and KZG MULTI CHECK OK when every case
// ends as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../algoplonk_amd/csrc/backend.h"
#include "../../algoplonk_amd/csrc/kzg_protocol.h"

namespace apk {
void set_error(const char*, ...) {}
int env_int(const char*, int dflt, int, int) { return dflt; }
// (the fold of these cases runs on the host: device -1)
int g1_lincomb_segments_bn254(int, const void*, const void*, const uint64_t*, uint32_t, void*) { return APK_ERR_HIP; }
int g1_lincomb_segments_bls12381(int, const void*, const void*, const uint64_t*, uint32_t, void*) { return APK_ERR_HIP; }
}  // namespace apk

using namespace apk;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

struct Case {
    int curve, expect;
    uint32_t count;
    std::vector<uint8_t> g1, g2, digests, points, values, hs;
};

template <class FR, class FP, class PP, int CURVE_ID>
static int run_case(const Case& c, std::string& weights) {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    using Fr = Fe<FR>;
    using Aff = Affine<FP>;
    constexpr size_t FPB = FP::N * 4;
    if (c.g1.size() != 2 * FPB || c.g2.size() != 8 * FPB || c.count == 0 || c.digests.size() != c.count * sizeof(Aff) ||
        c.hs.size() != c.count * sizeof(Aff) || c.values.size() != c.count * sizeof(Fr) || c.points.size() != c.count * sizeof(Fr)) return -1;
    apk_kzg_vk vk{};
    vk.curve = CURVE_ID;
    memcpy(vk.g1, c.g1.data(), c.g1.size());
    memcpy(vk.g2[0], c.g2.data(), 4 * FPB);
    memcpy(vk.g2[1], c.g2.data() + 4 * FPB, 4 * FPB);
    Aff g1;
    typename K::G2 g2[2];
    if (K::key_load(&vk, g1, g2)) return 2;
    std::vector<Aff> digs(c.count), Hs(c.count);
    std::vector<Fr> vals(c.count), zs(c.count), lambda(c.count);
    memcpy(digs.data(), c.digests.data(), c.digests.size());
    memcpy(Hs.data(), c.hs.data(), c.hs.size());
    memcpy(vals.data(), c.values.data(), c.values.size());
    memcpy(zs.data(), c.points.data(), c.points.size());
    if (!K::multi_scalars_ok(c.count, zs.data(), vals.data())) return 3;
    K::multi_weights(&vk, g1, c.count, digs.data(), zs.data(), vals.data(), Hs.data(), lambda.data());
    const uint8_t* lb = reinterpret_cast<const uint8_t*>(lambda.data());
    char hex[3];
    for (size_t i = 0; i < c.count * sizeof(Fr); i++) { snprintf(hex, sizeof hex, "%02x", lb[i]); weights += hex; }
    const char* why = "";
    const int rc = K::multi_check(-1, &vk, g1, g2, c.count, digs.data(), zs.data(), vals.data(), Hs.data(), &why);
    return rc == APK_OK ? 1 : rc == APK_ERR_VERIFY ? 0 : -1;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: kzg_multi_check cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int nb = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        Case c;
        std::string g1, g2, digests, points, values, hs, weights;
        if (!(ss >> c.curve >> c.expect >> g1 >> g2 >> c.count >> digests >> points >> values >> hs)) { fprintf(stderr, "case %d: malformed line\n", nb); return 2; }
        c.g1 = unhex(g1); c.g2 = unhex(g2); c.digests = unhex(digests); c.points = unhex(points); c.values = unhex(values); c.hs = unhex(hs);
        const int got = c.curve == 0 ? run_case<FrBN254, FpBN254, PairBN254, APK_BN254>(c, weights) : run_case<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(c, weights);
        printf("case %d: curve %d count %u -> %d (expected %d) weights %s\n", nb, c.curve, c.count, got, c.expect, weights.empty() ? "-" : weights.c_str());
        if (got != c.expect) bad++;
        nb++;
    }
    if (nb == 0 || bad) { printf("KZG MULTI CHECK FAILED: %d of %d cases\n", bad, nb); return 1; }
    printf("KZG MULTI CHECK OK: %d cases\n", nb);
    return 0;
}

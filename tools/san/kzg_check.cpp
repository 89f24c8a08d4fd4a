// Sanitizer tier: algoplonk_amd/csrc/kzg_protocol.h (fold challenge, fold, pairing check, key and point checks) driven
// stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer - no libapk, no GPU, no interpreter:
//     make -C algoplonk_amd/csrc san-kzg && tools/san/kzg_check cases.txt
// One case per line (tests/test_kzg_host.py writes them from its big-integer model), every field hex of the C-ABI's in-memory
// encodings ("-" = empty):
//     curve batch expect g1 g2 count digests values point extra h
// curve 0 BN254 / 1 BLS12-381; batch 0 = kzg.Verify on (digests[0], values[0]), 1 = BatchVerifySinglePoint; expect 1 = the
// opening verifies, 0 = it is rejected, 2 = the key is refused.  Prints KZG CHECK OK when every case ends as expected.
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
}  // namespace apk

using namespace apk;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

struct Case {
    int curve, batch, expect;
    uint32_t count;
    std::vector<uint8_t> g1, g2, digests, values, point, extra, h;
};

template <class FR, class FP, class PP, int CURVE_ID>
static int run_case(const Case& c) {
    using K = KzgProtocol<FR, FP, PP, CURVE_ID>;
    using Fr = Fe<FR>;
    using Aff = Affine<FP>;
    constexpr size_t FPB = FP::N * 4;
    if (c.g1.size() != 2 * FPB || c.g2.size() != 8 * FPB || c.digests.size() != c.count * sizeof(Aff) ||
        c.values.size() != c.count * sizeof(Fr) || c.point.size() != sizeof(Fr) || c.h.size() != sizeof(Aff) || c.count == 0) return -1;
    apk_kzg_vk vk{};
    vk.curve = CURVE_ID;
    memcpy(vk.g1, c.g1.data(), c.g1.size());
    memcpy(vk.g2[0], c.g2.data(), 4 * FPB);
    memcpy(vk.g2[1], c.g2.data() + 4 * FPB, 4 * FPB);
    Aff g1, H;
    typename K::G2 g2[2];
    if (K::key_load(&vk, g1, g2)) return 2;
    std::vector<Aff> digs(c.count);
    std::vector<Fr> vals(c.count);
    Fr z;
    memcpy(digs.data(), c.digests.data(), c.digests.size());
    memcpy(vals.data(), c.values.data(), c.values.size());
    memcpy(&z, c.point.data(), sizeof z);
    memcpy(&H, c.h.data(), sizeof H);
    Aff digest = digs[0];
    Fr value = vals[0];
    if (c.batch) {
        for (const Aff& d : digs) if (!K::point_ok(d)) return 0;
        uint8_t raw[32];
        const Fr gamma = kzg_fold_challenge<FR, FP>(z, digs.data(), vals.data(), c.count, c.extra.data(), c.extra.size(), raw);
        K::kzg_fold(gamma, digs.data(), vals.data(), c.count, digest, value);
    }
    return K::kzg_check(g1, g2, digest, z, value, H) ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: kzg_check cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int nb = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        Case c;
        std::string g1, g2, digests, values, point, extra, h;
        if (!(ss >> c.curve >> c.batch >> c.expect >> g1 >> g2 >> c.count >> digests >> values >> point >> extra >> h)) { fprintf(stderr, "case %d: malformed line\n", nb); return 2; }
        c.g1 = unhex(g1); c.g2 = unhex(g2); c.digests = unhex(digests); c.values = unhex(values); c.point = unhex(point);
        c.extra = unhex(extra); c.h = unhex(h);
        const int got = c.curve == 0 ? run_case<FrBN254, FpBN254, PairBN254, APK_BN254>(c) : run_case<FrBLS12381, FpBLS12381, PairBLS12381, APK_BLS12_381>(c);
        printf("case %d: curve %d batch %d count %u -> %d (expected %d)\n", nb, c.curve, c.batch, c.count, got, c.expect);
        if (got != c.expect) bad++;
        nb++;
    }
    if (nb == 0 || bad) { printf("KZG CHECK FAILED: %d of %d cases\n", bad, nb); return 1; }
    printf("KZG CHECK OK: %d cases\n", nb);
    return 0;
}

// Prints the answers of the planner of apk_kzg_recover_cosets (algoplonk_amd/csrc/kzg_recover_plan.h) over a space it enumerates
// itself.  Host only, no GPU:
//   make -C algoplonk_amd/csrc recover-plan-dump   ->   tools/kzg_recover_plan_dump
//   make -C algoplonk_amd/csrc san-recover-plan    ->   tools/san/kzg_recover_plan_dump, the same program under ASAN + UBSAN
//   tools/kzg_recover_plan_dump plans    log n = 2 .. 6, every l = 2 .. n / 2, and the known sets "all", "one" (the last coset), "first"
//                                        (the first half), "even", "odd-reversed" (the odd cosets, rows in descending order), len = k l:
//                                          {"n": , "l": , "np": , "logs": [log n, log l, log n'], "indices": [..], "len": , "rc": , "k": , "m": ,
//                                           "row_of": [n'], "missing": [m], "vanish": [lanes, grid, block, lds], "scatter": [..], "divide": [..],
//                                           "tiles": , "check": [lo, hi]}
//   tools/kzg_recover_plan_dump grids    n' = 2, 4 .. 2^16 at l = 2, k = 1: the three launches; and the tile count at m = 0, 1, tile - 1,
//                                        tile, tile + 1 (n' = 1024):   {"np": , "m": , "vanish": [..], "scatter": [..], "divide": [..], "tiles": }
//   tools/kzg_recover_plan_dump rules    every argument rule at its edge:   {"rule": name, "n": , "l": , "count": , "len": , "rc": , "message": }
// Several words run one after the other.  tests/test_kzg_recover_host.py holds the output to a Python restatement.
#include <stdio.h>
#include <string.h>
#include <numeric>
#include "../algoplonk_amd/csrc/kzg_recover_plan.h"

using namespace apk;

static void print_launch(const char* name, const RecoverLaunch& L) { printf("\"%s\": [%u, %u, %u, %u], ", name, L.lanes, L.grid, L.block, L.lds_bytes); }

static void plan_line(uint32_t n, uint32_t l, const std::vector<uint64_t>& idx, uint64_t len) {
    const RecoverPlan p = recover_plan(n, l, (uint32_t)idx.size(), idx.data(), len);
    printf("{\"n\": %u, \"l\": %u, \"np\": %u, \"logs\": [%d, %d, %d], \"indices\": [", n, l, p.np, p.log_n, p.log_l, p.log_np);
    for (size_t i = 0; i < idx.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)idx[i]);
    printf("], \"len\": %llu, \"rc\": %d, \"k\": %u, \"m\": %u, \"row_of\": [", (unsigned long long)len, p.verdict.rc, p.k, p.m);
    for (size_t i = 0; i < p.row_of.size(); i++) printf("%s%d", i ? ", " : "", p.row_of[i]);
    printf("], \"missing\": [");
    for (size_t i = 0; i < p.missing.size(); i++) printf("%s%u", i ? ", " : "", p.missing[i]);
    printf("], ");
    print_launch("vanish", p.vanish);
    print_launch("scatter", p.scatter);
    print_launch("divide", p.divide);
    printf("\"tiles\": %u, \"check\": [%llu, %llu]}\n", p.tiles, (unsigned long long)p.check_lo, (unsigned long long)p.check_hi);
}

static void dump_plans() {
    for (int log_n = 2; log_n <= 6; log_n++)
        for (uint32_t l = 2; l <= (1u << log_n) / 2; l *= 2) {
            const uint32_t n = 1u << log_n, np = n / l;
            std::vector<uint64_t> all(np), one{np - 1}, first(np / 2), even, odd;
            std::iota(all.begin(), all.end(), 0);
            std::iota(first.begin(), first.end(), 0);
            for (uint32_t i = 0; i < np; i += 2) even.push_back(i);
            for (uint32_t i = np; i-- > 0;) if (i & 1) odd.push_back(i);
            for (const auto& idx : {all, one, first, even, odd})
                if (!idx.empty()) plan_line(n, l, idx, (uint64_t)idx.size() * l);
        }
}

static void grid_line(uint32_t np, uint32_t k) {
    std::vector<uint64_t> idx(k);
    std::iota(idx.begin(), idx.end(), 0);
    const RecoverPlan p = recover_plan(2ull * np, 2, k, idx.data(), 1);
    printf("{\"np\": %u, \"m\": %u, \"rc\": %d, ", np, p.m, p.verdict.rc);
    print_launch("vanish", p.vanish);
    print_launch("scatter", p.scatter);
    print_launch("divide", p.divide);
    printf("\"tiles\": %u}\n", p.tiles);
}

static void dump_grids() {
    for (uint32_t np = 2; np <= (1u << 16); np *= 2) grid_line(np, 1);
    for (uint32_t m : {0u, 1u, KZG_RECOVER_TILE - 1, KZG_RECOVER_TILE, KZG_RECOVER_TILE + 1}) grid_line(1024, 1024 - m);
}

static void rule_line(const char* rule, uint64_t n, uint32_t l, const std::vector<uint64_t>& idx, uint64_t len) {
    const uint32_t count = (uint32_t)idx.size();
    RecoverVerdict v = recover_check_call(l, count, len);
    if (v.rc == APK_OK) v = recover_plan(n, l, count, idx.data(), len).verdict;
    printf("{\"rule\": \"%s\", \"n\": %llu, \"l\": %u, \"count\": %u, \"len\": %llu, \"rc\": %d, \"message\": \"%s\"}\n", rule, (unsigned long long)n, l, count,
           (unsigned long long)len, v.rc, v.message);
}

static std::vector<uint64_t> range(uint64_t k) {
    std::vector<uint64_t> v(k);
    std::iota(v.begin(), v.end(), 0);
    return v;
}

static void dump_rules() {
    const uint64_t n = 64;
    const uint32_t l = 4, np = 16;
    rule_line("ok", n, l, range(4), 16);
    rule_line("count=0", n, l, {}, 1);
    rule_line("len=0", n, l, range(4), 0);
    rule_line("l=0", n, 0, range(4), 1);
    rule_line("l=1", n, 1, range(4), 1);
    rule_line("l=3", n, 3, range(4), 1);
    rule_line("l=n/2", n, 32, range(2), 64);
    rule_line("l=n", n, 64, range(1), 1);
    rule_line("count=n'", n, l, range(np), 64);
    rule_line("count=n'+1", n, l, range(np + 1), 64);
    rule_line("len=kl", n, l, range(5), 20);
    rule_line("len=kl+1", n, l, range(5), 21);
    rule_line("index=n'-1", n, l, {0, np - 1}, 8);
    rule_line("index=n'", n, l, {0, np}, 8);
    rule_line("repeat", n, l, {3, 7, 3}, 8);
    rule_line("np=2^16", 1ull << 17, 2, range(2), 4);
    rule_line("np=2^17", 1ull << 18, 2, range(2), 4);
    // the order of the rules: the first that fails is the one reported
    rule_line("order: count before index", n, l, std::vector<uint64_t>(np + 1, 99), 1);
    rule_line("order: index before repeat", n, l, {1, 1, 99}, 1);
    rule_line("order: repeat before len", n, l, {1, 1}, 99);
    rule_line("order: len before np", 1ull << 18, 2, range(2), 5);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: kzg_recover_plan_dump plans | grids | rules ...\n"); return 2; }
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "plans")) dump_plans();
        else if (!strcmp(argv[i], "grids")) dump_grids();
        else if (!strcmp(argv[i], "rules")) dump_rules();
        else { fprintf(stderr, "kzg_recover_plan_dump: unknown word %s\n", argv[i]); return 2; }
    }
    return 0;
}

// Prints the answers of the FK20 openings' planner (algoplonk_amd/csrc/kzg_fk20_plan.h) over a space it enumerates itself.  Host
// only, no GPU:
//   make -C algoplonk_amd/csrc fk20-plan-dump   ->   tools/kzg_fk20_plan_dump
//   make -C algoplonk_amd/csrc san-fk20-plan    ->   tools/san/kzg_fk20_plan_dump, the same program under ASAN + UBSAN
//   tools/kzg_fk20_plan_dump shape    log n = 3 .. 7, every l = 1, 2, 4 .. n / 2: the shape and the source of every position of t
//                                       {"log_n": , "l": , "n": , "np": , "logs": [log n, log l, log n'], "pair": [2n', n'], "prepare_stages": ,
//                                        "sub_log": , "t": [SRS index or -1 = infinity, 2n of them]}
//   tools/kzg_fk20_plan_dump gather   m = 2, 4 .. 2^16:  {"m": , "launches": [[k0, k1], ...]}
//   tools/kzg_fk20_plan_dump chunks   l = 2, 4 .. 2^10:  {"l": , "args_max": NTT_ARGS_MAX, "chunks": [[odd, c0, cnt], ...]}
//   tools/kzg_fk20_plan_dump rules    log n = 3 .. 7: the coset-size rule at l = 0 .. n + 1; for l = 1, 2, 4 .. n / 2 the SRS rule at
//                                     count = n-l-2 .. n-l+1 and n-2, n-1, the length rule and has_quotient at len = 0, 1, l, l+1, n, n+1
//                                       {"rule": "size" | "srs" | "len", "n": , "l": , "x": count or len, "rc": , "message": , "has_quotient": }
// Several words run one after the other.  tests/test_kzg_fk20_plan.py holds the output to tests/kzg_all_model.py,
// tests/kzg_cosets_model.py and a Python restatement of the rules.
#include <stdio.h>
#include <string.h>
#include "../algoplonk_amd/csrc/kzg_fk20_plan.h"

using namespace apk;

static void dump_shape() {
    for (int log_n = 3; log_n <= 7; log_n++)
        for (uint32_t l = 1; l <= (1u << log_n) / 2; l *= 2) {
            const Fk20Shape s = fk20_shape(log_n, l);
            printf("{\"log_n\": %d, \"l\": %u, \"n\": %u, \"np\": %u, \"logs\": [%d, %d, %d], \"pair\": [%u, %u], \"prepare_stages\": %d, \"sub_log\": %d, \"t\": [",
                   log_n, s.l, s.n, s.np, s.log_n, s.log_l, s.log_np, s.pair_big(), s.pair_small(), s.prepare_stages(), s.sub_log());
            for (uint32_t i = 0; i < 2 * s.n; i++) printf("%s%lld", i ? ", " : "", (long long)fk20_t_source(s, i));
            printf("]}\n");
        }
}

static void dump_gather() {
    for (uint32_t m = 2; m <= (1u << 16); m *= 2) {
        const Fk20Gather g = fk20_gather(m);
        printf("{\"m\": %u, \"launches\": [", m);
        for (int i = 0; i < g.count; i++) printf("%s[%u, %u]", i ? ", " : "", g.launch[i].k0, g.launch[i].k1);
        printf("]}\n");
    }
}

static void dump_chunks() {
    for (uint32_t l = 2; l <= (1u << 10); l *= 2) {
        printf("{\"l\": %u, \"args_max\": %d, \"chunks\": [", l, NTT_ARGS_MAX);
        for (uint32_t i = 0; i < fk20_chunks(l); i++) {
            const Fk20Chunk c = fk20_chunk(l, i);
            printf("%s[%d, %u, %d]", i ? ", " : "", c.odd, c.c0, c.cnt);
        }
        printf("]}\n");
    }
}

static void rule_line(const char* rule, uint32_t n, uint32_t l, long long x, const Fk20Verdict& v, int has_quotient) {
    printf("{\"rule\": \"%s\", \"n\": %u, \"l\": %u, \"x\": %lld, \"rc\": %d, \"message\": \"%s\", \"has_quotient\": %d}\n", rule, n, l, x, v.rc, v.message,
           has_quotient);
}

static void dump_rules() {
    for (int log_n = 3; log_n <= 7; log_n++) {
        const uint32_t n = 1u << log_n;
        for (uint32_t l = 0; l <= n + 1; l++) rule_line("size", n, l, 0, fk20_check_coset_size(n, l), -1);
        for (uint32_t l = 1; l <= n / 2; l *= 2) {
            const Fk20Shape s = fk20_shape(log_n, l);
            const long long counts[6] = {(long long)n - l - 2, (long long)n - l - 1, (long long)n - l, (long long)n - l + 1, (long long)n - 2, (long long)n - 1};
            for (long long c : counts) rule_line("srs", n, l, c, fk20_check_srs(n, l, (uint64_t)c), -1);
            const long long lens[6] = {0, 1, l, (long long)l + 1, n, (long long)n + 1};
            for (long long len : lens) rule_line("len", n, l, len, fk20_check_len(n, l, (uint64_t)len), fk20_has_quotient(s, (uint64_t)len) ? 1 : 0);
        }
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: kzg_fk20_plan_dump shape | gather | chunks | rules ...\n"); return 2; }
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "shape")) dump_shape();
        else if (!strcmp(argv[i], "gather")) dump_gather();
        else if (!strcmp(argv[i], "chunks")) dump_chunks();
        else if (!strcmp(argv[i], "rules")) dump_rules();
        else { fprintf(stderr, "kzg_fk20_plan_dump: unknown word %s\n", argv[i]); return 2; }
    }
    return 0;
}

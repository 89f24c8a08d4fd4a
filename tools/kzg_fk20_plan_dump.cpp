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
//   tools/kzg_fk20_plan_dump multi    the batched call (apk_kzg_open_cosets_multi), one line per answer, each with a "multi" key:
//       "groups"  count = 1 .. 64:            {"multi": "groups", "count": , "max": 64, "group_max": 16, "groups": [[b0, size], ...]}
//       "chunks"  l in {2, 16, 64} x G in {1, 3, 16}:  {"multi": "chunks", "l": , "G": , "rows": G l, "args_max": , "chunks": [[odd, c0, cnt], ...]}
//       "sizes"   (log n, l) = (3, 4), (3, 2), (7, 2), (12, 64), (17, 64), (14, 64) - n' = 2, 4, 64, 64, 2048, 256 - x G in {1, 3, 16}: the scratch
//                 in points and scalars and every grid
//                                       {"multi": "sizes", "log_n": , "l": , "np": , "G": , "points": , "scalars": , "upload": , "big_points": ,
//                                        "small_points": , "grid_scalars": , "grid_pointwise": [x, y], "log_group": , "grid_points": , "grid_small_stage": }
//       "layout"  (n, l) = (8, 2), (8, 4), (64, 8), G = 3: every index of the layout, b-major
//                                       {"multi": "layout", "n": , "l": , "G": , "skips_infinity_rows": 0, "value0": [G], "row": [[l] x G],
//                                        "by_coset": [[n] x G]  (by_coset[b][i l + j]), "work_hat": [[2n'] x G], "work_cc": [[2n'] x G],
//                                        "second": [[n'] x G]  (position of k), "gather_source": [[n'] x G]  (-1 = infinity), "result": [[n'] x G]}
//       "check"   n = 8, l = 2: the argument rules in their order - every combination of msm_only, prepared, count in {0, 1, 2, 64, 65},
//                 a null polys / lens / out_h / polys[first] / polys[last], and len in {0, 1, n, n + 1} in the first and in the last row
//                                       {"multi": "check", "n": , "msm_only": , "prepared": , "count": , "null": "" | "polys" | "lens" | "out_h" | "first" | "last",
//                                        "bad_row": -1 | 0 | count - 1, "len": , "rc": , "message": }
//                 and the wording of rule 6:  {"multi": "not_device", "row": , "rc": , "message": }
// Several words run one after the other.  tests/test_kzg_fk20_plan.py holds the output to tests/kzg_all_model.py,
// tests/kzg_cosets_model.py and a Python restatement of the rules; tests/test_kzg_cosets_multi_plan.py does the same for the word `multi`.
#include <stdio.h>
#include <string.h>
#include <initializer_list>
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

static void dump_multi() {
    for (uint32_t count = 1; count <= FK20_MULTI_MAX; count++) {
        printf("{\"multi\": \"groups\", \"count\": %u, \"max\": %u, \"group_max\": %u, \"groups\": [", count, FK20_MULTI_MAX, FK20_GROUP_MAX);
        for (uint32_t g = 0; g < fk20_multi_groups(count); g++) {
            const Fk20Group grp = fk20_multi_group(count, g);
            printf("%s[%u, %u]", g ? ", " : "", grp.b0, grp.size);
        }
        printf("]}\n");
    }
    const uint32_t Gs[3] = {1, 3, 16};
    for (uint32_t l : {2u, 16u, 64u})
        for (uint32_t G : Gs) {
            const Fk20Multi m = fk20_multi(7, l, G);
            printf("{\"multi\": \"chunks\", \"l\": %u, \"G\": %u, \"rows\": %u, \"args_max\": %d, \"chunks\": [", l, G, m.rows(), NTT_ARGS_MAX);
            for (uint32_t i = 0; i < fk20_chunks(m.rows()); i++) {
                const Fk20Chunk c = fk20_chunk(m.rows(), i);
                printf("%s[%d, %u, %d]", i ? ", " : "", c.odd, c.c0, c.cnt);
            }
            printf("]}\n");
        }
    const int sizes[6][2] = {{3, 4}, {3, 2}, {7, 2}, {12, 64}, {17, 64}, {14, 64}};      // n' = 2, 4, 64, 64, 2048, 256
    for (const auto& sz : sizes)
        for (uint32_t G : Gs) {
            const Fk20Multi m = fk20_multi(sz[0], (uint32_t)sz[1], G);
            printf("{\"multi\": \"sizes\", \"log_n\": %d, \"l\": %u, \"np\": %u, \"G\": %u, \"points\": %zu, \"scalars\": %zu, \"upload\": %zu, "
                   "\"big_points\": %u, \"small_points\": %u, \"grid_scalars\": %u, \"grid_pointwise\": [%u, %u], \"log_group\": %d, \"grid_points\": %u, "
                   "\"grid_small_stage\": %u}\n",
                   sz[0], m.s.l, m.s.np, G, m.scratch_points(), m.scratch_scalars(), m.upload_scalars(), m.big_points(), m.small_points(), m.grid_scalars(),
                   m.grid_pointwise_x(), m.grid_pointwise_y(), fk20_pointwise_log_group(m.s.log_l), m.grid_points(), m.grid_small_stage());
        }
    const int layouts[3][2] = {{3, 2}, {3, 4}, {6, 8}};
    for (const auto& ly : layouts) {
        const Fk20Multi m = fk20_multi(ly[0], (uint32_t)ly[1], 3);
        const Fk20Shape& s = m.s;
        printf("{\"multi\": \"layout\", \"n\": %u, \"l\": %u, \"G\": %u, \"skips_infinity_rows\": %d", s.n, s.l, m.G, FK20_MULTI_SKIPS_INFINITY_ROWS ? 1 : 0);
        printf(", \"value0\": [");
        for (uint32_t b = 0; b < m.G; b++) printf("%s%zu", b ? ", " : "", m.value(b, 0));
        printf("], \"row\": [");
        for (uint32_t b = 0; b < m.G; b++) {
            printf("%s[", b ? ", " : "");
            for (uint32_t c = 0; c < s.l; c++) printf("%s%zu", c ? ", " : "", m.row(b, c));
            printf("]");
        }
        printf("], \"by_coset\": [");
        for (uint32_t b = 0; b < m.G; b++) {
            printf("%s[", b ? ", " : "");
            for (uint32_t i = 0; i < s.np; i++)
                for (uint32_t j = 0; j < s.l; j++) printf("%s%zu", i + j ? ", " : "", m.by_coset(b, i, j));
            printf("]");
        }
        printf("], \"work_hat\": [");
        for (uint32_t b = 0; b < m.G; b++) {
            printf("%s[", b ? ", " : "");
            for (uint32_t i = 0; i < s.pair_big(); i++) printf("%s%zu", i ? ", " : "", m.work_hat(b, i));
            printf("]");
        }
        printf("], \"work_cc\": [");
        for (uint32_t b = 0; b < m.G; b++) {
            printf("%s[", b ? ", " : "");
            for (uint32_t k = 0; k < s.pair_big(); k++) printf("%s%zu", k ? ", " : "", m.work_cc(b, k));
            printf("]");
        }
        printf("], \"second\": [");
        for (uint32_t b = 0; b < m.G; b++) {
            printf("%s[", b ? ", " : "");
            for (uint32_t k = 0; k < s.np; k++) printf("%s%zu", k ? ", " : "", m.second_at(b, k));
            printf("]");
        }
        printf("], \"gather_source\": [");
        for (uint32_t b = 0; b < m.G; b++) {
            printf("%s[", b ? ", " : "");
            for (uint32_t k = 0; k < s.np; k++) printf("%s%lld", k ? ", " : "", (long long)m.gather_source(b, k));
            printf("]");
        }
        printf("], \"result\": [");
        for (uint32_t b = 0; b < m.G; b++) {
            printf("%s[", b ? ", " : "");
            for (uint32_t i = 0; i < s.np; i++) printf("%s%zu", i ? ", " : "", m.result(b, i));
            printf("]");
        }
        printf("]}\n");
    }
    // the argument rules: every combination, so that the ORDER shows (the first rule that fails is the one reported)
    const uint32_t n = 8, l = 2;
    static const int some = 0;
    const void* polys[FK20_MULTI_MAX + 1];
    uint64_t lens[FK20_MULTI_MAX + 1];
    const char* nulls[6] = {"", "polys", "lens", "out_h", "first", "last"};
    for (int msm_only = 0; msm_only < 2; msm_only++)
        for (int prepared = 0; prepared < 2; prepared++)
            for (uint32_t count : {0u, 1u, 2u, 64u, 65u})
                for (const char* null : nulls)
                    for (int bad_row : {-1, 0, 1})                  // 1 = the last row
                        for (uint64_t len : {0ull, 1ull, 8ull, 9ull}) {
                            if (bad_row < 0 && len != 1) continue;   // (no row differs: every length is 3)
                            for (uint32_t b = 0; b <= FK20_MULTI_MAX; b++) { polys[b] = &some; lens[b] = 3; }
                            const uint32_t last = count ? count - 1 : 0;
                            if (!strcmp(null, "first")) polys[0] = nullptr;
                            if (!strcmp(null, "last")) polys[last] = nullptr;
                            if (bad_row >= 0) lens[bad_row ? last : 0] = len;
                            const Fk20Verdict v = fk20_multi_check(msm_only != 0, prepared ? l : 0, n, count, strcmp(null, "polys") ? polys : nullptr,
                                                                   strcmp(null, "lens") ? lens : nullptr, strcmp(null, "out_h") ? (const void*)&some : nullptr);
                            printf("{\"multi\": \"check\", \"n\": %u, \"msm_only\": %d, \"prepared\": %d, \"count\": %u, \"null\": \"%s\", \"bad_row\": %d, "
                                   "\"len\": %llu, \"rc\": %d, \"message\": \"%s\"}\n",
                                   n, msm_only, prepared, count, null, bad_row < 0 ? -1 : (int)(bad_row ? last : 0), (unsigned long long)(bad_row < 0 ? 3 : len), v.rc,
                                   v.message);
                        }
    for (uint32_t row : {0u, 63u}) {
        const Fk20Verdict v = fk20_multi_not_device(row);
        printf("{\"multi\": \"not_device\", \"row\": %u, \"rc\": %d, \"message\": \"%s\"}\n", row, v.rc, v.message);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: kzg_fk20_plan_dump shape | gather | chunks | rules | multi ...\n"); return 2; }
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "shape")) dump_shape();
        else if (!strcmp(argv[i], "gather")) dump_gather();
        else if (!strcmp(argv[i], "chunks")) dump_chunks();
        else if (!strcmp(argv[i], "rules")) dump_rules();
        else if (!strcmp(argv[i], "multi")) dump_multi();
        else { fprintf(stderr, "kzg_fk20_plan_dump: unknown word %s\n", argv[i]); return 2; }
    }
    return 0;
}

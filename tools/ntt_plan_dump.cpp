// Prints the NTT planner's decisions (algoplonk_amd/csrc/ntt_plan.h) as JSON, one line per input line: what one launch sequence of
// `count` same-size transforms takes.  Host only, no GPU:
//   make -C algoplonk_amd/csrc ntt-plan-dump   ->   tools/ntt_plan_dump
// A line (on stdin, or the program's arguments as one line):
//   log_n count  TILE_LOG STAGES RADIX4 THREADS  loaded loaded_foreign have_wide
// TILE_LOG, STAGES, RADIX4 and THREADS are the APK_NTT_* knobs of those names as ntt_run.h hands them to the planner (0 0 -1 0: the
// rules).  The tile element is 36 bytes (FeU of both scalar fields); out_len = 2^log_n, no twiddle shift, canonical outputs.
// tests/test_ntt_model.py holds tests/ntt_model.py to this output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../algoplonk_amd/csrc/ntt_plan.h"

using namespace apk;

static void dump(char* line) {
    long v[9];
    int nv = 0;
    for (char* t = strtok(line, " \t\r\n"); t && nv < 9; t = strtok(nullptr, " \t\r\n")) v[nv++] = strtol(t, nullptr, 0);
    if (nv == 0) return;
    if (nv < 9 || v[0] < 1 || v[0] > 31) { printf("{\"error\": \"expected: log_n (1..31) count TILE_LOG STAGES RADIX4 THREADS loaded loaded_foreign have_wide\"}\n"); return; }
    NttKnobs k;
    k.tile_log = (int)v[2]; k.stages = (int)v[3]; k.radix4 = (int)v[4]; k.threads = (int)v[5];
    NttPlanIn in{};
    in.log_n = (int)v[0]; in.count = (int)v[1];
    in.out_len = 1u << in.log_n;
    in.fe_u_bytes = 36;
    in.loaded = v[6] != 0; in.loaded_foreign = v[7] != 0; in.have_wide = v[8] != 0;
    const NttPlan p = ntt_plan(k, in);
    printf("{\"rc\": %d, \"message\": \"%s\"", p.rc, p.message);
    if (p.rc != APK_OK) { printf("}\n"); return; }
    printf(", \"tile_log\": %d, \"passes\": [", p.pass[0].tile_log);
    for (int i = 0; i < p.passes; i++) {
        const NttPassArgs& a = p.pass[i];
        printf("%s[%d, %d, %d, %d, %d]", i ? ", " : "", a.t0, a.t1, a.first, a.last, a.radix4);
    }
    printf("], \"grid_x\": %u, \"threads\": %u, \"lds_bytes\": %llu, \"needs_wide\": %d, \"paths\": %u}\n", p.grid_x, p.threads,
           (unsigned long long)p.lds_bytes, (int)p.needs_wide, p.paths);
}

int main(int argc, char** argv) {
    static char line[4096];
    if (argc > 1) {
        line[0] = 0;
        for (int i = 1; i < argc; i++) { strncat(line, argv[i], sizeof line - strlen(line) - 2); strcat(line, " "); }
        dump(line);
        return 0;
    }
    while (fgets(line, sizeof line, stdin)) dump(line);
    return 0;
}

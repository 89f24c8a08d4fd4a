// Prints the gang planner's decisions (algoplonk_amd/csrc/gang_plan.h) over a space it enumerates itself.  Host only, no GPU:
//   make -C algoplonk_amd/csrc gang-plan-dump   ->   tools/gang_plan_dump
//   tools/gang_plan_dump meetings   every meeting of 1..4 requests - each an MSM batch (table A or B, 1..4 MSMs: mA1 .. mB4), a batch of
//                                   transforms (shape X or Y, 1, 3 or 4 of them: nX1 .. nY4) or a flush (f) - at the capacity pairs
//                                   (MSM, NTT) = (4, 8) (8, 4) (12, 16) (16, 12).  One JSON line per plan:
//                                     {"caps": [msm, ntt], "reqs": ["mA3", ...], "groups": [[kind, [req ...], [first ...], total, res_base, [res_off ...]], ...]}
//   tools/gang_plan_dump shapes     two transform requests that differ in ONE field of the shape (0 = none .. 8), and two MSM requests
//                                   over the same / another table: "<what> <groups>" per line
//   tools/gang_plan_dump flush      every gang of 1..4 members with 0..3 recorded launches each over the signatures a, b, c (b is a's
//                                   kernel with another grid.x, c another kernel with a's shape), walked step by step the way
//                                   gang_flush walks it.  One line per gang, the launches of step 0 | of step 1 | of step 2, each the members
//                                   it carries:  <member 0's list>,<member 1's>,... = 02 1|0 1|2
//   tools/gang_plan_dump sigs       two members whose one record differs in ONE compared field (0 = none .. 5): "<field> <groups>"
// tests/test_gang_model.py holds tests/gang_model.py - the rules as gang_launch and flush_cmds stated them before this header - to
// this output, and checks the plans' invariants.
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../algoplonk_amd/csrc/gang_plan.h"

using namespace apk;

static const char TABLES[2] = {'A', 'B'}, SHAPES[2] = {'X', 'Y'};
static const int NTT_COUNTS[3] = {1, 3, 4};
static const int PRE = 0, POST = 0, SCALE = 0;      // addresses to tell tables and twiddle vectors apart

struct Choice { std::string name; GangPlanReq req; };

static std::vector<Choice> choices() {
    std::vector<Choice> c;
    for (int t = 0; t < 2; t++)
        for (uint32_t b = 1; b <= 4; b++) c.push_back({std::string("m") + TABLES[t] + std::to_string(b), GangPlanReq{GANG_KIND_MSM, b, &TABLES[t], GangNttShape{}}});
    for (int s = 0; s < 2; s++)
        for (int k : NTT_COUNTS)      // shape Y: the inverse transform, everything else as X
            c.push_back({std::string("n") + SHAPES[s] + std::to_string(k), GangPlanReq{GANG_KIND_NTT, (uint32_t)k, nullptr, GangNttShape{1, s == 1, 4096, &PRE, &POST, &SCALE, 0, false}}});
    c.push_back({"f", GangPlanReq{GANG_KIND_FLUSH, 0, nullptr, GangNttShape{}}});
    return c;
}

static void dump_meetings() {
    const std::vector<Choice> ch = choices();
    const uint32_t caps[4][2] = {{4, 8}, {8, 4}, {12, 16}, {16, 12}};
    const int C = (int)ch.size();
    for (const auto& cap : caps)
        for (int count = 1; count <= GANG_MAX; count++) {
            int total = 1;
            for (int i = 0; i < count; i++) total *= C;
            for (int code = 0; code < total; code++) {
                GangPlanReq reqs[GANG_MAX];
                int pick[GANG_MAX];
                for (int i = 0, c = code; i < count; i++, c /= C) { pick[i] = c % C; reqs[i] = ch[pick[i]].req; }
                const GangPlan p = gang_plan_meeting(reqs, count, cap[0], cap[1]);
                printf("{\"caps\": [%u, %u], \"reqs\": [", cap[0], cap[1]);
                for (int i = 0; i < count; i++) printf("%s\"%s\"", i ? ", " : "", ch[pick[i]].name.c_str());
                printf("], \"groups\": [");
                for (int g = 0; g < p.groups; g++) {
                    const GangGroup& G = p.group[g];
                    printf("%s[%d, [", g ? ", " : "", G.kind);
                    for (int k = 0; k < G.n; k++) printf("%s%d", k ? ", " : "", G.req[k]);
                    printf("], [");
                    for (int k = 0; k < G.n; k++) printf("%s%u", k ? ", " : "", G.first[k]);
                    printf("], %u, %u, [", G.total, G.res_base);
                    for (int k = 0; k < G.n; k++) printf("%s%u", k ? ", " : "", G.res_off(k));
                    printf("]]");
                }
                printf("]}\n");
            }
        }
}

static void dump_shapes() {
    const GangNttShape base{1, false, 4096, &PRE, &POST, &SCALE, 0, false};
    for (int f = 0; f <= 8; f++) {
        GangNttShape o = base;
        if (f == 1) o.which = 0;
        if (f == 2) o.inverse = true;
        if (f == 3) o.out_len = 4095;
        if (f == 4) o.pre = &POST;
        if (f == 5) o.post = &SCALE;
        if (f == 6) o.scale = &PRE;
        if (f == 7) o.sub_log = 1;
        if (f == 8) o.semi = true;
        const GangPlanReq reqs[2] = {{GANG_KIND_NTT, 2, nullptr, base}, {GANG_KIND_NTT, 2, nullptr, o}};
        printf("ntt%d %d\n", f, gang_plan_meeting(reqs, 2, 16, 16).groups);
    }
    for (int t = 0; t < 2; t++) {
        const GangPlanReq reqs[2] = {{GANG_KIND_MSM, 2, &TABLES[0], GangNttShape{}}, {GANG_KIND_MSM, 2, &TABLES[t], GangNttShape{}}};
        printf("msm%d %d\n", t, gang_plan_meeting(reqs, 2, 16, 16).groups);
    }
}

static GangSig sig_of(char c) {
    if (c == 'a') return GangSig{true, 0x1000, 8, 1, 256, 0};
    if (c == 'b') return GangSig{true, 0x1000, 9, 1, 256, 0};
    return GangSig{true, 0x2000, 8, 1, 256, 0};
}

static void dump_flush() {
    std::vector<std::string> lists = {""};
    for (size_t lo = 0, len = 1; len <= 3; len++) {
        const size_t hi = lists.size();
        for (size_t i = lo; i < hi; i++) for (char c = 'a'; c <= 'c'; c++) lists.push_back(lists[i] + c);
        lo = hi;
    }
    const int L = (int)lists.size();      // 40
    std::string line;
    for (int count = 1; count <= GANG_MAX; count++) {
        int total = 1;
        for (int i = 0; i < count; i++) total *= L;
        for (int code = 0; code < total; code++) {
            const std::string* rec[GANG_MAX];
            size_t longest = 0;
            line.clear();
            for (int m = 0, c = code; m < count; m++, c /= L) {
                rec[m] = &lists[c % L];
                if (rec[m]->size() > longest) longest = rec[m]->size();
                if (m) line += ',';
                line += *rec[m];
            }
            line += " = ";
            for (size_t i = 0; i < 3; i++) {       // gang_flush's walk (gang_run.h), a step at a time; it stops at the longest list
                if (i) line += '|';
                if (i >= longest) continue;
                GangSig sigs[GANG_MAX];
                for (int m = 0; m < count; m++) sigs[m] = i < rec[m]->size() ? sig_of((*rec[m])[i]) : GangSig{};
                const GangFlushStep s = gang_plan_flush_step(sigs, count);
                for (int g = 0; g < s.groups; g++) {
                    if (g) line += ' ';
                    for (int k = 0; k < s.n[g]; k++) line += (char)('0' + s.member[g][k]);
                }
            }
            line += '\n';
            fputs(line.c_str(), stdout);
        }
    }
}

static void dump_sigs() {
    for (int f = 0; f <= 5; f++) {
        GangSig sigs[2] = {sig_of('a'), sig_of('a')};
        if (f == 1) sigs[1].fn = 0x2000;
        if (f == 2) sigs[1].grid_x = 9;
        if (f == 3) sigs[1].grid_y = 2;
        if (f == 4) sigs[1].block_x = 64;
        if (f == 5) sigs[1].lds = 1024;
        printf("%d %d\n", f, gang_plan_flush_step(sigs, 2).groups);
    }
}

int main(int argc, char** argv) {
    const char* what = argc > 1 ? argv[1] : "";
    if (!strcmp(what, "meetings")) dump_meetings();
    else if (!strcmp(what, "shapes")) dump_shapes();
    else if (!strcmp(what, "flush")) dump_flush();
    else if (!strcmp(what, "sigs")) dump_sigs();
    else { fprintf(stderr, "usage: gang_plan_dump meetings | shapes | flush | sigs\n"); return 2; }
    return 0;
}

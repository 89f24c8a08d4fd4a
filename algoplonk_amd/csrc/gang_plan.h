// The gang's planner: what ONE meeting of a gang (gang.h) launches - which members' MSM batches and transforms share a launch
// sequence, where every member's operands sit inside the merged batch and its sums in the lead's result area - and which of the
// kernels the members recorded on their way to the meeting go out as one launch.  Plain integer bookkeeping: no HIP include, no
// device, builds with `g++ -std=c++17` - tools/gang_plan_dump.cpp prints its plans over an enumerated space and
// tests/test_gang_model.py holds the Python model (tests/gang_model.py) to them on the CPU; tools/san/host_hammer.cpp runs
// meetings of real threads through it.  GPU-free like msm_plan.h and ntt_plan.h.
//
// gang_run.h launches what gang_plan_flush says; the backend (backend_impl.h gang_launch) turns its requests into GangPlanReq
// records, asks for the plan and assembles the launch arguments from its offsets.  A mistake in these rules hands a member its
// neighbour's commitment with APK_OK: they stand here, each in ONE place.
#pragma once
#include <stdint.h>
#include "gang.h"

namespace apk {

// GangReq::kind - what a member came to the meeting for
enum { GANG_KIND_MSM = 1,      // a commitment batch (commit)
       GANG_KIND_NTT = 2,      // a batch of same-size transforms (run_ntt_batch)
       GANG_KIND_FLUSH = 3 };  // nothing but the kernels it has recorded: it is about to wait for the stream (sync_results)

// ---- the meeting --------------------------------------------------------------------------------------------------------------
// What makes transforms of two members one launch: everything the pass kernel takes ONCE per launch.  (The operands' pointers and
// input lengths are per transform and may differ.)  pre / post / scale are compared as addresses only.
struct GangNttShape {
    int which;
    bool inverse;
    uint32_t out_len;
    const void *pre, *post, *scale;
    int sub_log;
    bool semi;
    bool operator==(const GangNttShape& o) const {
        return which == o.which && inverse == o.inverse && out_len == o.out_len && pre == o.pre && post == o.post && scale == o.scale && sub_log == o.sub_log && semi == o.semi;
    }
};
// one member's request, as far as the plan depends on it
struct GangPlanReq {
    int kind;
    uint32_t count;           // MSM: the batch (1..MSM_MAX_BATCH); NTT: the transforms (1..NTT_MAX_BATCH); FLUSH: unused
    const void* table;        // MSM: the bases' table, compared as an address
    GangNttShape shape;       // NTT
};
// one launch sequence: the requests req[0..n) (indices into the meeting's list, ascending) as ONE batch of `total` operands
struct GangGroup {
    int kind;
    int n;
    int req[GANG_MAX];
    uint32_t first[GANG_MAX]; // req[k]'s operands are [first[k], first[k] + its count) of the merged batch
    uint32_t total;
    uint32_t res_base;        // MSM: the sequence writes its `total` sums from here on in the lead's XYZZ result area
    uint32_t res_off(int k) const { return res_base + first[k]; }     // ... so req[k]'s own sums start here
};
struct GangPlan {
    int groups = 0;
    GangGroup group[GANG_MAX];     // in launch order
};

// The merged launches of one meeting.  `reqs` are the posted requests in member-index order (Gang::run_locked); msm_cap is the
// number of MSMs the lead's workspace takes in one sequence (ws_batch), ntt_cap the transforms its scratch takes
// (NTT_MAX_BATCH x the context's gang size).
//
// Requests that can share a launch sequence do - MSM batches over the same table, transforms of the same shape - anything else
// goes by itself.  First fit in request order: the first request not yet placed opens a group, and every later one that matches
// it and still fits joins, behind those already in.  A request that does not match the opener, or does not fit, is left for a
// later group; FLUSH requests belong to none.  (Every request fits by itself - a proof's batch is at most MSM_MAX_BATCH /
// NTT_MAX_BATCH, the capacities at least that - so every MSM / NTT request is in exactly one group.)
//
// Nothing is reordered inside a member: it has ONE request per meeting, and the sequence that carries it is queued behind
// everything any member launched or recorded before the meeting (the flush below goes first), so each proof sees the stream
// order it would have had alone.
//
// The MSM sums of a meeting's sequences sit one behind the other in the lead's XYZZ area (slot_pinned.h PIN_XYZZ, MSM_ARGS_MAX
// points): res_base runs over the MSM groups in launch order, and a member finds its own sums at res_off = res_base + its first
// operand.  The plan does not refuse a meeting whose sums run past the area: the launch does (run_msm_body, "result area
// overflow").
inline GangPlan gang_plan_meeting(const GangPlanReq* reqs, int count, uint32_t msm_cap, uint32_t ntt_cap) {
    GangPlan p;
    bool done[GANG_MAX] = {false, false, false, false};
    uint32_t res_base = 0;
    for (int i = 0; i < count; i++) {
        if (done[i] || reqs[i].kind == GANG_KIND_FLUSH) continue;
        const bool msm = reqs[i].kind == GANG_KIND_MSM;
        const uint32_t cap = msm ? msm_cap : ntt_cap;
        GangGroup g{};
        g.kind = reqs[i].kind;
        g.res_base = msm ? res_base : 0;
        for (int j = i; j < count; j++) {
            if (done[j] || reqs[j].kind != g.kind) continue;
            if (msm ? reqs[j].table != reqs[i].table : !(reqs[j].shape == reqs[i].shape)) continue;
            if (g.total + reqs[j].count > cap) continue;
            g.req[g.n] = j;
            g.first[g.n] = g.total;
            g.n++;
            g.total += reqs[j].count;
            done[j] = true;
        }
        if (!g.n) continue;     // (a request larger than the capacity by itself: nobody posts one)
        if (msm) res_base += g.total;
        p.group[p.groups++] = g;
    }
    return p;
}

// ---- the flush ----------------------------------------------------------------------------------------------------------------
// What makes the same step of two members one launch: the same kernel (the address of the function that launches it - one per
// functor, launch bound and argument list) with the same launch shape.  grid.z is the member index of a merged launch (only
// launches with grid.z == 1 are recorded), block.y / .z are 1 for every recorded kernel.
struct GangSig {
    bool some;                // false: this member has recorded fewer steps
    uintptr_t fn;
    uint32_t grid_x, grid_y, block_x, lds;
    bool operator==(const GangSig& o) const { return fn == o.fn && grid_x == o.grid_x && grid_y == o.grid_y && block_x == o.block_x && lds == o.lds; }
};
struct GangFlushStep {
    int groups = 0;
    int n[GANG_MAX];
    int member[GANG_MAX][GANG_MAX];    // group g launches step i of member[g][0..n[g]) at once, blockIdx.z = position in the group
};
// Step i of every member's recorded list (sigs[m]: member m's record i, or none), first fit in member order: instance i of every
// member in ONE launch when they are the same kernel with the same launch shape (they are: the members run the same prover over
// the same circuit), else one by one.  The caller walks i upwards and launches a step's groups before the next step's, so every
// member's records reach the stream in the order it made them; where members interleave differently from how they would have
// alone does not matter, since members never touch each other's buffers.
inline GangFlushStep gang_plan_flush_step(const GangSig* sigs, int count) {
    GangFlushStep s;
    bool done[GANG_MAX] = {false, false, false, false};
    for (int a = 0; a < count; a++) {
        if (done[a] || !sigs[a].some) continue;
        int& ng = s.n[s.groups];
        ng = 0;
        for (int b = a; b < count; b++) {
            if (done[b] || !sigs[b].some || !(sigs[b] == sigs[a])) continue;
            s.member[s.groups][ng++] = b;
            done[b] = true;
        }
        s.groups++;
    }
    return s;
}

}  // namespace apk

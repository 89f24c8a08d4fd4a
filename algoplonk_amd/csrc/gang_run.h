// The gang's runner: what of a gang (gang.h) touches HIP, beside the planner (gang_plan.h) and the kernel wrappers (gang_kernel.h)
// and free of the prover - no slot, no backend.  A gang member's element-wise / scan / reduction kernels are RECORDED between two
// meetings (GangRecorder) and go out at the next one, the same step of every member in ONE launch where gang_plan_flush_step says
// so (gang_flush).  MsmReq / NttReq are what a member posts at a commitment / transform batch: the backend's gang_launch plans
// the meeting from them and assembles the merged arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <new>
#include <vector>

#include "dev_buf.h"       // KCHK
#include "gang_kernel.h"
#include "gang_plan.h"
#include "msm_run.h"       // MsmTables, MsmBatchArgs
#include "ntt_plan.h"      // NTT_MAX_BATCH

namespace apk {

// a recorded launch: grid, block, the arguments by value
constexpr size_t CMD_BLOB = 1024;
struct Cmd {
    dim3 grid, block;
    uint32_t lds = 0;
    int (*multi)(hipStream_t, const Cmd* const*, int) = nullptr;   // launches this kernel for `count` recorded instances
    alignas(16) unsigned char blob[CMD_BLOB];                       // Pack<P...>: the instance's arguments
    GangSig sig() const { return GangSig{true, reinterpret_cast<uintptr_t>(multi), grid.x, grid.y, block.x, lds}; }
};

// ONE launch for `count` recorded instances of a kernel, blockIdx.z = instance (a recorded launch has grid.z == 1: a lone
// instance goes out with the grid it was recorded with)
template <class K, int BOUNDS, class... P>
int launch_multi(hipStream_t st, const Cmd* const* cmds, int count) {
    static_assert(sizeof(Pack<P...>) <= CMD_BLOB, "kernel arguments exceed a recorded launch's blob");
    static_assert(sizeof(GangPack<P...>) <= 4096, "a gang's arguments exceed the kernel argument segment");
    GangPack<P...> g{};
    for (int i = 0; i < count; i++) g.m[i] = *reinterpret_cast<const Pack<P...>*>(cmds[i]->blob);
    dim3 grid = cmds[0]->grid;
    grid.z = (uint32_t)count;
    polyG_kernel<K, BOUNDS, P...><<<grid, cmds[0]->block, cmds[0]->lds, st>>>(g);
    KCHK();
    return APK_OK;
}

// the launches a gang member has recorded since its last meeting
class GangRecorder {
  public:
    template <class K, int BOUNDS, class... P>
    void record(dim3 grid, dim3 block, size_t lds, P... p) {
        cmds_.emplace_back();
        Cmd& c = cmds_.back();
        c.grid = grid; c.block = block; c.lds = (uint32_t)lds;
        c.multi = &launch_multi<K, BOUNDS, P...>;
        new (c.blob) Pack<P...>(make_pack_impl(p...));
    }
    void clear() { cmds_.clear(); }
    size_t size() const { return cmds_.size(); }
    const Cmd& operator[](size_t i) const { return cmds_[i]; }

  private:
    std::vector<Cmd> cmds_;
};

// Launch what the members of a meeting have recorded on `st`, step by step as gang_plan_flush_step groups them, and forget it
// (after a failed launch too: nothing more is launched then).  *merged: launches that carried more than one member.
inline int gang_flush(GangRecorder* const* recs, int count, hipStream_t st, int* merged) {
    size_t longest = 0;
    for (int m = 0; m < count; m++) if (recs[m]->size() > longest) longest = recs[m]->size();
    int rc = APK_OK;
    for (size_t i = 0; i < longest && rc == APK_OK; i++) {
        GangSig sigs[GANG_MAX];
        for (int m = 0; m < count; m++) sigs[m] = i < recs[m]->size() ? (*recs[m])[i].sig() : GangSig{};
        const GangFlushStep s = gang_plan_flush_step(sigs, count);
        for (int g = 0; g < s.groups && rc == APK_OK; g++) {
            const Cmd* grp[GANG_MAX];
            for (int k = 0; k < s.n[g]; k++) grp[k] = &(*recs[s.member[g][k]])[i];
            rc = grp[0]->multi(st, grp, s.n[g]);
            if (s.n[g] > 1) ++*merged;
        }
    }
    for (int m = 0; m < count; m++) recs[m]->clear();
    return rc;
}

// ---- what a member posts at a merge point (GangReq::args) ----------------------------------------------------------------------
struct MsmReq {
    const MsmTables* T;
    MsmBatchArgs a;
    GangPlanReq plan_req() const { return GangPlanReq{GANG_KIND_MSM, a.batch, T, GangNttShape{}}; }
};
template <class Fr>
struct NttReq {
    int which; bool inverse; int count;
    const Fr* ins[NTT_MAX_BATCH]; Fr* outs[NTT_MAX_BATCH]; uint32_t in_lens[NTT_MAX_BATCH];
    uint32_t out_len; const Fr *pre, *post, *scale; int sub_log; bool semi;
    GangPlanReq plan_req() const { return GangPlanReq{GANG_KIND_NTT, (uint32_t)count, nullptr, GangNttShape{which, inverse, out_len, pre, post, scale, sub_log, semi}}; }
};

}  // namespace apk

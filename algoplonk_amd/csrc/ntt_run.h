// The NTT's runner: the knobs from the environment and the launches of one planned sequence, beside the kernels (kernels_ntt.h) and
// the planner (ntt_plan.h) and free of the prover - no slot, gang, gate or statistics.  The backend (backend_impl.h
// run_ntt_batch_now) picks the table and the workspace, plans the sequence and hands both to ntt_launch.
#pragma once
#include <hip/hip_runtime.h>

#include "backend.h"
#include "dev_buf.h"
#include "kernels_ntt.h"
#include "ntt_plan.h"

namespace apk {

// The NTT's knobs (ntt_plan.h: NttKnobs, with what each one does and why its default is what it is), from the environment:
// latched at the first transform of the process.
inline const NttKnobs& ntt_knobs() {
    static const NttKnobs k = [] {
        NttKnobs e;
        e.tile_log = env_int("APK_NTT_TILE_LOG", 0, 0, NTT_TILE_LOG);
        e.stages = env_int("APK_NTT_STAGES", 0, 0, NTT_TILE_LOG);
        e.radix4 = env_int("APK_NTT_RADIX4", -1, -1, 1);
        e.threads = env_int("APK_NTT_THREADS", 0, 0, NTT_THREADS) & ~63;   // whole waves, <= the launch bound
        return e;
    }();
    return k;
}

// the pass kernels' dynamic LDS above the 64 KiB a kernel gets unasked: the largest tile
template <class FRP>
int ntt_allow_tile_lds() {
    const int lds = (int)(((size_t)1 << NTT_TILE_LOG) * sizeof(FeU<FRP>));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ntt_pass_kernel<FRP, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ntt_pass_kernel<FRP, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return APK_OK;
}

// The passes of a planned sequence of `count` transforms, on `st`.  twu: `tw` holds FeU records (ntt_pass_kernel<.., TWU>).
template <class FRP>
int ntt_launch(hipStream_t st, const NttPlan& plan, const NttBatch& nb, int count, const Fe<FRP>* tw, bool twu, const Fe<FRP>* pre,
               const Fe<FRP>* post, const Fe<FRP>* scale) {
    const dim3 grid(plan.grid_x, count);
    for (int p = 0; p < plan.passes; p++) {
        if (twu) ntt_pass_kernel<FRP, true><<<grid, plan.threads, plan.lds_bytes, st>>>(nb, tw, pre, post, scale, plan.pass[p]);
        else ntt_pass_kernel<FRP, false><<<grid, plan.threads, plan.lds_bytes, st>>>(nb, tw, pre, post, scale, plan.pass[p]);
        KCHK();
    }
    return APK_OK;
}

}  // namespace apk

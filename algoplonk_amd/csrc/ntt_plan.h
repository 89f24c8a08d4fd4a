// The NTT's planner: every decision about one launch sequence of same-size transforms - the tile, the stages of every pass, radix 4,
// the lanes per workgroup, the grid and the LDS - and the path counters it bumps.  Plain integer arithmetic: no HIP include, no
// device, builds with `g++ -std=c++17` - tools/ntt_plan_dump.cpp prints its plans and tests/test_ntt_model.py holds the Python model
// (tests/ntt_model.py) to them on the CPU.  GPU-free like msm_plan.h.
//
// ntt_run.h fills NttKnobs from the environment and launches what a plan says; the backend (backend_impl.h run_ntt_batch_now) picks
// the table and the workspace and asks for the plan.  The rules and the measurements behind their defaults live here, each in ONE
// place.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "../../include/apk.h"

namespace apk {

// ---- constants (the kernels of kernels_ntt.h read the same ones) --------------------------------------------------------------
constexpr int NTT_TILE_LOG = 11;     // largest tile a workgroup may hold: 2^11 elements of 36 bytes (FeU) = 72 KiB of LDS; what a
                                     // transform takes is the plan's tile_log (2^9 or 2^10 by rule)
constexpr int NTT_THREADS = 256;     // lanes per workgroup: the pass kernel's launch bound
// up to NTT_MAX_BATCH same-size transforms per launch (blockIdx.y): the three wire polynomials share launches,
// which triples the workgroup count of these latency-bound small transforms
constexpr int NTT_MAX_BATCH = 4;     // ... of ONE proof
constexpr int NTT_ARGS_MAX = 16;     // ... per launch: a gang of up to four proofs shares its launches (gang.h)
constexpr int NTT_LOG_MAX = 29;      // largest transform whose passes hand each other elements through a workspace
constexpr int NTT_PASSES_MAX = NTT_LOG_MAX;   // one stage per pass (APK_NTT_STAGES=1) at the largest size

struct NttPassArgs {
    int log_n;
    int tile_log;        // log2(elements per workgroup tile)
    int t0, t1;          // stages [t0, t1)
    int first, last;     // first pass gathers bit-reversed + pre-multiplies; last pass post-multiplies
    uint32_t out_len;    // last pass: elements >= out_len are not written
    int radix4;          // two stages per LDS round trip (large transforms; see the kernel)
    int tw_shift;        // the twiddle table belongs to a transform 2^tw_shift times this size (sub-coset transforms: tw[j << tw_shift])
    int semi;            // last pass without post / scale: outputs only below 2r (same residues), for readers that unpack them into
                         // lazy limbs anyway (the quotient kernel); 0 = canonical
};

// ---- knobs: one field per APK_NTT_* environment variable the plan reads (filled by ntt_knobs in ntt_run.h, once per process) ---
// (APK_NTT_TWU is not among them: it chooses how a context's twiddle TABLES are built, and is read where they are)
struct NttKnobs {
    // small transforms are latency-bound: 512-element tiles (18 KiB LDS) give >= 256 workgroups at 2^17.  Large ones were
    // assumed bandwidth-bound (2048-element tiles, fewest passes) until round 3 measured them: at 2^21 / 2^23 the 72 KiB tile
    // leaves two workgroups = 2 waves per SIMD on a CU, the pass runs at 6.9 cycles per VALU instruction and 1.9 TB/s - bound
    // by neither (profiles/r03_pmc_bls12381_2p21_*).  1024-element tiles (36 KiB, 4 workgroups per CU), 9 stages per pass:
    // 6.84 instead of 8.65 ms of NTT per BLS12-381 2^21 proof; 512 / 7 is the same, 2048 with 8..10 stages all 8.6 ms.
    int tile_log = 0;    // APK_NTT_TILE_LOG: 0 = the rule (9 up to 2^19, 10 above), else up to NTT_TILE_LOG - what the LDS tile holds
    int stages = 0;      // APK_NTT_STAGES: 0 = the rule (7 up to 2^19, 9 above), else the most stages per pass
    // radix 4 (two stages per LDS round trip, one four-element group per lane and step) pays above 2^19 only: kernels_ntt.h
    // ... and, with other proofs in flight, from 2^17 up: the instruction saving shows there (BN254 2^17, same box,
    // under the round-4 wave priorities: 508.6 -> 513.7 proofs/s) while a lone proof's latency-bound launches would lose
    // ~0.6 % to the halved lane count.
    int radix4 = -1;     // APK_NTT_RADIX4: -1 = that rule, 0 never, 1 always
    int threads = 0;     // APK_NTT_THREADS: 0 = the rule (NTT_THREADS; with radix 4 a lane per four-element group), else the lanes
                         // per workgroup - whole waves, at most NTT_THREADS
};

// ---- the plan of one launch sequence ------------------------------------------------------------------------------------------
// path counters a sequence bumps (backend_impl.h maps them to its P_* indices)
enum NttPathBit : uint32_t { NTT_PATH_SEQ = 1u << 0, NTT_PATH_R4 = 1u << 1, NTT_PATH_R4_LOAD = 1u << 2, NTT_PATH_DEVICE_LOAD = 1u << 3 };
struct NttPlanIn {
    int log_n;               // log2 of the transform
    int count;               // same-size transforms in the sequence (blockIdx.y)
    uint32_t out_len;        // NttPassArgs::out_len
    int tw_shift;            // NttPassArgs::tw_shift
    bool semi;               // NttPassArgs::semi
    uint32_t fe_u_bytes;     // size of a tile element (FeU: 36 bytes for both scalar fields)
    bool have_wide;          // the stream has a workspace for what the passes hand each other
    bool loaded, loaded_foreign;   // other proofs keep the GPU busy (asked only where ntt_plan_reads_load says); and not this context's own
};
struct NttPlan {
    int rc = APK_OK;
    char message[64] = {0};  // the refusal, when rc != APK_OK
    int passes = 0;
    NttPassArgs pass[NTT_PASSES_MAX];   // [passes]
    uint32_t grid_x = 0;     // workgroups per transform
    uint32_t threads = 0;    // lanes per workgroup
    size_t lds_bytes = 0;    // the tile
    bool needs_wide = false; // more than one pass: they hand each other unsaturated-limb elements through the workspace
    uint32_t paths = 0;      // NttPathBit set
};

// The sizes whose radix-4 choice follows the load: the only ones a caller needs the device's load figure for.
inline bool ntt_plan_reads_load(int log_n) { return log_n >= 17 && log_n <= 19; }

inline NttPlan ntt_plan(const NttKnobs& k, const NttPlanIn& in) {
    NttPlan p;
    if (in.count < 1 || in.count > NTT_ARGS_MAX) {
        p.rc = APK_ERR_ARG;
        snprintf(p.message, sizeof p.message, "ntt: batch of %d", in.count);
        return p;
    }
    const int log_n = in.log_n;
    int tile_log = log_n <= 19 ? 9 : 10;     // (NttKnobs::tile_log has the measurements)
    int max_s = log_n <= 19 ? 7 : 9;
    if (k.tile_log) tile_log = k.tile_log;
    if (k.stages) max_s = k.stages;
    if (tile_log > log_n) tile_log = log_n;
    if (max_s > tile_log) max_s = tile_log;
    p.passes = (log_n + max_s - 1) / max_s;
    p.needs_wide = p.passes > 1;
    if (p.needs_wide && (!in.have_wide || log_n > NTT_LOG_MAX)) {
        p.rc = APK_ERR_STATE;
        snprintf(p.message, sizeof p.message, "ntt: no workspace for this stream");
        return p;
    }
    const int radix4 = k.radix4 >= 0 ? k.radix4 : (log_n > 19 || (log_n >= 17 && in.loaded) ? 1 : 0);   // (NttKnobs::radix4)
    p.paths = NTT_PATH_SEQ;
    if (radix4) {
        p.paths |= NTT_PATH_R4;
        if (k.radix4 < 0 && log_n <= 19) { p.paths |= NTT_PATH_R4_LOAD; if (in.loaded_foreign) p.paths |= NTT_PATH_DEVICE_LOAD; }
    }
    p.threads = NTT_THREADS;
    if (radix4) {
        p.threads = (1u << tile_log) / 4;
        if (p.threads < 64) p.threads = 64;
        if (p.threads > (uint32_t)NTT_THREADS) p.threads = NTT_THREADS;
    }
    if (k.threads) p.threads = (uint32_t)k.threads;
    p.grid_x = 1u << (log_n - tile_log);
    p.lds_bytes = ((size_t)1 << tile_log) * in.fe_u_bytes;
    int t0 = 0;
    for (int i = 0; i < p.passes; i++) {     // the stages that are left, spread evenly over the passes that are left
        const int s = (log_n - t0 + (p.passes - i) - 1) / (p.passes - i);
        NttPassArgs& a = p.pass[i];
        a.log_n = log_n; a.tile_log = tile_log; a.t0 = t0; a.t1 = t0 + s;
        a.first = (i == 0); a.last = (i == p.passes - 1);
        a.out_len = in.out_len;
        a.radix4 = radix4;
        a.tw_shift = in.tw_shift;
        a.semi = in.semi ? 1 : 0;
        t0 += s;
    }
    return p;
}

}  // namespace apk

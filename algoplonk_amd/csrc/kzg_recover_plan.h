// The planner of apk_kzg_recover_cosets (include/apk.h): the polynomial back from any sufficient set of its cells.  Everything
// here is plain integer bookkeeping: no HIP include, no device, builds with `g++ -std=c++17` - tools/kzg_recover_plan_dump.cpp
// prints its answers and tests/test_kzg_recover_host.py holds them to a Python restatement on the CPU.  GPU-free like
// kzg_fk20_plan.h, msm_plan.h, ntt_plan.h and gang_plan.h.
//
// The runner (kzg_recover_run.h) launches what recover_plan says, the backend (backend_impl.h kzg_recover_cosets) and the host
// form (kzg_recover_host.h) refuse what it refuses.  A mistake in these rules returns a wrong polynomial with APK_OK: they stand
// here, each in ONE place.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../include/apk.h"

namespace apk {

constexpr uint32_t KZG_RECOVER_THREADS = 256;    // lanes per workgroup of every launch
constexpr uint32_t KZG_RECOVER_TILE = 256;       // roots a workgroup of the vanish kernel stages in LDS at a time
constexpr uint32_t KZG_RECOVER_FR_BYTES = 32;    // a scalar of either curve

struct RecoverVerdict {
    int rc = APK_OK;
    char message[160] = {0};     // the refusal, when rc != APK_OK
};

// ---- the rules that need no domain: what the C-ABI checks before it looks for a device -------------------------------------------
inline RecoverVerdict recover_check_call(uint32_t l, uint32_t count, uint64_t len) {
    RecoverVerdict v;
    if (count == 0 || len == 0) {
        v.rc = APK_ERR_ARG;
        snprintf(v.message, sizeof v.message, "kzg: recovery from %u cells of a polynomial of %llu coefficients", count, (unsigned long long)len);
    } else if (l < 2 || (l & (l - 1))) {
        v.rc = APK_ERR_ARG;
        snprintf(v.message, sizeof v.message, "kzg: cosets of %u points (a power of two, at least 2)", l);
    }
    return v;
}

// ---- a launch ------------------------------------------------------------------------------------------------------------------
struct RecoverLaunch {
    uint32_t lanes = 0, grid = 0, block = KZG_RECOVER_THREADS, lds_bytes = 0;
};
inline RecoverLaunch recover_launch(uint32_t lanes, uint32_t lds_bytes) {
    RecoverLaunch L;
    L.lanes = lanes;
    L.grid = (lanes + KZG_RECOVER_THREADS - 1) / KZG_RECOVER_THREADS;
    L.lds_bytes = lds_bytes;
    return L;
}

// ---- the plan of one call ------------------------------------------------------------------------------------------------------
// n points in the domain (a power of two), cosets of l points, n' = n / l of them; k = count known ones, m = n' - k missing.
//   row_of[i]   the row of `values` that holds coset i, or -1                                            (n' entries)
//   missing     the m coset indices that have no row, ascending: the roots a_i = w^(i l) of Z             (m entries)
//   vanish      2n' lanes (zH, then zG), the roots through LDS in `tiles` tiles of KZG_RECOVER_TILE
//   scatter     n lanes;  divide  n lanes
//   check_lo .. check_hi   the coefficients that must be zero: [len, k l)  (empty when len = k l)
struct RecoverPlan {
    RecoverVerdict verdict;
    uint32_t n = 0, l = 0, np = 0, k = 0, m = 0;
    int log_n = 0, log_l = 0, log_np = 0;
    std::vector<int32_t> row_of;
    std::vector<uint32_t> missing;
    RecoverLaunch vanish, scatter, divide;
    uint32_t tiles = 0;
    uint64_t check_lo = 0, check_hi = 0;
};

// The rules in the order of include/apk.h; recover_check_call has passed.
inline RecoverPlan recover_plan(uint64_t n64, uint32_t l, uint32_t count, const uint64_t* indices, uint64_t len) {
    RecoverPlan p;
    RecoverVerdict& v = p.verdict;
    auto refuse = [&](void) -> RecoverPlan& { v.rc = APK_ERR_ARG; return p; };
    if (l > n64 / 2) {
        snprintf(v.message, sizeof v.message, "kzg: cosets of %u points in a domain of %llu (a power of two, 2..n/2)", l, (unsigned long long)n64);
        return refuse();
    }
    p.n = (uint32_t)n64; p.l = l;
    p.log_n = __builtin_ctzll(n64); p.log_l = __builtin_ctz(l); p.log_np = p.log_n - p.log_l;
    p.np = p.n >> p.log_l;
    if (count > p.np) {
        snprintf(v.message, sizeof v.message, "kzg: %u cells, the domain of %u points has %u cosets of %u", count, p.n, p.np, l);
        return refuse();
    }
    for (uint32_t r = 0; r < count; r++)
        if (indices[r] >= p.np) {
            snprintf(v.message, sizeof v.message, "kzg: cell %u is coset %llu of %u", r, (unsigned long long)indices[r], p.np);
            return refuse();
        }
    p.row_of.assign(p.np, -1);
    for (uint32_t r = 0; r < count; r++) {
        int32_t& slot = p.row_of[indices[r]];
        if (slot >= 0) {
            snprintf(v.message, sizeof v.message, "kzg: cells %d and %u are both coset %llu", slot, r, (unsigned long long)indices[r]);
            p.row_of.clear();
            return refuse();
        }
        slot = (int32_t)r;
    }
    if (len > (uint64_t)count * l) {
        snprintf(v.message, sizeof v.message, "kzg: too few cells: %llu coefficients need %llu cells of %u points, %u given", (unsigned long long)len,
                 (unsigned long long)((len + l - 1) / l), l, count);
        p.row_of.clear();
        return refuse();
    }
    if (p.np > APK_KZG_RECOVER_MAX_COSETS) {
        snprintf(v.message, sizeof v.message, "kzg: %u cosets, recovery takes at most %u", p.np, (unsigned)APK_KZG_RECOVER_MAX_COSETS);
        p.row_of.clear();
        return refuse();
    }
    p.k = count; p.m = p.np - count;
    p.missing.reserve(p.m);
    for (uint32_t i = 0; i < p.np; i++)
        if (p.row_of[i] < 0) p.missing.push_back(i);
    p.tiles = (p.m + KZG_RECOVER_TILE - 1) / KZG_RECOVER_TILE;
    p.vanish = recover_launch(2 * p.np, KZG_RECOVER_TILE * KZG_RECOVER_FR_BYTES);
    p.scatter = recover_launch(p.n, 0);
    p.divide = recover_launch(p.n, 0);
    p.check_lo = len; p.check_hi = (uint64_t)count * l;
    return p;
}

}  // namespace apk

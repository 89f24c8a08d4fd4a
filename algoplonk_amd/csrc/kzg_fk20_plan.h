// The planner of the FK20 openings - apk_kzg_open_all (every point of the domain) and apk_kzg_open_cosets (every coset of l
// points) - which are ONE computation: the whole-domain call is the cosets call at l = 1.  Everything here is plain integer
// bookkeeping: no HIP include, no device, builds with `g++ -std=c++17` - tools/kzg_fk20_plan_dump.cpp prints its answers and
// tests/test_kzg_fk20_plan.py holds them to the big-integer models (tests/kzg_all_model.py, tests/kzg_cosets_model.py) on the CPU.
// GPU-free like msm_plan.h, ntt_plan.h and gang_plan.h.
//
// The runners (kzg_all_run.h, kzg_cosets_run.h) launch what fk20_gather says; the backend (backend_impl.h kzg_fk20_*) fills t
// from fk20_t_source, refuses what the fk20_check_* rules refuse and splits the small NTTs as fk20_chunk says.  A mistake in these
// rules returns wrong proofs with APK_OK: they stand here, each in ONE place.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "../../include/apk.h"
#include "ntt_plan.h"      // NTT_ARGS_MAX

namespace apk {

// ---- the shape ----------------------------------------------------------------------------------------------------------------
// n points in the domain, cosets of l points (l = 1: the whole-domain call), n' = n / l proofs.  The convolution behind the proofs
// has size 2n' (kernels_kzg_all.h, kernels_kzg_cosets.h): l of them side by side in the prepare call, one in every open call.
struct Fk20Shape {
    uint32_t n, l, np;
    int log_n, log_l, log_np;
    uint32_t pair_big() const { return 2 * np; }          // the transform pair of an open call: inverse over 2n' points ...
    uint32_t pair_small() const { return np; }            // ... then forward over n'
    int prepare_stages() const { return log_np + 1; }     // the stages the prepare call runs over its 2n-point array: log 2n'
    int sub_log() const { return log_l; }                 // the small NTTs are size-n' transforms on the size-n table (run_ntt_batch)
};
inline Fk20Shape fk20_shape(int log_n, uint32_t l) {
    Fk20Shape s{};
    s.log_n = log_n; s.n = 1u << log_n;
    s.l = l; s.log_l = __builtin_ctz(l);
    s.np = s.n >> s.log_l; s.log_np = log_n - s.log_l;
    return s;
}

// ---- the argument rules that depend on (n, l, count, len) alone -------------------------------------------------------------------
// (the state of the context - MSM-only, prepared, "one coset size per context", device memory - is the backend's to check)
struct Fk20Verdict {
    int rc = APK_OK;
    char message[160] = {0};     // the refusal, when rc != APK_OK
};
// apk_kzg_cosets_prepare: l a power of two in 2 .. n / 2
inline Fk20Verdict fk20_check_coset_size(uint32_t n, uint32_t l) {
    Fk20Verdict v;
    if (l < 2 || (l & (l - 1)) || l > n / 2) {
        v.rc = APK_ERR_ARG;
        snprintf(v.message, sizeof v.message, "kzg: cosets of %u points in a domain of %u (a power of two, 2..n/2)", l, n);
    }
    return v;
}
// both prepare calls: the highest SRS index used is n - l - 1 (fk20_t_source), so count >= n - l
inline Fk20Verdict fk20_check_srs(uint32_t n, uint32_t l, uint64_t count) {
    Fk20Verdict v;
    if (count >= (uint64_t)n - l) return v;
    v.rc = APK_ERR_ARG;
    if (l == 1) snprintf(v.message, sizeof v.message, "kzg: %llu SRS points, the openings at every point need %u", (unsigned long long)count, n - 1);
    else snprintf(v.message, sizeof v.message, "kzg: %llu SRS points, the openings on cosets of %u points need %u", (unsigned long long)count, l, n - l);
    return v;
}
// both open calls: 1 <= len <= n
inline Fk20Verdict fk20_check_len(uint32_t n, uint32_t l, uint64_t len) {
    Fk20Verdict v;
    if (len >= 1 && len <= n) return v;
    v.rc = APK_ERR_ARG;
    snprintf(v.message, sizeof v.message, "kzg: %llu coefficients, the openings %s take 1..%u", (unsigned long long)len, l == 1 ? "at every point" : "on every coset", n);
    return v;
}
// deg f < l: f is its own remainder on every coset (l = 1: a constant), every quotient the zero polynomial, every H infinity
inline bool fk20_has_quotient(const Fk20Shape& s, uint64_t len) { return len > s.l; }

// ---- the source of t ----------------------------------------------------------------------------------------------------------
// The prepare call transforms 2n affine points t with t[c + l u] = t_c[u], u < 2n':
//     t_c = (s_(c+l(n'-2)) .. s_(c+l), s_c, infinity x (n'+1))
// so position c + l u holds SRS point c + l (n' - 2 - u) for u <= n' - 2 and infinity behind.  At l = 1 this is
// t = (s_(n-2) .. s_0, infinity x (n+1)).  The SRS index for a position < 2n, or FK20_T_INFINITY.
constexpr int64_t FK20_T_INFINITY = -1;
inline int64_t fk20_t_source(const Fk20Shape& s, uint32_t pos) {
    const uint32_t c = pos & (s.l - 1), u = pos >> s.log_l;
    return u + 1 < s.np ? (int64_t)c + (int64_t)s.l * (s.np - 2 - u) : FK20_T_INFINITY;
}

// ---- the gather ---------------------------------------------------------------------------------------------------------------
// kzg_all_gather_kernel over m points: lane k of a launch (k0, k1) reads c[k + m - 2] and writes the bit-reversed position of k
// among the first m points of the SAME array (infinity at k = m - 1, which reads nothing).  The lanes of a launch run in no order,
// so no launch may write what another of its lanes reads:
//   lanes 0 and 1 read m - 2 and m - 1, BELOW m, and write 0 and m / 2; lanes 2 .. m-1 read m .. 2m - 4 and write below m.  So
//   (0,2) goes before (2,m) moves anything into the first m points, and from m = 8 on (m / 2 < m - 2) neither reads what it writes.
//   m = 4: lane 1 writes position 2 = m - 2, which lane 0 reads: the two go one after the other.
//   m = 2: lane 0 reads and writes position 0, lane 1 writes infinity to position 1 = m - 1; nothing is left for a second launch.
struct Fk20Range { uint32_t k0, k1; };
struct Fk20Gather {
    int count = 0;
    Fk20Range launch[3];
};
inline Fk20Gather fk20_gather(uint32_t m) {
    Fk20Gather g;
    if (m == 4) {
        g.launch[g.count++] = {0, 1};
        g.launch[g.count++] = {1, 2};
    } else {
        g.launch[g.count++] = {0, 2};
    }
    if (m > 2) g.launch[g.count++] = {2, m};
    return g;
}

// ---- the chunks of the small NTTs -----------------------------------------------------------------------------------------------
// An open call on cosets transforms 2l sequences of n' scalars - the even half of every A^_c, then the odd half - at most
// NTT_ARGS_MAX per launch sequence: chunk i < fk20_chunks(l) covers the sequences c0 .. c0 + cnt - 1 of one parity.
struct Fk20Chunk { int odd; uint32_t c0; int cnt; };
inline uint32_t fk20_chunks(uint32_t l) { return 2 * ((l + NTT_ARGS_MAX - 1) / NTT_ARGS_MAX); }
inline Fk20Chunk fk20_chunk(uint32_t l, uint32_t i) {
    const uint32_t per = fk20_chunks(l) / 2, c0 = (i % per) * NTT_ARGS_MAX;
    return Fk20Chunk{(int)(i / per), c0, (int)(l - c0 < (uint32_t)NTT_ARGS_MAX ? l - c0 : (uint32_t)NTT_ARGS_MAX)};
}

}  // namespace apk

// The planner of the FK20 openings - apk_kzg_open_all (every point of the domain) and apk_kzg_open_cosets (every coset of l
// points) - which are ONE computation: the whole-domain call is the cosets call at l = 1; and of apk_kzg_open_cosets_multi, many
// polynomials on every coset in one call (groups, layout, scratch, grids and argument rules).  Everything here is plain integer
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
// (the batched call below transforms 2 G l sequences: the same two functions over G l rows in place of l)

// ---- the lanes of the pointwise sums -------------------------------------------------------------------------------------------
// kzg_cosets_pointwise_kernel: min(4 l, 64) lanes serve one output, a workgroup of one wave 64 >> log_group outputs
constexpr uint32_t FK20_POINTWISE_THREADS = 64;      // KZG_COSETS_THREADS
inline int fk20_pointwise_log_group(int log_l) { return log_l + 2 < 6 ? log_l + 2 : 6; }
inline uint32_t fk20_pointwise_blocks(const Fk20Shape& s) {
    const uint32_t per = FK20_POINTWISE_THREADS >> fk20_pointwise_log_group(s.log_l);
    return (s.pair_big() + per - 1) / per;
}

// ---- MANY polynomials on every coset in one call (apk_kzg_open_cosets_multi; kzg_cosets_multi_run.h) ------------------------------
// GROUPS.  A call of `count` polynomials runs cdiv(count, NTT_ARGS_MAX) groups one after another on the slot's stream; their sizes
// differ by at most one, the larger first (17 = 9 + 8, not 16 + 1: a group of one pays every stage launch for one polynomial).
// G <= NTT_ARGS_MAX keeps the G size-n value transforms of a group in one run_ntt_batch launch sequence.
constexpr uint32_t FK20_MULTI_MAX = APK_KZG_COSETS_MULTI_MAX;
constexpr uint32_t FK20_GROUP_MAX = NTT_ARGS_MAX;
struct Fk20Group { uint32_t b0, size; };      // the polynomials b0 .. b0 + size - 1 of the call
inline uint32_t fk20_multi_groups(uint32_t count) { return (count + FK20_GROUP_MAX - 1) / FK20_GROUP_MAX; }
inline Fk20Group fk20_multi_group(uint32_t count, uint32_t g) {
    const uint32_t groups = fk20_multi_groups(count), base = count / groups, extra = count % groups;
    return Fk20Group{g * base + (g < extra ? g : extra), base + (g < extra ? 1u : 0u)};
}
inline uint32_t fk20_multi_largest_group(uint32_t count) { return fk20_multi_group(count, 0).size; }

// INFINITY ROWS.  A polynomial with len <= l (fk20_has_quotient false) GOES THROUGH every step like its neighbours: its gathered
// sequences are all zero, a zero scalar has no set bit, infinity in gives infinity out of every butterfly, and the finish writes
// (0, 0) - the zeros the single call writes.  No row of a group is special, so no launch depends on the lengths.
constexpr bool FK20_MULTI_SKIPS_INFINITY_ROWS = false;

// LAYOUT of a group of G polynomials b < G, with c < l, u and i < n', j < l, k < 2n'.  Scalars in units of one Fr, points in units of
// one XYZZ point; every area starts at 0 of its own array.
//   values        NTT_n(f_b) at                     b n + .
//   by_coset      the same coset-major at           b n + i l + j
//   rows          the gathered sequences a_(b,c) and both halves of A^_(b,c): row (b l + c) of n' scalars = b n + c n' + u
//   work          G blocks of 2n' points:           P^_b[i] at b 2n' + brev_{log 2n'}(i); after the inverse stages cc_b[k] at b 2n' + k
//   second        G blocks of n' points, OUT OF PLACE: second[b n' + brev_{log n'}(k)] = cc_b[k + n' - 2], infinity at k = n' - 1;
//                 after the forward stages H_(b,i) at b n' + i
//   result        the affine H_(b,i) at             b n' + i
// The single call gathers in place, with launch-order rules at m = 2, 4 and >= 8 (fk20_gather); side by side block b's destination
// would overlap block b / 2's source.  The second array removes the hazard: ONE launch of G n' lanes, none reading what another writes.
// Both stage kernels pair (i, i + 2^t) inside aligned blocks of 2^(t+1) <= 2n' (n') points and take the twiddle from i mod 2^t: with
// contiguous blocks of 2n' (n') points no butterfly crosses a polynomial, whatever G.
constexpr int64_t FK20_GATHER_INFINITY = -1;
inline uint32_t fk20_brev(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}
struct Fk20Multi {
    Fk20Shape s;
    uint32_t G;
    // scalars
    size_t value(uint32_t b, uint32_t k) const { return (size_t)b * s.n + k; }
    size_t by_coset(uint32_t b, uint32_t i, uint32_t j) const { return (size_t)b * s.n + (size_t)i * s.l + j; }
    size_t row(uint32_t b, uint32_t c) const { return (size_t)b * s.l + c; }                       // x n' scalars
    uint32_t rows() const { return G * s.l; }                                                      // of one parity: fk20_chunk(rows(), .)
    // points
    size_t work_hat(uint32_t b, uint32_t i) const { return (size_t)b * s.pair_big() + fk20_brev(i, s.log_np + 1); }
    size_t work_cc(uint32_t b, uint32_t k) const { return (size_t)b * s.pair_big() + k; }
    size_t second_at(uint32_t b, uint32_t k) const { return (size_t)b * s.np + fk20_brev(k, s.log_np); }
    int64_t gather_source(uint32_t b, uint32_t k) const { return k + 1 == s.np ? FK20_GATHER_INFINITY : (int64_t)work_cc(b, k + s.np - 2); }
    size_t result(uint32_t b, uint32_t i) const { return (size_t)b * s.np + i; }
    // the transforms in the exponent: kzg_all_stages(work, big_points(), log 2n') then (second, small_points(), log n')
    uint32_t big_points() const { return G * s.pair_big(); }
    uint32_t small_points() const { return G * s.pair_small(); }
    // SCRATCH of a slot, for its largest group so far: 3 G n' points (second, then work; the affine results go where work was) and
    // 5 G n scalars (rows, even halves, odd halves, values, by_coset), and G n more for the host form's uploads: scratch_in holds ONE vector
    size_t scratch_points() const { return (size_t)3 * G * s.np; }
    size_t scratch_scalars() const { return (size_t)5 * G * s.n; }
    size_t upload_scalars() const { return (size_t)G * s.n; }
    // GRIDS (workgroups; the lanes per workgroup are the kernels' launch bounds)
    uint32_t grid_scalars() const { return (G * s.n + 255) / 256; }                   // values and split: G n lanes, 256 per workgroup
    uint32_t grid_pointwise_x() const { return fk20_pointwise_blocks(s); }            // the single kernel's grid ...
    uint32_t grid_pointwise_y() const { return G; }                                   // ... x G in blockIdx.y
    uint32_t grid_points() const { return (G * s.np + 127) / 128; }                   // gather, finish, a stage over 2 G n' points (KZG_ALL_THREADS)
    uint32_t grid_small_stage() const { return (G * s.np / 2 + 127) / 128; }          // a stage over G n' points
};
inline Fk20Multi fk20_multi(int log_n, uint32_t l, uint32_t G) { return Fk20Multi{fk20_shape(log_n, l), G}; }

// THE ARGUMENT RULES, in their order; the message names the offending row where there is one.  prepared_l: the coset size the
// context is prepared for, 0 = apk_kzg_cosets_prepare has not run.  (Rule 6 - in the device form a polys[b] that is not device
// memory - needs the runtime and is the backend's; fk20_multi_not_device words it.)
inline Fk20Verdict fk20_multi_check(bool msm_only, uint32_t prepared_l, uint32_t n, uint32_t count, const void* const* polys, const uint64_t* lens,
                                    const void* out_h) {
    Fk20Verdict v;
    if (msm_only) { v.rc = APK_ERR_STATE; snprintf(v.message, sizeof v.message, "MSM-only context has no NTT domain"); return v; }                  // 1
    if (!prepared_l) { v.rc = APK_ERR_STATE; snprintf(v.message, sizeof v.message, "kzg: apk_kzg_cosets_prepare has not run on this context"); return v; }   // 2
    v.rc = APK_ERR_ARG;
    if (count == 0 || count > FK20_MULTI_MAX) { snprintf(v.message, sizeof v.message, "kzg: %u polynomials on every coset (1..%u)", count, FK20_MULTI_MAX); return v; }   // 3
    if (!polys || !lens || !out_h) { snprintf(v.message, sizeof v.message, "null argument"); return v; }                                            // 4
    for (uint32_t b = 0; b < count; b++)
        if (!polys[b]) { snprintf(v.message, sizeof v.message, "kzg: polynomial %u is null", b); return v; }
    for (uint32_t b = 0; b < count; b++) {                                                                                                           // 5
        const Fk20Verdict r = fk20_check_len(n, prepared_l, lens[b]);
        if (r.rc != APK_OK) { snprintf(v.message, sizeof v.message, "polynomial %u: %.140s", b, r.message); return v; }
    }
    // (not one of the call's rules, a limit of the lane indices: a group's 2 G n' points and G n scalars are counted in 32 bits)
    if ((uint64_t)fk20_multi_largest_group(count) * n >= (1ull << 32)) { snprintf(v.message, sizeof v.message, "kzg: groups of %u polynomials of %u coefficients", fk20_multi_largest_group(count), n); return v; }
    v.rc = APK_OK;
    return v;
}
inline Fk20Verdict fk20_multi_not_device(uint32_t b) {                                                                                               // 6
    Fk20Verdict v;
    v.rc = APK_ERR_ARG;
    snprintf(v.message, sizeof v.message, "kzg: polynomial %u is not device memory", b);
    return v;
}

}  // namespace apk

// KZG opening kernels (kzg.Open, kzg.BatchOpenSinglePoint) in their general-length, table-free
// form: any number of coefficients, any point, no table of powers of the point.  The prover's own openings (backend_impl.h
// round 4) keep their fused form over the power tables it needs anyway.
//
// One suffix-Horner pass gives the quotient AND the value:  S_j = sum_{m >= j} g_m z^(m - j)  is  q_(j-1)  for j >= 1 (the
// coefficients of (g(X) - g(z)) / (X - z)) and  g(z)  for j = 0 - the remainder of the division is the value.
//
// Lane map: lane t of workgroup b owns the KZG_LANE_CHUNK consecutive coefficients from b * KZG_BLOCK_SPAN + t * KZG_LANE_CHUNK.
//   1. KzgFoldBlockK   g_m = sum_i coef_i f_i[m] (shorter polynomials zero-extended; the fold is never written out), Horner over
//                      the lane's chunk, a suffix scan of the lane totals with the constant multiplier z^KZG_LANE_CHUNK through
//                      LDS, the workgroup-local S_j to q[j - 1], the workgroup's total to tot[b]
//   2. KzgCarryK       one workgroup: tot[b] <- carry into workgroup b = sum_{c > b} tot[c] z^(KZG_BLOCK_SPAN (c - b - 1)), in
//                      place; what is left over at the front is S_0 = g(z)
//   3. KzgApplyK       q[j - 1] += z^(end of j's workgroup - j) * carry; the lane raises z to the power of its first element by
//                      square-and-multiply and walks on from there
// Batch evaluation is launch 1 without the quotient (KzgEvalBlockK, blockIdx.y = polynomial) and launch 2 with one workgroup
// per polynomial.  Openings at several points (KzgGroup*K at the end of this file) are the three launches with the row - one
// polynomial at its own point - as a grid dimension.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ff.h"
#include "ffu.h"

namespace apk {

constexpr int KZG_THREADS = 256;
constexpr int KZG_LANE_CHUNK = 8;                              // coefficients per lane
constexpr int KZG_BLOCK_SPAN = KZG_THREADS * KZG_LANE_CHUNK;   // coefficients per workgroup
constexpr int KZG_MAX_POLYS = 32;                              // = APK_KZG_MAX_POLYS

template <class FR>
struct KzgPolys {
    const Fe<FR>* f[KZG_MAX_POLYS];
    uint32_t len[KZG_MAX_POLYS];
    Fe<FR> coef[KZG_MAX_POLYS];   // the fold's weights gamma^i (coef[0] is not read: it is 1)
    uint32_t count;
    uint32_t max_len;             // the longest polynomial = the length of the fold
};
// rows of workgroup totals: row p starts at tot + p * stride and holds one total per workgroup that len[p] coefficients span
template <class FR>
struct KzgRows {
    Fe<FR>* tot;
    uint32_t stride;
    uint32_t len[KZG_MAX_POLYS];
};

template <class FR>
__device__ __forceinline__ Fe<FR> kzg_pow(Fe<FR> base, uint32_t e) {
    Fe<FR> r = Fe<FR>::one();
    while (e) {
        if (e & 1u) r = r * base;
        e >>= 1;
        if (e) base = Fe<FR>::sqr(base);
    }
    return r;
}

// Suffix scan over the lanes of a workgroup (or over anything laid out one total per lane): on return `mine` = sum_{u >= t}
// total_u w^(u - t); the result is the exclusive one, sum_{u > t} total_u w^(u - t - 1).  sm holds KZG_THREADS elements.
template <class FR>
__device__ __forceinline__ Fe<FR> kzg_suffix_scan(Fe<FR>& mine, Fe<FR> w, Fe<FR>* sm) {
    using Fr = Fe<FR>;
    const uint32_t t = threadIdx.x;
    sm[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < KZG_THREADS; d <<= 1) {
        const bool has = t + d < KZG_THREADS;
        Fr o = has ? sm[t + d] : Fr::zero();
        __syncthreads();
        if (has) mine = mine + w * o;
        sm[t] = mine;
        __syncthreads();
        w = Fr::sqr(w);
    }
    return t + 1 < KZG_THREADS ? sm[t + 1] : Fr::zero();
}

// coefficient m of the fold
template <class FR>
__device__ __forceinline__ Fe<FR> kzg_fold_coeff(const KzgPolys<FR>& a, uint32_t m) {
    using Fr = Fe<FR>;
    Fr g = m < a.len[0] ? a.f[0][m] : Fr::zero();
    for (uint32_t i = 1; i < a.count; i++)
        if (m < a.len[i]) g = g + a.coef[i] * a.f[i][m];
    return g;
}

// launch 1 of an opening: grid = cdiv(max_len, KZG_BLOCK_SPAN).  q has max_len - 1 elements.
template <class FR>
struct KzgFoldBlockK {
    static __device__ __forceinline__ void run(KzgPolys<FR> a, Fe<FR> z, Fe<FR>* __restrict__ q, Fe<FR>* __restrict__ tot) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t base = blockIdx.x * KZG_BLOCK_SPAN + threadIdx.x * KZG_LANE_CHUNK;
        Fr v[KZG_LANE_CHUNK];
        Fr run = Fr::zero();
#pragma unroll
        for (int k = KZG_LANE_CHUNK - 1; k >= 0; k--) {
            const uint32_t m = base + k;
            if (m < a.max_len) run = kzg_fold_coeff<FR>(a, m) + z * run;     // (beyond the end the running value is still zero)
            v[k] = run;
        }
        const Fr zc = kzg_pow<FR>(z, KZG_LANE_CHUNK);
        Fr mine = run;
        const Fr carry = kzg_suffix_scan<FR>(mine, zc, sm);
        if (threadIdx.x == 0) tot[blockIdx.x] = mine;
        Fr zp = z;      // z^(chunk end - m)
#pragma unroll
        for (int k = KZG_LANE_CHUNK - 1; k >= 0; k--) {
            const uint32_t m = base + k;
            if (m >= 1 && m < a.max_len) q[m - 1] = v[k] + zp * carry;
            zp = zp * z;
        }
    }
};

// launch 1 of a batch evaluation: grid = (cdiv(longest, KZG_BLOCK_SPAN), count); workgroups beyond a polynomial's length exit
template <class FR>
struct KzgEvalBlockK {
    static __device__ __forceinline__ void run(KzgPolys<FR> a, Fe<FR> z, KzgRows<FR> rows) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t p = blockIdx.y, len = a.len[p];
        if (blockIdx.x * KZG_BLOCK_SPAN >= len) return;       // (uniform over the workgroup)
        const Fr* __restrict__ f = a.f[p];
        const uint32_t base = blockIdx.x * KZG_BLOCK_SPAN + threadIdx.x * KZG_LANE_CHUNK;
        Fr run = Fr::zero();
#pragma unroll
        for (int k = KZG_LANE_CHUNK - 1; k >= 0; k--) {
            const uint32_t m = base + k;
            if (m < len) run = f[m] + z * run;
        }
        const Fr zc = kzg_pow<FR>(z, KZG_LANE_CHUNK);
        Fr mine = run;
        (void)kzg_suffix_scan<FR>(mine, zc, sm);
        if (threadIdx.x == 0) rows.tot[(size_t)p * rows.stride + blockIdx.x] = mine;
    }
};

// launch 2: one workgroup per row.  Row p's totals become the carries INTO its workgroups, in place; value[p] = the row's
// polynomial at z.
template <class FR>
struct KzgCarryK {
    static __device__ __forceinline__ void run(KzgRows<FR> rows, Fe<FR> z, Fe<FR>* __restrict__ value) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t p = blockIdx.x, t = threadIdx.x;
        Fr* __restrict__ tot = rows.tot + (size_t)p * rows.stride;
        const uint32_t nb = (rows.len[p] + KZG_BLOCK_SPAN - 1) / KZG_BLOCK_SPAN;
        const uint32_t per = (nb + KZG_THREADS - 1) / KZG_THREADS;
        const uint32_t lo = min(t * per, nb), hi = min(lo + per, nb);
        const Fr w = kzg_pow<FR>(z, KZG_BLOCK_SPAN);
        Fr run = Fr::zero();
        for (uint32_t c = hi; c-- > lo;) run = tot[c] + w * run;
        // (a lane whose range is cut short or empty holds totals of zero beyond it, so every lane's range may count as `per` long)
        Fr mine = run;
        Fr acc = kzg_suffix_scan<FR>(mine, kzg_pow<FR>(w, per), sm);
        for (uint32_t c = hi; c-- > lo;) {
            const Fr x = tot[c];
            tot[c] = acc;
            acc = x + w * acc;
        }
        if (t == 0) value[p] = nb ? acc : Fr::zero();
    }
};

// launch 3 of an opening: same grid and lane map as launch 1.  The last workgroup has no carry.
template <class FR>
struct KzgApplyK {
    static __device__ __forceinline__ void run(const Fe<FR>* __restrict__ carries, Fe<FR> z, uint32_t max_len, Fe<FR>* __restrict__ q) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        const uint32_t end = (blockIdx.x + 1) * KZG_BLOCK_SPAN;
        if (end >= max_len) return;
        const Fr carry = carries[blockIdx.x];
        const uint32_t base = blockIdx.x * KZG_BLOCK_SPAN + threadIdx.x * KZG_LANE_CHUNK;
        Fr zp = kzg_pow<FR>(z, end - (base + KZG_LANE_CHUNK - 1));      // z^(end - m) for the lane's last element
#pragma unroll
        for (int k = KZG_LANE_CHUNK - 1; k >= 0; k--) {
            const uint32_t m = base + k;               // (m < end < max_len: every element of this workgroup exists)
            if (m >= 1) q[m - 1] = q[m - 1] + zp * carry;
            zp = zp * z;
        }
    }
};

// ---- openings at several points: a group of up to KZG_GROUP rows, each ONE polynomial at its own point (no fold, no weights) ----
// The three launches above with blockIdx.y (launch 2: blockIdx.x) as the row: row r reads f[r][0 .. len[r]), divides by X - z[r]
// into q[r] (len[r] - 1 elements; not touched when len[r] == 1) and keeps its workgroup totals in row r of `tot` (stride
// elements apart).  Same lane map, same order of the field operations as KzgFoldBlockK with one polynomial: the same bytes.
constexpr int KZG_GROUP = 4;                                   // = MSM_MAX_BATCH: a group's quotients are one MSM batch
template <class FR>
struct KzgGroup {
    const Fe<FR>* f[KZG_GROUP];
    Fe<FR>* q[KZG_GROUP];
    Fe<FR> z[KZG_GROUP];          // the points, by value
    uint32_t len[KZG_GROUP];
};

// launch 1: grid = (cdiv(longest, KZG_BLOCK_SPAN), rows); workgroups beyond their row's polynomial exit
template <class FR>
struct KzgGroupBlockK {
    static __device__ __forceinline__ void run(KzgGroup<FR> g, Fe<FR>* __restrict__ tot, uint32_t stride) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t r = blockIdx.y, len = g.len[r];
        if (blockIdx.x * KZG_BLOCK_SPAN >= len) return;       // (uniform over the workgroup)
        const Fr* __restrict__ f = g.f[r];
        Fr* __restrict__ q = g.q[r];
        const Fr z = g.z[r];
        const uint32_t base = blockIdx.x * KZG_BLOCK_SPAN + threadIdx.x * KZG_LANE_CHUNK;
        Fr v[KZG_LANE_CHUNK];
        Fr run = Fr::zero();
#pragma unroll
        for (int k = KZG_LANE_CHUNK - 1; k >= 0; k--) {
            const uint32_t m = base + k;
            if (m < len) run = f[m] + z * run;
            v[k] = run;
        }
        const Fr zc = kzg_pow<FR>(z, KZG_LANE_CHUNK);
        Fr mine = run;
        const Fr carry = kzg_suffix_scan<FR>(mine, zc, sm);
        if (threadIdx.x == 0) tot[(size_t)r * stride + blockIdx.x] = mine;
        Fr zp = z;      // z^(chunk end - m)
#pragma unroll
        for (int k = KZG_LANE_CHUNK - 1; k >= 0; k--) {
            const uint32_t m = base + k;
            if (m >= 1 && m < len) q[m - 1] = v[k] + zp * carry;
            zp = zp * z;
        }
    }
};

// launch 2: one workgroup per row, KzgCarryK with the row's own point; value[r] = f_r(z_r)
template <class FR>
struct KzgGroupCarryK {
    static __device__ __forceinline__ void run(KzgGroup<FR> g, Fe<FR>* __restrict__ tot_all, uint32_t stride, Fe<FR>* __restrict__ value) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t r = blockIdx.x, t = threadIdx.x;
        Fr* __restrict__ tot = tot_all + (size_t)r * stride;
        const uint32_t nb = (g.len[r] + KZG_BLOCK_SPAN - 1) / KZG_BLOCK_SPAN;
        const uint32_t per = (nb + KZG_THREADS - 1) / KZG_THREADS;
        const uint32_t lo = min(t * per, nb), hi = min(lo + per, nb);
        const Fr w = kzg_pow<FR>(g.z[r], KZG_BLOCK_SPAN);
        Fr run = Fr::zero();
        for (uint32_t c = hi; c-- > lo;) run = tot[c] + w * run;
        Fr mine = run;
        Fr acc = kzg_suffix_scan<FR>(mine, kzg_pow<FR>(w, per), sm);
        for (uint32_t c = hi; c-- > lo;) {
            const Fr x = tot[c];
            tot[c] = acc;
            acc = x + w * acc;
        }
        if (t == 0) value[r] = acc;      // (len[r] >= 1: the row has a workgroup)
    }
};

// launch 3: grid = (cdiv(longest, KZG_BLOCK_SPAN) - 1, rows); a row's last workgroup, and whatever lies beyond it, has no carry
template <class FR>
struct KzgGroupApplyK {
    static __device__ __forceinline__ void run(KzgGroup<FR> g, const Fe<FR>* __restrict__ carries, uint32_t stride) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        const uint32_t r = blockIdx.y;
        const uint32_t end = (blockIdx.x + 1) * KZG_BLOCK_SPAN;
        if (end >= g.len[r]) return;                          // (uniform over the workgroup)
        Fr* __restrict__ q = g.q[r];
        const Fr z = g.z[r];
        const Fr carry = carries[(size_t)r * stride + blockIdx.x];
        const uint32_t base = blockIdx.x * KZG_BLOCK_SPAN + threadIdx.x * KZG_LANE_CHUNK;
        Fr zp = kzg_pow<FR>(z, end - (base + KZG_LANE_CHUNK - 1));      // z^(end - m) for the lane's last element
#pragma unroll
        for (int k = KZG_LANE_CHUNK - 1; k >= 0; k--) {
            const uint32_t m = base + k;               // (m < end < len[r]: every element of this workgroup exists)
            if (m >= 1) q[m - 1] = q[m - 1] + zp * carry;
            zp = zp * z;
        }
    }
};

}  // namespace apk

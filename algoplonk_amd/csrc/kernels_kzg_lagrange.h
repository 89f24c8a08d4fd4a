// KZG openings in evaluation form (include/apk.h apk_kzg_open_lagrange*): the polynomial is given by its n values f_i = f(w^i)
// on the context's domain, natural order, and the quotient leaves here by its n values too - the MSM that follows runs over the
// Lagrange SRS.  No transform.  With d_i = w^i - z:
//   z off the domain   v = f(z) = (z^n - 1)/n * sum_i f_i w^i / (z - w^i)         q_i = (f_i - v) / d_i  for every i
//   z = w^m            v = f_m     q_i = (f_i - f_m) / d_i  for i != m            q_m = -w^(-m) * sum_{i != m} q_i w^i
// (the quotient has degree <= n - 2, so its values at the n - 1 other points fix the one at w^m: sum_i q_i w^i = n * [X^(n-1)] q = 0)
//
// The host decides "on the domain" (z^n == 1) and passes that and (z^n - 1)/n by value; WHICH m is found here: the one lane whose
// d_i is zero stores i to a device word and goes on with d_i = 1.
//
// The inverses come from one batch inversion over the whole domain with NO field inversion on the device: the product of all n
// denominators is known in closed form,
//   z off the domain   prod_i (w^i - z) = z^n - 1  (n is even)      - the host inverts it and passes 1/(z^n - 1)
//   z = w^m            prod_{i != m} (w^i - w^m) = -n w^(-m)        - the host passes 1/n, the inverse is -w^m / n
// so 1/d_i = (the product of every other denominator) / (the whole product).  (A first form inverted each workgroup's product by
// one lane: that lane's Fe::inv chain took 142 us whatever the size, 5/6 of the opening's own time - the kernel trace under
// profiles/.)
//
// Lane map: lane t of workgroup b owns the KZG_LAG_LANE_CHUNK consecutive values from b * KZG_LAG_BLOCK_SPAN + t * KZG_LAG_LANE_CHUNK.
//   1. KzgLagProdK     tot[b] = the product of workgroup b's denominators; lanes past n hold the identity
//      KzgLagInvK      inv[i] = 1 / d_i: chunk-local products, an inclusive prefix and an inclusive suffix product scan of the lane
//                      totals through LDS, the product of the OTHER workgroups' totals, then
//                      1/d_i = (everything before i) * (everything after i) * (the other workgroups) / (the whole product)
//   2. KzgLagSumK      off the domain only: workgroup partials of sum_i f_i w^i inv[i]; blockIdx.y = polynomial
//      KzgLagValueK    one workgroup per polynomial: v = -(z^n - 1)/n * the partials' sum, or f_m on the domain
//   3. KzgLagQuotK     q_i = (g_i - v) inv[i] in place over the inverses, g_i = sum_j coef_j f_j[i] folded on the fly; on the domain
//                      q_m = 0 for now and the workgroup's partial of sum_{i != m} q_i w^i
//      KzgLagFillK     on the domain only, one workgroup: q_m from the partials
// w^i comes from the context's table of w^k, k < n/2 (w^(k + n/2) = -w^k).
//
// Openings at several points (KzgLagGroup*K at the end of this file) are the six launches with the row - one vector at its own
// point, on the domain or off it - as a grid dimension.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ff.h"
#include "ffu.h"
#include "kernels_kzg.h"

namespace apk {

constexpr int KZG_LAG_LANE_CHUNK = 4;                                    // values per lane
constexpr int KZG_LAG_BLOCK_SPAN = KZG_THREADS * KZG_LAG_LANE_CHUNK;     // values per workgroup

// w^i, i < n, from tw[k] = w^k for k < n/2
template <class FR>
__device__ __forceinline__ Fe<FR> kzg_lag_omega(const Fe<FR>* __restrict__ tw, uint32_t n, uint32_t i) {
    const uint32_t h = n >> 1;
    return i < h ? tw[i] : Fe<FR>::neg(tw[i - h]);
}

// the workgroup's sum of `mine`, valid in lane 0.  sm holds KZG_THREADS elements and is free again on return.
template <class FR>
__device__ __forceinline__ Fe<FR> kzg_lag_block_sum(Fe<FR> mine, Fe<FR>* sm) {
    const uint32_t t = threadIdx.x;
    sm[t] = mine;
    __syncthreads();
    for (uint32_t d = KZG_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d) sm[t] = sm[t] + sm[t + d];
        __syncthreads();
    }
    const Fe<FR> r = sm[0];
    __syncthreads();
    return r;
}

// the workgroup's product of `mine`, in every lane.  sm holds KZG_THREADS elements and is free again on return.
template <class FR>
__device__ __forceinline__ Fe<FR> kzg_lag_block_product(Fe<FR> mine, Fe<FR>* sm) {
    const uint32_t t = threadIdx.x;
    sm[t] = mine;
    __syncthreads();
    for (uint32_t d = KZG_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d) sm[t] = sm[t] * sm[t + d];
        __syncthreads();
    }
    const Fe<FR> r = sm[0];
    __syncthreads();
    return r;
}

// the lane's denominators d_i = w^i - z; the identity past n and at z itself, where *at receives i when `at` is not null
template <class FR>
__device__ __forceinline__ void kzg_lag_denominators(const Fe<FR>* __restrict__ tw, uint32_t n, const Fe<FR>& z, uint32_t base,
                                                     Fe<FR>* d, uint32_t* __restrict__ at) {
    using Fr = Fe<FR>;
#pragma unroll
    for (int k = 0; k < KZG_LAG_LANE_CHUNK; k++) {
        const uint32_t i = base + k;
        d[k] = Fr::one();
        if (i < n) {
            const Fr x = kzg_lag_omega<FR>(tw, n, i) - z;
            if (!x.is_zero()) d[k] = x;
            else if (at) *at = i;
        }
    }
}

// launch 1a: grid = cdiv(n, KZG_LAG_BLOCK_SPAN).  tot[b] = workgroup b's product; *at receives m when z = w^m.
template <class FR>
struct KzgLagProdK {
    static __device__ __forceinline__ void run(const Fe<FR>* __restrict__ tw, uint32_t n, Fe<FR> z, Fe<FR>* __restrict__ tot,
                                               uint32_t* __restrict__ at) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        Fr d[KZG_LAG_LANE_CHUNK];
        kzg_lag_denominators<FR>(tw, n, z, blockIdx.x * KZG_LAG_BLOCK_SPAN + threadIdx.x * KZG_LAG_LANE_CHUNK, d, at);
        Fr p = d[0];
#pragma unroll
        for (int k = 1; k < KZG_LAG_LANE_CHUNK; k++) p = p * d[k];
        p = kzg_lag_block_product<FR>(p, sm);
        if (threadIdx.x == 0) tot[blockIdx.x] = p;
    }
};

// launch 1b: same grid.  inv has n elements.  tot: the gridDim.x workgroup products of launch 1a.  whole = 1/(z^n - 1) off the
// domain, 1/n on it (the inverse of the whole product is then -w^m / n, m = *at).
template <class FR>
struct KzgLagInvK {
    static __device__ __forceinline__ void run(const Fe<FR>* __restrict__ tw, uint32_t n, Fe<FR> z, const Fe<FR>* __restrict__ tot, Fe<FR> whole,
                                               uint32_t on_domain, const uint32_t* __restrict__ at, Fe<FR>* __restrict__ inv) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr pre[KZG_THREADS], suf[KZG_THREADS];
        const uint32_t t = threadIdx.x, nb = gridDim.x;
        const uint32_t base = blockIdx.x * KZG_LAG_BLOCK_SPAN + t * KZG_LAG_LANE_CHUNK;
        Fr d[KZG_LAG_LANE_CHUNK], lp[KZG_LAG_LANE_CHUNK];      // the denominators; their running product inside the chunk
        kzg_lag_denominators<FR>(tw, n, z, base, d, nullptr);
        lp[0] = d[0];
#pragma unroll
        for (int k = 1; k < KZG_LAG_LANE_CHUNK; k++) lp[k] = lp[k - 1] * d[k];
        // inclusive product scans of the lane totals: pre[t] = totals 0..t, suf[t] = totals t..255
        Fr up = lp[KZG_LAG_LANE_CHUNK - 1], dn = up;
        pre[t] = up;
        suf[t] = dn;
        __syncthreads();
        for (uint32_t s = 1; s < KZG_THREADS; s <<= 1) {
            const bool hl = t >= s, hr = t + s < KZG_THREADS;
            const Fr a = hl ? pre[t - s] : Fr::one(), b = hr ? suf[t + s] : Fr::one();
            __syncthreads();
            if (hl) up = up * a;
            if (hr) dn = dn * b;
            pre[t] = up;
            suf[t] = dn;
            __syncthreads();
        }
        const Fr before = t ? pre[t - 1] : Fr::one(), after = t + 1 < KZG_THREADS ? suf[t + 1] : Fr::one();
        __syncthreads();
        // 1 / (this workgroup's product) = (the other workgroups' products) / (the whole product)
        Fr others = Fr::one();
        if (nb > 1) {                                           // (uniform over the launch)
            for (uint32_t c = t; c < nb; c += KZG_THREADS)
                if (c != blockIdx.x) others = others * tot[c];
            others = kzg_lag_block_product<FR>(others, pre);
        }
        if (on_domain) {
            const uint32_t m = *at;
            whole = Fr::neg(whole * kzg_lag_omega<FR>(tw, n, m < n ? m : 0));      // (the host saw z^n == 1, so launch 1a stored m < n)
        }
        Fr run = before * after * (others * whole);             // 1 / (this lane's total), then times the chunk's factors after k
#pragma unroll
        for (int k = KZG_LAG_LANE_CHUNK - 1; k >= 0; k--) {
            const uint32_t i = base + k;
            if (i < n) inv[i] = k ? run * lp[k - 1] : run;
            run = run * d[k];
        }
    }
};

// launch 2 off the domain: grid = (cdiv(n, KZG_LAG_BLOCK_SPAN), count); part[p * gridDim.x + b] = workgroup b's share of
// sum_i f_p[i] w^i inv[i]
template <class FR>
struct KzgLagSumK {
    static __device__ __forceinline__ void run(KzgPolys<FR> a, const Fe<FR>* __restrict__ tw, uint32_t n, const Fe<FR>* __restrict__ inv,
                                               Fe<FR>* __restrict__ part) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const Fr* __restrict__ f = a.f[blockIdx.y];
        const uint32_t base = blockIdx.x * KZG_LAG_BLOCK_SPAN + threadIdx.x * KZG_LAG_LANE_CHUNK;
        Fr acc = Fr::zero();
#pragma unroll
        for (int k = 0; k < KZG_LAG_LANE_CHUNK; k++) {
            const uint32_t i = base + k;
            if (i < n) acc = acc + f[i] * (kzg_lag_omega<FR>(tw, n, i) * inv[i]);
        }
        acc = kzg_lag_block_sum<FR>(acc, sm);
        if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
    }
};

// launch 2, the finish: grid = count.  value[p] (and pinned[p], the host's view, when there is one) = f_p(z).  nb = the
// workgroups of KzgLagSumK; scale = (z^n - 1)/n.
template <class FR>
struct KzgLagValueK {
    static __device__ __forceinline__ void run(KzgPolys<FR> a, const Fe<FR>* __restrict__ part, uint32_t nb, Fe<FR> scale, uint32_t on_domain,
                                               const uint32_t* __restrict__ at, Fe<FR>* __restrict__ value, Fe<FR>* __restrict__ pinned) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t p = blockIdx.x, t = threadIdx.x;
        Fr v;
        if (on_domain) {                                        // (uniform over the launch)
            if (t) return;
            const uint32_t m = *at;
            v = m < a.max_len ? a.f[p][m] : Fr::zero();         // (the host saw z^n == 1, so launch 1 stored m < n)
        } else {
            Fr acc = Fr::zero();
            for (uint32_t c = t; c < nb; c += KZG_THREADS) acc = acc + part[(size_t)p * nb + c];
            acc = kzg_lag_block_sum<FR>(acc, sm);
            if (t) return;
            v = Fr::neg(scale * acc);                           // 1 / (z - w^i) = -inv[i]
        }
        value[p] = v;
        if (pinned) pinned[p] = v;
    }
};

// launch 3: grid = cdiv(n, KZG_LAG_BLOCK_SPAN).  q holds the inverses on entry and the quotient's values on return.  The value
// of the fold comes from the device (vptr, the single opening: nothing was read back) or by value (the batch call folded it on
// the host).  On the domain part[b] = workgroup b's share of sum_{i != m} q_i w^i.
template <class FR>
struct KzgLagQuotK {
    static __device__ __forceinline__ void run(KzgPolys<FR> a, const Fe<FR>* __restrict__ tw, uint32_t n, const Fe<FR>* __restrict__ vptr, Fe<FR> vval,
                                               uint32_t on_domain, const uint32_t* __restrict__ at, Fe<FR>* __restrict__ q, Fe<FR>* __restrict__ part) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const Fr v = vptr ? *vptr : vval;
        const uint32_t m = on_domain ? *at : 0xffffffffu;
        const uint32_t base = blockIdx.x * KZG_LAG_BLOCK_SPAN + threadIdx.x * KZG_LAG_LANE_CHUNK;
        Fr acc = Fr::zero();
#pragma unroll
        for (int k = 0; k < KZG_LAG_LANE_CHUNK; k++) {
            const uint32_t i = base + k;
            if (i < n) {
                Fr x = (kzg_fold_coeff<FR>(a, i) - v) * q[i];
                if (i == m) x = Fr::zero();
                q[i] = x;
                if (on_domain) acc = acc + x * kzg_lag_omega<FR>(tw, n, i);
            }
        }
        if (!on_domain) return;                                 // (uniform over the launch)
        acc = kzg_lag_block_sum<FR>(acc, sm);
        if (threadIdx.x == 0) part[blockIdx.x] = acc;
    }
};

// launch 3, the finish on the domain: one workgroup.  q[m] = -w^(-m) * sum of the nb partials; w^(-m) = w^(n - m).
template <class FR>
struct KzgLagFillK {
    static __device__ __forceinline__ void run(const Fe<FR>* __restrict__ tw, uint32_t n, const Fe<FR>* __restrict__ part, uint32_t nb,
                                               const uint32_t* __restrict__ at, Fe<FR>* __restrict__ q) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t t = threadIdx.x;
        Fr acc = Fr::zero();
        for (uint32_t c = t; c < nb; c += KZG_THREADS) acc = acc + part[c];
        acc = kzg_lag_block_sum<FR>(acc, sm);
        if (t) return;
        const uint32_t m = *at;
        if (m >= n) return;                                     // (the host saw z^n == 1, so some lane of launch 1 stored m < n)
        q[m] = Fr::neg(m ? kzg_lag_omega<FR>(tw, n, n - m) * acc : acc);
    }
};

// ---- openings at several points: a group of up to KZG_GROUP rows, each ONE vector at its own point (no fold, no weights) ----------
// The six launches above with blockIdx.y (the two finishing launches: blockIdx.x) as the row.  Row r reads f[r][0 .. n), keeps its
// inverses and then its quotient in q[r] (n elements), its m word in *at[r], and its workgroup products, then its partial sums,
// then its quotient's partials in row r of `aux` (stride elements apart, stride >= the workgroups over n).  A group may hold rows
// on the domain and rows off it: on_domain[r] is uniform over the workgroups of a row.  Same lane map and the same order of the
// field operations as the single form with one vector - launches 1a, 1b and the fill ARE the single form's bodies: the same bytes.
template <class FR>
struct KzgLagGroup {
    const Fe<FR>* f[KZG_GROUP];
    Fe<FR>* q[KZG_GROUP];
    uint32_t* at[KZG_GROUP];        // where row r's m goes when z[r] = w^m
    Fe<FR> z[KZG_GROUP];            // the points, by value
    Fe<FR> scale[KZG_GROUP];        // (z^n - 1)/n
    Fe<FR> whole[KZG_GROUP];        // 1/(z^n - 1) off the domain, 1/n on it
    uint32_t on_domain[KZG_GROUP];
};

// launch 1a: grid = (cdiv(n, KZG_LAG_BLOCK_SPAN), rows)
template <class FR>
struct KzgLagGroupProdK {
    static __device__ __forceinline__ void run(KzgLagGroup<FR> g, const Fe<FR>* __restrict__ tw, uint32_t n, Fe<FR>* __restrict__ aux, uint32_t stride) {
        const uint32_t r = blockIdx.y;
        KzgLagProdK<FR>::run(tw, n, g.z[r], aux + (size_t)r * stride, g.at[r]);
    }
};

// launch 1b: same grid
template <class FR>
struct KzgLagGroupInvK {
    static __device__ __forceinline__ void run(KzgLagGroup<FR> g, const Fe<FR>* __restrict__ tw, uint32_t n, const Fe<FR>* __restrict__ aux, uint32_t stride) {
        const uint32_t r = blockIdx.y;
        KzgLagInvK<FR>::run(tw, n, g.z[r], aux + (size_t)r * stride, g.whole[r], g.on_domain[r], g.at[r], g.q[r]);
    }
};

// launch 2: same grid; the workgroups of a row on the domain exit
template <class FR>
struct KzgLagGroupSumK {
    static __device__ __forceinline__ void run(KzgLagGroup<FR> g, const Fe<FR>* __restrict__ tw, uint32_t n, Fe<FR>* __restrict__ aux, uint32_t stride) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t r = blockIdx.y;
        if (g.on_domain[r]) return;                             // (uniform over the workgroup)
        const Fr* __restrict__ f = g.f[r];
        const Fr* __restrict__ inv = g.q[r];
        const uint32_t base = blockIdx.x * KZG_LAG_BLOCK_SPAN + threadIdx.x * KZG_LAG_LANE_CHUNK;
        Fr acc = Fr::zero();
#pragma unroll
        for (int k = 0; k < KZG_LAG_LANE_CHUNK; k++) {
            const uint32_t i = base + k;
            if (i < n) acc = acc + f[i] * (kzg_lag_omega<FR>(tw, n, i) * inv[i]);
        }
        acc = kzg_lag_block_sum<FR>(acc, sm);
        if (threadIdx.x == 0) aux[(size_t)r * stride + blockIdx.x] = acc;
    }
};

// launch 2, the finish: grid = rows.  value[r] = f_r(z_r); nb = the workgroups of a row
template <class FR>
struct KzgLagGroupValueK {
    static __device__ __forceinline__ void run(KzgLagGroup<FR> g, const Fe<FR>* __restrict__ aux, uint32_t stride, uint32_t nb, uint32_t n,
                                               Fe<FR>* __restrict__ value) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t r = blockIdx.x, t = threadIdx.x;
        Fr v;
        if (g.on_domain[r]) {                                   // (uniform over the workgroup)
            if (t) return;
            const uint32_t m = *g.at[r];
            v = m < n ? g.f[r][m] : Fr::zero();                 // (the host saw z^n == 1, so launch 1 stored m < n)
        } else {
            const Fr* __restrict__ part = aux + (size_t)r * stride;
            Fr acc = Fr::zero();
            for (uint32_t c = t; c < nb; c += KZG_THREADS) acc = acc + part[c];
            acc = kzg_lag_block_sum<FR>(acc, sm);
            if (t) return;
            v = Fr::neg(g.scale[r] * acc);                      // 1 / (z - w^i) = -inv[i]
        }
        value[r] = v;
    }
};

// launch 3: grid = (cdiv(n, KZG_LAG_BLOCK_SPAN), rows).  q[r] holds the inverses on entry and the quotient's values on return;
// value[r] is what launch 2 left.  A row on the domain leaves its workgroups' shares of sum_{i != m} q_i w^i in its row of aux.
template <class FR>
struct KzgLagGroupQuotK {
    static __device__ __forceinline__ void run(KzgLagGroup<FR> g, const Fe<FR>* __restrict__ tw, uint32_t n, const Fe<FR>* __restrict__ value,
                                               Fe<FR>* __restrict__ aux, uint32_t stride) {
        wave_priority<APK_PRIO_FR>();
        using Fr = Fe<FR>;
        __shared__ Fr sm[KZG_THREADS];
        const uint32_t r = blockIdx.y, on_domain = g.on_domain[r];
        const Fr* __restrict__ f = g.f[r];
        Fr* __restrict__ q = g.q[r];
        const Fr v = value[r];
        const uint32_t m = on_domain ? *g.at[r] : 0xffffffffu;
        const uint32_t base = blockIdx.x * KZG_LAG_BLOCK_SPAN + threadIdx.x * KZG_LAG_LANE_CHUNK;
        Fr acc = Fr::zero();
#pragma unroll
        for (int k = 0; k < KZG_LAG_LANE_CHUNK; k++) {
            const uint32_t i = base + k;
            if (i < n) {
                Fr x = (f[i] - v) * q[i];
                if (i == m) x = Fr::zero();
                q[i] = x;
                if (on_domain) acc = acc + x * kzg_lag_omega<FR>(tw, n, i);
            }
        }
        if (!on_domain) return;                                 // (uniform over the workgroup)
        acc = kzg_lag_block_sum<FR>(acc, sm);
        if (threadIdx.x == 0) aux[(size_t)r * stride + blockIdx.x] = acc;
    }
};

// launch 3, the finish: grid = rows; the workgroup of a row off the domain exits
template <class FR>
struct KzgLagGroupFillK {
    static __device__ __forceinline__ void run(KzgLagGroup<FR> g, const Fe<FR>* __restrict__ tw, uint32_t n, const Fe<FR>* __restrict__ aux, uint32_t stride,
                                               uint32_t nb) {
        const uint32_t r = blockIdx.x;
        if (!g.on_domain[r]) return;                            // (uniform over the workgroup)
        KzgLagFillK<FR>::run(tw, n, aux + (size_t)r * stride, nb, g.at[r], g.q[r]);
    }
};

}  // namespace apk

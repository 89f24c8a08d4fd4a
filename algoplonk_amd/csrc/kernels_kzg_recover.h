// The kernels of apk_kzg_recover_cosets: the polynomial back from ANY k of its n' cells (a cell = its l values on one coset of the
// domain), the middle of the sampling pipeline between apk_kzg_open_cosets (the producer) and apk_kzg_batch_verify_cosets.
//
// Notation of kernels_kzg_cosets.h: w generates the size-n domain, l = 2^k' is the coset size, n' = n / l, a_i = w^(i l), coset i
// holds x_(i,j) = w^(i + n' j), j < l - the roots of X^l - a_i.  g is the context's coset shift (FRP::COSET_SHIFT): g^n != 1, so
// g^l a_t is never an a_i.  K = the k known coset indices, their values in rows (row of coset i, column j = f(x_(i,j))), M = the
// other m = n' - k.  f has len <= k l coefficients.
//     (1)  Z(X) = prod_{i in M} (X^l - a_i)             a polynomial in X^l: on the domain it takes n' distinct values
//          zH[t] = prod_{i in M} (a_t - a_i)      t < n'    zero exactly for t in M
//          zG[t] = prod_{i in M} (g^l a_t - a_i)  t < n'    never zero
//     (2)  E[i + n' j] = values_i[j] zH[i] for i in K,  0 for i in M         natural order, n entries: (f Z) on the domain
//     (3)  P = IDFT_n(E)                               P = f Z, since deg f Z < len + m l <= n
//     (4)  PG[q] = P(g w^q)                            forward coset transform, size n
//     (5)  Q[q] = PG[q] / zG[q mod n']                 = f(g w^q)
//     (6)  f_c = g^(-c) IDFT_n(Q)_c
// For ANY k rows - cells of one polynomial or not - E vanishes on the m l points of the missing cosets, so Z divides P and f comes
// out with no coefficient at or above k l: it is THE polynomial below degree k l through the k l points.  A caller that states
// len < k l and finds a non-zero coefficient in [len, k l) did not hold cells of one polynomial of len coefficients
// (APK_ERR_VERIFY; tail_nonzero_kernel of kernels_poly.h over those words, before anything is copied out).
//
// Launches of a call, all plain, on one stream; no lane waits for memory another workgroup writes:
//   kzg_recover_roots_kernel     the m roots a_i, i in M, gathered from the context's table of w^e into a compact array
//   kzg_recover_vanish_kernel    (1): 2n' lanes, 2 n' m multiplications - the only kernel with arithmetic weight
//   kzg_recover_scatter_kernel   (2): the inverse permutation of kzg_cosets_values_kernel, fused with the product by zH
//   run_ntt                      (3) inverse, scaled by 1 / n;  (4) forward with `pre` = g^c
//   kzg_recover_divide_kernel    (5), in place
//   run_ntt                      (6) inverse with `post` = g^(-c) / n
//   tail_nonzero_kernel          the coefficients in [len, k l)
//   kzg_recover_emit_kernel      the len coefficients to the caller's device buffer (or not one word, after a non-zero tail)
//
// Out of scope: polynomials of more than n coefficients; recovery from single points instead of whole cosets; more than
// APK_KZG_RECOVER_MAX_COSETS cosets (the vanish kernel is quadratic in n'); a sub-quadratic vanishing polynomial.
#pragma once
#include "ff.h"
#include "kzg_recover_plan.h"

namespace apk {

// w^e for e < n from the table tw[e] = w^e, e < n / 2  (w^(n/2) = -1)
template <class FR>
__device__ __forceinline__ Fe<FR> kzg_recover_domain_power(const Fe<FR>* __restrict__ tw, uint32_t e, uint32_t half_n) {
    return e < half_n ? tw[e] : Fe<FR>::neg(tw[e - half_n]);
}

// roots[j] = a_(missing[j]) = w^(missing[j] l);  j < m
template <class FR>
__global__ void __launch_bounds__(KZG_RECOVER_THREADS) kzg_recover_roots_kernel(const uint32_t* __restrict__ missing, uint32_t m,
                                                                                const Fe<FR>* __restrict__ tw, int log_l, uint32_t half_n,
                                                                                Fe<FR>* __restrict__ roots) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    roots[j] = kzg_recover_domain_power<FR>(tw, missing[j] << log_l, half_n);
}

// Lane t < n': zh[t] = prod_j (a_t - roots[j]);  lane n' + t: zg_inv[t] = 1 / prod_j (g^l a_t - roots[j]).  gl = g^l.
// A workgroup stages the roots through LDS, KZG_RECOVER_TILE at a time (one per lane); every lane multiplies its running product
// by (y - root) for the tile's roots, y in registers.  m and the tile bounds are workgroup-uniform: every lane - the ones beyond
// 2n' included - reaches every __syncthreads().  m = 0: the loop does not run, nothing is read, zh = zg_inv = 1.
template <class FR>
__global__ void __launch_bounds__(KZG_RECOVER_THREADS) kzg_recover_vanish_kernel(const Fe<FR>* __restrict__ roots, uint32_t m,
                                                                                 const Fe<FR>* __restrict__ tw, uint32_t np, int log_l,
                                                                                 uint32_t half_n, Fe<FR> gl, Fe<FR>* __restrict__ zh,
                                                                                 Fe<FR>* __restrict__ zg_inv) {
    using Fr = Fe<FR>;
    static_assert(KZG_RECOVER_TILE == KZG_RECOVER_THREADS, "one root per lane and tile");
    static_assert(sizeof(Fr) == KZG_RECOVER_FR_BYTES, "the planner's LDS figure");
    __shared__ Fr sh[KZG_RECOVER_TILE];
    const uint32_t lane = blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    const bool live = lane < 2 * np, shifted = lane >= np;
    const uint32_t t = lane & (np - 1u);
    Fr y = Fr::one(), acc = Fr::one();
    if (live) {
        y = kzg_recover_domain_power<FR>(tw, t << log_l, half_n);
        if (shifted) y = y * gl;
    }
    for (uint32_t base = 0; base < m; base += KZG_RECOVER_TILE) {
        const uint32_t cnt = m - base < KZG_RECOVER_TILE ? m - base : KZG_RECOVER_TILE;
        if (threadIdx.x < cnt) sh[threadIdx.x] = roots[base + threadIdx.x];
        __syncthreads();
        if (live)
            for (uint32_t j = 0; j < cnt; j++) acc = acc * (y - sh[j]);
        __syncthreads();
    }
    if (!live) return;
    if (shifted) zg_inv[t] = Fr::inv(acc);
    else zh[t] = acc;
}

// e[i + n' j] = values[row_of[i] l + j] zh[i], or zero where coset i has no row;  p = i + n' j < n
template <class FR>
__global__ void __launch_bounds__(KZG_RECOVER_THREADS) kzg_recover_scatter_kernel(const Fe<FR>* __restrict__ values, const int32_t* __restrict__ row_of,
                                                                                  const Fe<FR>* __restrict__ zh, uint32_t n, int log_np, int log_l,
                                                                                  Fe<FR>* __restrict__ e) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = p & ((1u << log_np) - 1u), j = p >> log_np;
    const int32_t row = row_of[i];
    e[p] = row < 0 ? Fe<FR>::zero() : values[((size_t)row << log_l) + j] * zh[i];
}

// q[p] *= zg_inv[p mod n'];  p < n
template <class FR>
__global__ void __launch_bounds__(KZG_RECOVER_THREADS) kzg_recover_divide_kernel(Fe<FR>* __restrict__ q, const Fe<FR>* __restrict__ zg_inv, uint32_t n,
                                                                                 uint32_t np) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    q[p] = q[p] * zg_inv[p & (np - 1u)];
}

// out[c] = f[c], c < len - unless the tail check before it stamped this call's epoch into *flag
template <class FR>
__global__ void __launch_bounds__(KZG_RECOVER_THREADS) kzg_recover_emit_kernel(const Fe<FR>* __restrict__ f, uint32_t len, const uint32_t* __restrict__ flag,
                                                                               uint32_t epoch, Fe<FR>* __restrict__ out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= len || *flag == epoch) return;
    out[c] = f[c];
}

}  // namespace apk

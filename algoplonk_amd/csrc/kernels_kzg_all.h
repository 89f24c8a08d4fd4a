// The kernels of apk_kzg_open_all: the openings of ONE polynomial at every point of its domain (Feist - Khovratovich, "FK20").
//
// f has len <= n coefficients, s_j = [tau^j]G1 is the canonical SRS, w the domain's generator, w_2n that of the size-2n domain.
//     H_i = [(f - f(w^i)) / (X - w^i)] = sum_{k <= n-2} w^(ik) h_k,     h_k = sum_{j <= n-2-k} f_(k+1+j) s_j
// so the n openings are the forward size-n transform IN THE EXPONENT of the points h_k, and the h_k are a correlation of the
// coefficients with the SRS, taken as a cyclic convolution of size 2n:
//     a = (f_1 .. f_(n-1), 0 x (n+1))          A^ = DFT_2n(a)      scalars: two size-n NTTs of the context (kzg_all_run.h)
//     t = (s_(n-2) .. s_0, inf x (n+1))        T^ = DFT_2n(t)      points: once per context (apk_kzg_all_prepare)
//     c = IDFT_2n(A^_i T^_i)                   h_k = c[k + n - 2], k <= n - 2
// Both sequences have n - 1 terms: the linear convolution has 2n - 3 and nothing wraps.  The 1/(2n) of the inverse transform
// rides in A^ (the NTT's scale operand).
//
// Launches, all plain, on one stream; no lane waits for memory another workgroup writes:
//   kzg_all_pointwise_kernel   P^_i = A^_i T^_i, written to the bit-reversed position of the 2n-point XYZZ work array
//   stage kernel x log(2n)     decimation in time, inverse twiddles: work = c, natural order
//   kzg_all_gather_kernel      c[k + n - 2] to the bit-reversed position k of the FIRST n points of the same array (two launches:
//                              the two sources below n move before anything is written there), infinity at n - 1
//   stage kernel x log(n)      forward twiddles: work[i] = H_i
//   kzg_all_finish_kernel      XYZZ -> affine, infinity = (0, 0)
// The stages are the hot path: (log 2n) n + (log n) n / 2 butterflies, each a scalar multiplication by a twiddle.  Two forms:
//   kzg_all_stage_glv_kernel   the twiddle comes split (kzg_all_twiddles.h): k1 and k2 are walked together over P and
//                              phi(P) = (beta X, Y, ZZ, ZZZ) - HALF_BITS doublings and as many additions
//   lagrange_stage_kernel      (kernels_setup.h, as it is) over plain tables of powers: 255 doublings, ~128 additions
// Same group elements either way, so the same bytes (APK_KZG_ALL_GLV picks).
#pragma once
#include "ec.h"
#include "kernels_setup.h"      // scalar_mul_point, lagrange_load_kernel, lagrange_stage_kernel
#include "kzg_all_twiddles.h"   // KzgAllTwiddle

namespace apk {

constexpr int KZG_ALL_THREADS = 128;

// P^_i = A^_i T^_i.  A^_(2i) = a_even[i], A^_(2i+1) = a_odd[i] (Montgomery); that[] = T^ affine, natural order.
template <class FR, class FP>
__global__ void __launch_bounds__(KZG_ALL_THREADS) kzg_all_pointwise_kernel(const Fe<FR>* __restrict__ a_even, const Fe<FR>* __restrict__ a_odd,
                                                                            const Affine<FP>* __restrict__ that, uint32_t n2, int log_n2,
                                                                            XYZZ<FP>* __restrict__ work) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n2) return;
    const Fe<FR> a = (i & 1u) ? a_odd[i >> 1] : a_even[i >> 1];
    const Affine<FP> t = that[i];
    const uint32_t j = __brev(i) >> (32 - log_n2);
    if (a.is_zero() || t.is_inf()) { work[j] = XYZZ<FP>::inf(); return; }
    work[j] = scalar_mul_point<FR, FP>(XYZZ<FP>::from_affine(t), Fe<FR>::from_mont(a));
}

// limb-wise choice among three field elements; exactly one of the masks is all ones
template <class F>
__device__ __forceinline__ F kzg_all_pick(uint32_t ma, uint32_t mb, uint32_t mc, const F& a, const F& b, const F& c) {
    F r;
#pragma unroll
    for (int i = 0; i < F::N; i++) r.l[i] = (a.l[i] & ma) | (b.l[i] & mb) | (c.l[i] & mc);
    return r;
}

// One decimation-in-time stage t of a transform over `points` = 2 * half points: pairs (i, i + 2^t), twiddle w_2n^(+-e) with
// e = (i mod 2^t) << shift < n_tab.  tab[j] = the split of w_2n^j, j < n_tab = n; the size-2n transform has shift = log(2n) - 1 - t
// and the size-n transform the same (its twiddles are the even entries).  inverse: w_2n^(-e) = -w_2n^(n_tab - e).
// beta in Montgomery form.
template <class FP>
__global__ void __launch_bounds__(KZG_ALL_THREADS) kzg_all_stage_glv_kernel(XYZZ<FP>* __restrict__ work, const KzgAllTwiddle* __restrict__ tab,
                                                                            Fe<FP> beta, uint32_t half, int t, int shift, uint32_t n_tab,
                                                                            int inverse) {
    using F = Fe<FP>;
    using Pt = XYZZ<FP>;
    constexpr int W = KZG_ALL_HALF_WORDS;
    const uint32_t bf = blockIdx.x * blockDim.x + threadIdx.x;
    if (bf >= half) return;
    const uint32_t low = bf & ((1u << t) - 1u);
    const uint32_t i0 = ((bf >> t) << (t + 1)) | low, i1 = i0 | (1u << t);
    Pt v = work[i1];
    if (low != 0 && !v.is_inf()) {
        const uint32_t e = low << shift;
        const KzgAllTwiddle tw = tab[inverse ? n_tab - e : e];
        const uint32_t flip = inverse ? 3u : 0u;
        const bool neg1 = ((tw.neg ^ flip) & 1u) != 0, neg2 = ((tw.neg ^ flip) & 2u) != 0;
        // A = +-P, B = +-phi(P) = (beta X, +-Y, ZZ, ZZZ), S = A + B (phi(P) = lambda P is never +-P for a point of order r)
        Pt A = v;
        if (neg1) A.neg_inplace();
        const F bx = beta * v.X;
        const F by = neg2 ? F::neg(v.Y) : v.Y;
        Pt S = A;
        S.add(Pt{bx, by, v.ZZ, v.ZZZ});
        uint32_t k1[W], k2[W];
#pragma unroll
        for (int w = 0; w < W; w++) { k1[w] = tw.k1[w]; k2[w] = tw.k2[w]; }
        Pt acc = Pt::inf();
        bool started = false;
        for (int bit = 0; bit < 32 * W; bit++) {
            const uint32_t b1 = k1[W - 1] >> 31, b2 = k2[W - 1] >> 31;
#pragma unroll
            for (int w = W - 1; w > 0; w--) { k1[w] = (k1[w] << 1) | (k1[w - 1] >> 31); k2[w] = (k2[w] << 1) | (k2[w - 1] >> 31); }
            k1[0] <<= 1; k2[0] <<= 1;
            if (started) acc = Pt::dbl(acc);
            if (b1 | b2) {
                // the operand by masks, not from an array of points: 1 0 -> A, 0 1 -> B, 1 1 -> S
                const uint32_t ma = 0u - (b1 & (b2 ^ 1u)), mb = 0u - (b2 & (b1 ^ 1u)), ms = 0u - (b1 & b2);
                Pt op;
                op.X = kzg_all_pick(ma, mb, ms, A.X, bx, S.X);
                op.Y = kzg_all_pick(ma, mb, ms, A.Y, by, S.Y);
                op.ZZ = kzg_all_pick(ma | mb, 0u, ms, A.ZZ, A.ZZ, S.ZZ);
                op.ZZZ = kzg_all_pick(ma | mb, 0u, ms, A.ZZZ, A.ZZZ, S.ZZZ);
                acc.add(op);
                started = true;
            }
        }
        v = acc;
    }
    Pt u = work[i0];
    Pt s = u;
    s.add(v);
    v.neg_inplace();
    u.add(v);
    work[i0] = s;
    work[i1] = u;
}

// work[bit-reversed k] = c[k + n - 2] for k0 <= k < k1 <= n, infinity for k = n - 1; c and work are the SAME array (the first n
// of its 2n points are the destination).  k in [0, 2) reads c[n - 2], c[n - 1] and writes positions 0 and n / 2 < n - 2; k in
// [2, n) reads c[n .. 2n - 4] and writes below n: neither launch reads what it writes.
template <class FP>
__global__ void __launch_bounds__(KZG_ALL_THREADS) kzg_all_gather_kernel(XYZZ<FP>* work, uint32_t n, int log_n, uint32_t k0, uint32_t k1) {
    const uint32_t k = k0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= k1) return;
    const uint32_t j = __brev(k) >> (32 - log_n);
    work[j] = k == n - 1 ? XYZZ<FP>::inf() : work[(size_t)k + n - 2];
}

// out[i] = work[i] in affine form, infinity = (0, 0)
template <class FP>
__global__ void __launch_bounds__(KZG_ALL_THREADS) kzg_all_finish_kernel(const XYZZ<FP>* __restrict__ work, uint32_t count,
                                                                         Affine<FP>* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = work[i].to_affine();
}

}  // namespace apk

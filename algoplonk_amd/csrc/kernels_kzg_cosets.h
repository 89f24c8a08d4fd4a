// The kernels of apk_kzg_open_cosets: the openings of ONE polynomial on every coset of l points of its domain (Feist -
// Khovratovich, "FK20", the multi-point form).
//
// n = the domain, w its generator, l = 2^k the coset size (2 <= l <= n / 2), n' = n / l, w_2n' = w_2n^l, s_j = [tau^j]G1,
// f has len <= n coefficients.  Coset i < n' holds x_(i,j) = w^(i + n' j), j < l; all of them satisfy x^l = a_i = w^(i l).
//     H_i = [(f - I_i) / (X^l - a_i)] = sum_{m <= n'-2} (w^l)^(i m) h_m,     h_m = sum_j f_(j + l(m+1)) s_j,  h_(n'-1) = infinity
// so the n' proofs are the forward size-n' transform IN THE EXPONENT of the points h_m, and the h_m are l correlations of
// strided coefficients with strided SRS points, each a cyclic convolution of size 2n', summed BEFORE the inverse transform:
//     a_c = (f_(c+l), f_(c+2l) .. f_(c+l(n'-1)), 0 x (n'+1))         A^_c = DFT_2n'(a_c)     2l size-n' NTTs per call
//     t_c = (s_(c+l(n'-2)) .. s_(c+l), s_c, inf x (n'+1))            T^_c = DFT_2n'(t_c)     once per context
//     P^_i = sum_{c<l} A^_c[i] T^_c[i],   cc = IDFT_2n'(P^),   h_m = cc[m + n' - 2]
// The highest SRS index read is n - l - 1.  The 1 / (2n') of the inverse transform rides in A^ (the NTT's scale operand), which
// also leaves A^ as PLAIN integers below r - the bits the pointwise kernel walks - instead of Montgomery residues.
//
// Launches of a call, all plain, on one stream; no lane waits for memory another workgroup writes:
//   kzg_cosets_split_kernel       a_c[u] = f_(c + l(u+1)), the l strided gathers (the twist by w_2n'^u is the NTT's `pre`)
//   kzg_cosets_values_kernel      NTT_n(f) from natural to coset-major order
//   kzg_cosets_pointwise_kernel   P^_i, written to the bit-reversed position of the 2n'-point XYZZ work array: the hot path
//   then kernels_kzg_all.h's sequence with n' in place of n: inverse stages, the two gathers, forward stages, finish
// and of apk_kzg_cosets_prepare:
//   lagrange_load_kernel, log(2n') stages over 2n points (the l transforms side by side), kzg_cosets_table_kernel
//
// THE TABLE.  tab[(4 i + v) l + c] = [2^(64 v)] T^_c[i], affine, for i < 2n', v < 4, c < l: the 4 l bases of output i are
// contiguous, window-major.  8n affine points (64 MiB for BN254 at 2^17, 12 MiB for BLS12-381 at 2^14, whatever l).
//
// THE POINTWISE KERNEL.  Output i is a sum of l scalar multiplications over bases that are constants of the context.  Each 256-bit
// scalar is cut into four 64-bit windows and window v meets the base [2^(64 v)] T^_c[i], so output i is a sum of 4 l "pairs"
// (c, v) of a 64-bit scalar and a fixed base.  A group of min(4 l, 64) lanes serves one output: lane q takes the pairs q,
// q + group, .. and walks them TOGETHER from bit 63 down - one doubling per bit for all its pairs, one mixed addition per set
// bit - so the doublings are paid once per lane, not once per term, and no Horner recombination follows.  The lanes' partial sums
// meet in an LDS tree as in lincomb_reduce_kernel.  The bases and the scalar words are read from memory where they are used: no
// array of points is indexed at run time (it would go to scratch).  Every addition is the COMPLETE form of ec.h (madd / add fall
// through to doubling or infinity): a crafted polynomial makes the terms of an output equal or opposite.  A zero scalar has no
// set bit and an infinite base is skipped by madd: neither contributes.
//
// Out of scope: evaluation-form input; polynomials of more than n coefficients (the blinded polynomials of a proof); several
// coset sizes on one context; cosets of a size-2n extension of the domain (a polynomial of len <= n / 2 coefficients IS
// erasure-coded by its n' cells: kernels_kzg_recover.h brings it back from any half of them).
#pragma once
#include "ec.h"
#include "kernels_kzg_all.h"    // the stage, gather and finish kernels

namespace apk {

constexpr int KZG_COSETS_THREADS = 64;     // lanes per workgroup of the pointwise kernel: one wave
constexpr int KZG_COSETS_WINDOWS = 4;      // 64-bit windows of a 256-bit scalar

// a[c n' + u] = f_(c + l(u + 1)) for u < n' - 1 (zero beyond len), a[c n' + n' - 1] = 0;  idx < n = l n'
template <class FR>
__global__ void __launch_bounds__(256) kzg_cosets_split_kernel(const Fe<FR>* __restrict__ f, uint32_t len, uint32_t n, int log_np, int log_l,
                                                               Fe<FR>* __restrict__ a) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const uint32_t c = idx >> log_np, u = idx & ((1u << log_np) - 1u);
    const uint64_t src = (uint64_t)c + ((uint64_t)(u + 1) << log_l);
    a[idx] = src < len ? f[src] : Fe<FR>::zero();      // (u = n' - 1: src >= n >= len)
}

// out[i l + j] = v[i + n' j]: coset i's values side by side;  idx < n
template <class FR>
__global__ void __launch_bounds__(256) kzg_cosets_values_kernel(const Fe<FR>* __restrict__ v, uint32_t n, int log_np, int log_l,
                                                                Fe<FR>* __restrict__ out) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const uint32_t i = idx >> log_l, j = idx & ((1u << log_l) - 1u);
    out[idx] = v[i + (j << log_np)];
}

// Prepare: work holds the l transforms side by side - block b = bit-reversed c (of log l bits) is T^_c in natural order, 2n'
// points each, n2 = 2n in all.  One lane per point writes its four table entries (to_affine: infinity = (0, 0)).
template <class FP>
__global__ void __launch_bounds__(128) kzg_cosets_table_kernel(const XYZZ<FP>* __restrict__ work, uint32_t n2, int log_np2, int log_l,
                                                               Affine<FP>* __restrict__ tab) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n2) return;
    const uint32_t b = idx >> log_np2, i = idx & ((1u << log_np2) - 1u);
    const uint32_t c = __brev(b) >> (32 - log_l);
    XYZZ<FP> p = work[idx];
    for (int v = 0; v < KZG_COSETS_WINDOWS; v++) {
        tab[((((size_t)i * KZG_COSETS_WINDOWS) + v) << log_l) + c] = p.to_affine();
        if (v + 1 < KZG_COSETS_WINDOWS)
            for (int d = 0; d < 64; d++) p = XYZZ<FP>::dbl(p);
    }
}

// P^_i = sum_{c<l} A^_c[i] T^_c[i] for i < np2 = 2n', to work[bit-reversed i].  A^_c[2i] = a_even[c n' + i], A^_c[2i+1] =
// a_odd[c n' + i], PLAIN integers below r.  log_group = log2(lanes per output) = min(log l + 2, 6); a workgroup serves
// 64 >> log_group outputs.  The loop bounds of the tree are workgroup-uniform: every lane reaches every __syncthreads().
// The sum is stated ONCE, here: this kernel and kzg_cosets_pointwise_multi_kernel (kernels_kzg_cosets_multi.h: G polynomials over the
// same table, one per blockIdx.y) call it with their own operands and their workgroup's LDS array sh[KZG_COSETS_THREADS].
template <class FR, class FP>
__device__ __forceinline__ void kzg_cosets_pointwise_sum(const Fe<FR>* __restrict__ a_even, const Fe<FR>* __restrict__ a_odd,
                                                         const Affine<FP>* __restrict__ tab, uint32_t np2, int log_np2, int log_l, int log_group,
                                                         XYZZ<FP>* __restrict__ work, XYZZ<FP>* sh) {
    using Pt = XYZZ<FP>;
    static_assert(sizeof(Fe<FR>) == Fe<FR>::N * sizeof(uint32_t), "a scalar is its limbs");
    const uint32_t tid = threadIdx.x, group = 1u << log_group;
    const uint32_t q = tid & (group - 1u);
    const uint32_t i = blockIdx.x * (KZG_COSETS_THREADS >> log_group) + (tid >> log_group);
    const bool live = i < np2;
    Pt acc = Pt::inf();
    if (live) {
        const uint32_t np = np2 >> 1, pairs = (uint32_t)KZG_COSETS_WINDOWS << log_l, cmask = (1u << log_l) - 1u;
        const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(((i & 1u) ? a_odd : a_even) + (i >> 1));
        const Affine<FP>* __restrict__ base = tab + (size_t)i * pairs;
        for (int b = 63; b >= 0; b--) {
            acc = Pt::dbl(acc);
            for (uint32_t p = q; p < pairs; p += group) {
                const uint32_t c = p & cmask, v = p >> log_l;
                const uint32_t word = words[(size_t)c * np * Fe<FR>::N + 2 * v + ((uint32_t)b >> 5)];
                if ((word >> (b & 31)) & 1u) acc.madd(base[p]);
            }
        }
    }
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t stride = group >> 1; stride >= 1; stride >>= 1) {
        if (q < stride) {
            Pt a = sh[tid];
            a.add(sh[tid + stride]);
            sh[tid] = a;
        }
        __syncthreads();
    }
    if (live && q == 0) work[__brev(i) >> (32 - log_np2)] = sh[tid];
}
template <class FR, class FP>
__global__ void __launch_bounds__(KZG_COSETS_THREADS) kzg_cosets_pointwise_kernel(const Fe<FR>* __restrict__ a_even, const Fe<FR>* __restrict__ a_odd,
                                                                                  const Affine<FP>* __restrict__ tab, uint32_t np2, int log_np2,
                                                                                  int log_l, int log_group, XYZZ<FP>* __restrict__ work) {
    __shared__ XYZZ<FP> sh[KZG_COSETS_THREADS];
    kzg_cosets_pointwise_sum<FR, FP>(a_even, a_odd, tab, np2, log_np2, log_l, log_group, work, sh);
}

}  // namespace apk

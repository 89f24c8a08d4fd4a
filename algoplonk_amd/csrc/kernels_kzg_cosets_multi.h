// The kernels of apk_kzg_open_cosets_multi: the openings of G <= NTT_ARGS_MAX polynomials on every coset of their domain, side by
// side in the launches of ONE (kernels_kzg_cosets.h has the formulas and the table; kzg_fk20_plan.h "LAYOUT" has where everything
// lies).  A stage launch lasts as long as one butterfly's serial chain whether it has n' lanes or G n', so G polynomials pay the
// 2 log(2n') - 1 stage launches once: the stage kernels are those of the single call, unchanged, over G 2n' and G n' points - they
// pair (i, i + 2^t) inside aligned blocks of 2^(t+1) points and never cross a polynomial's 2n' (n') points.
//
// Launches of a group, all plain, on one stream; no lane waits for memory another workgroup writes:
//   kzg_cosets_values_multi_kernel      NTT_n(f_b) from natural to coset-major order, per polynomial          G n lanes
//   kzg_cosets_split_multi_kernel       a_(b,c)[u] = f_b[c + l(u+1)], zero beyond len_b                        G n lanes
//   kzg_cosets_pointwise_multi_kernel   P^_b over the SAME table: the single kernel's grid x G in blockIdx.y, and its body
//   kzg_cosets_gather_multi_kernel      cc_b[k + n' - 2] to the bit-reversed position k of block b of a SECOND array (the in-place
//                                       gather of the single call does not survive compaction: block b's destination overlaps
//                                       block b / 2's source)                                                 G n' lanes
// A polynomial of len <= l is no special case: its a_(b,c) are all zero, no bit is set, and infinity goes through every stage.
#pragma once
#include "kernels_kzg_cosets.h"
#include "ntt_plan.h"      // NTT_ARGS_MAX

namespace apk {

// the G sources of a group and their lengths, by value as the NTT's arguments travel
template <class FR>
struct KzgCosetsMultiSrc {
    const Fe<FR>* f[NTT_ARGS_MAX];
    uint32_t len[NTT_ARGS_MAX];
};

// out[b n + i l + j] = v[b n + i + n' j];  idx < total = G n
template <class FR>
__global__ void __launch_bounds__(256) kzg_cosets_values_multi_kernel(const Fe<FR>* __restrict__ v, uint32_t total, int log_n, int log_np, int log_l,
                                                                     Fe<FR>* __restrict__ out) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t k = idx & ((1u << log_n) - 1u);
    const uint32_t i = k >> log_l, j = k & ((1u << log_l) - 1u);
    out[idx] = v[(idx - k) + i + (j << log_np)];
}

// a[(b l + c) n' + u] = f_b[c + l(u + 1)] for u < n' - 1 (zero beyond len_b), 0 at u = n' - 1;  idx = b n + c n' + u < total = G n
template <class FR>
__global__ void __launch_bounds__(256) kzg_cosets_split_multi_kernel(KzgCosetsMultiSrc<FR> src, uint32_t total, int log_n, int log_np, int log_l,
                                                                    Fe<FR>* __restrict__ a) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t b = idx >> log_n, k = idx & ((1u << log_n) - 1u);
    const uint32_t c = k >> log_np, u = k & ((1u << log_np) - 1u);
    const uint64_t at = (uint64_t)c + ((uint64_t)(u + 1) << log_l);
    a[idx] = at < src.len[b] ? src.f[b][at] : Fe<FR>::zero();      // (u = n' - 1: at >= n >= len_b)
}

// kzg_cosets_pointwise_kernel for polynomial b = blockIdx.y: its rows of A^ start at b n = b l n' scalars, its block of work at
// b 2n' points; the table is the context's, the same for all.
template <class FR, class FP>
__global__ void __launch_bounds__(KZG_COSETS_THREADS) kzg_cosets_pointwise_multi_kernel(const Fe<FR>* __restrict__ a_even, const Fe<FR>* __restrict__ a_odd,
                                                                                        const Affine<FP>* __restrict__ tab, uint32_t np2, int log_np2,
                                                                                        int log_l, int log_group, XYZZ<FP>* __restrict__ work) {
    __shared__ XYZZ<FP> sh[KZG_COSETS_THREADS];
    const size_t b = blockIdx.y, rows = ((size_t)np2 >> 1) << log_l;
    kzg_cosets_pointwise_sum<FR, FP>(a_even + b * rows, a_odd + b * rows, tab, np2, log_np2, log_l, log_group, work + b * np2, sh);
}

// second[b n' + bit-reversed k] = work[b 2n' + k + n' - 2] for k < n' - 1, infinity for k = n' - 1;  idx = b n' + k < total = G n'.
// Out of place: no lane reads what any lane writes.
template <class FP>
__global__ void __launch_bounds__(KZG_ALL_THREADS) kzg_cosets_gather_multi_kernel(const XYZZ<FP>* __restrict__ work, uint32_t total, uint32_t np, int log_np,
                                                                                  XYZZ<FP>* __restrict__ second) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint32_t k = idx & (np - 1u);
    const uint32_t j = __brev(k) >> (32 - log_np);
    second[(idx - k) + j] = k == np - 1 ? XYZZ<FP>::inf() : work[(size_t)2 * (idx - k) + k + np - 2];
}

}  // namespace apk

// The fold of many coset openings' values: the device half of apk_kzg_batch_verify_cosets / apk_kzg_cosets_fold (include/apk.h;
// the rule is KzgProtocol::cosets_check of kzg_protocol.h).  Instantiated in lincomb_bn254.hip / lincomb_bls12381.hip, beside the
// segmented sums whose stream and pooled buffer (LincombScope) it shares.
//
//     q_c = sum_k scale_k step_k^c U_(k,c),   U_k = the size-l inverse transform of row k WITHOUT its 1 / l      c < l = 2^log_l
//
// `count` rows of l Fr (Montgomery, row-major); the host supplies per row scale_k = lambda_k / l and step_k = w^(-index[k]) and,
// once per call, the table tw[j] = g^(-j), j < 512, g the generator of the domain of 1 024 points.
//
//   kzg_cosets_fold_kernel         A workgroup of 256 lanes owns one TILE of KZG_FOLD_TILE = 1 024 elements = 1 024 / l whole rows
//                                  (32 KiB of consecutive memory; 2 <= l <= 1 024) and walks its tiles grid-stride.  Per tile:
//                                    load      lane t takes elements t, t + 256, t + 512, t + 768 of the run; element (row, c)
//                                              lands at (row, bit-reversed c).  Rows past `count` are zeros.
//                                    transform log_l butterfly stages over the whole tile at once - 512 butterflies a stage, two
//                                              per lane; a row is an aligned group of l elements, so one index map serves every
//                                              row.  Stage t (half = 2^t) reads tw[k (512 >> t)], k the position in the half:
//                                              the inverse l-th root's powers are the table read with a stride of 1 024 / l.
//                                    weights   every lane takes its four elements to registers, the tile becomes the rows'
//                                              powers: P(row, 0) = 1, P(row, 1) = step_row, then log_l doubling steps - step s
//                                              fills c in (2^s, 2^(s+1)] as P(c - 2^s) P(2^s), one product per element, the
//                                              elements of a step spread densely over the lanes.  Then element (row, c) becomes
//                                              U P(row, c) scale_row and goes back to the tile.
//                                    columns   a tree over the tile's rows: [0, h) += [h, 2h) for h = 512 .. l, after which the
//                                              first l elements are the tile's column sums; lane t adds columns t, t + 256, ..
//                                              to its four running sums (registers).
//                                  At its end a workgroup writes its l running sums to part[workgroup][c].
//   kzg_cosets_fold_reduce_kernel  one lane per column: adds the at most KZG_FOLD_GRID_MAX partials; q_c is canonical (every sum
//                                  and product of ff.h is).
//
// The tile is LIMB-MAJOR in LDS (limb i of element e at word i * 1 024 + e): lanes that touch consecutive elements touch
// consecutive banks; element-major, a 32-byte element at a 32-byte stride puts every fourth lane on one bank.
// Plain launches on the LincombScope stream, no cooperative launch, no atomics, no lane that waits on another workgroup's
// memory; every loop bound and every __syncthreads() is workgroup-uniform; one host synchronisation, at the end.  The products are
// the plain Fe product of ff.h.  Coset sizes above 1 024 do not come here: their interpolation runs on the host threads
// (KzgProtocol::cosets_fold), and only the point checks and the segmented sum of the verifier stay on the device.
#pragma once
#include "kernels_lincomb.h"

namespace apk {

constexpr uint32_t KZG_FOLD_TILE = 1024;        // field elements per tile: 32 KiB of LDS
constexpr int KZG_FOLD_LOG_TILE = 10;
constexpr uint32_t KZG_FOLD_LANES = 256;
constexpr uint32_t KZG_FOLD_PER_LANE = KZG_FOLD_TILE / KZG_FOLD_LANES;
constexpr uint32_t KZG_FOLD_GRID_MAX = 256;     // workgroups of a launch = partial sums per column

template <class FRP>
__device__ __forceinline__ Fe<FRP> fold_lds_get(const uint32_t* sh, uint32_t e) {
    Fe<FRP> r;
#pragma unroll
    for (int i = 0; i < Fe<FRP>::N; i++) r.l[i] = sh[i * KZG_FOLD_TILE + e];
    return r;
}
template <class FRP>
__device__ __forceinline__ void fold_lds_put(uint32_t* sh, uint32_t e, const Fe<FRP>& v) {
#pragma unroll
    for (int i = 0; i < Fe<FRP>::N; i++) sh[i * KZG_FOLD_TILE + e] = v.l[i];
}

template <class FRP>
__global__ void __launch_bounds__(KZG_FOLD_LANES) kzg_cosets_fold_kernel(const Fe<FRP>* __restrict__ values, const Fe<FRP>* __restrict__ scale,
                                                                         const Fe<FRP>* __restrict__ step, const Fe<FRP>* __restrict__ tw,
                                                                         uint32_t count, int log_l, uint32_t nb_tiles,
                                                                         Fe<FRP>* __restrict__ part) {
    using Fr = Fe<FRP>;
    static_assert(Fr::N * KZG_FOLD_TILE * 4 == 32768, "a tile is 32 KiB");
    __shared__ uint32_t sh[Fr::N * KZG_FOLD_TILE];
    const uint32_t t = threadIdx.x;
    const uint32_t l = 1u << log_l, rows_tile = KZG_FOLD_TILE >> log_l;
    const uint64_t total = (uint64_t)count << log_l;          // elements that exist
    Fr acc[KZG_FOLD_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < KZG_FOLD_PER_LANE; j++) acc[j] = Fr::zero();

    for (uint32_t tile = blockIdx.x; tile < nb_tiles; tile += gridDim.x) {      // workgroup-uniform
        const uint64_t base = (uint64_t)tile << KZG_FOLD_LOG_TILE;
        const uint32_t row0 = tile * rows_tile;
        // ---- load, bit-reversed inside each row
#pragma unroll
        for (uint32_t j = 0; j < KZG_FOLD_PER_LANE; j++) {
            const uint32_t e = t + j * KZG_FOLD_LANES;
            const Fr v = base + e < total ? values[base + e] : Fr::zero();
            const uint32_t c = e & (l - 1);
            fold_lds_put<FRP>(sh, (e - c) | (__brev(c) >> (32 - log_l)), v);
        }
        __syncthreads();
        // ---- the inverse transform of every row of the tile, 1 / l left out
        for (int s = 0; s < log_l; s++) {
            const uint32_t half = 1u << s;
#pragma unroll
            for (uint32_t j = 0; j < KZG_FOLD_TILE / 2 / KZG_FOLD_LANES; j++) {
                const uint32_t b = t + j * KZG_FOLD_LANES, k = b & (half - 1);
                const uint32_t i0 = ((b >> s) << (s + 1)) + k, i1 = i0 + half;
                const Fr u = fold_lds_get<FRP>(sh, i0);
                const Fr x = fold_lds_get<FRP>(sh, i1) * tw[k * ((KZG_FOLD_TILE / 2) >> s)];
                fold_lds_put<FRP>(sh, i0, u + x);
                fold_lds_put<FRP>(sh, i1, u - x);
            }
            __syncthreads();
        }
        // ---- the tile to registers; the rows' powers in its place
        Fr v[KZG_FOLD_PER_LANE];
#pragma unroll
        for (uint32_t j = 0; j < KZG_FOLD_PER_LANE; j++) v[j] = fold_lds_get<FRP>(sh, t + j * KZG_FOLD_LANES);
        __syncthreads();
        for (uint32_t i = t; i < 2 * rows_tile; i += KZG_FOLD_LANES) {
            const uint32_t row = i >> 1;
            Fr p = Fr::one();
            if ((i & 1u) && row0 + row < count) p = step[row0 + row];
            fold_lds_put<FRP>(sh, (row << log_l) | (i & 1u), p);
        }
        __syncthreads();
        for (int s = 0; s < log_l; s++) {
            // c in (2^s, 2^(s+1)], c < l: rows_tile * 2^s elements, spread over the lanes
            const uint32_t span = 1u << s, todo = rows_tile << s;
            for (uint32_t i = t; i < todo; i += KZG_FOLD_LANES) {
                const uint32_t row = i >> s, c = span + 1 + (i & (span - 1));
                if (c < l) {
                    const uint32_t r0 = row << log_l;
                    fold_lds_put<FRP>(sh, r0 + c, fold_lds_get<FRP>(sh, r0 + c - span) * fold_lds_get<FRP>(sh, r0 + span));
                }
            }
            __syncthreads();
        }
        // ---- element (row, c) = U step^c scale
#pragma unroll
        for (uint32_t j = 0; j < KZG_FOLD_PER_LANE; j++) {
            const uint32_t e = t + j * KZG_FOLD_LANES, row = row0 + (e >> log_l);
            const Fr sc = row < count ? scale[row] : Fr::zero();
            v[j] = v[j] * fold_lds_get<FRP>(sh, e) * sc;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < KZG_FOLD_PER_LANE; j++) fold_lds_put<FRP>(sh, t + j * KZG_FOLD_LANES, v[j]);
        __syncthreads();
        // ---- the tile's column sums
        for (uint32_t h = KZG_FOLD_TILE / 2; h >= l; h >>= 1) {
            for (uint32_t i = t; i < h; i += KZG_FOLD_LANES) fold_lds_put<FRP>(sh, i, fold_lds_get<FRP>(sh, i) + fold_lds_get<FRP>(sh, i + h));
            __syncthreads();
        }
#pragma unroll
        for (uint32_t j = 0; j < KZG_FOLD_PER_LANE; j++) {
            const uint32_t c = t + j * KZG_FOLD_LANES;
            if (c < l) acc[j] = acc[j] + fold_lds_get<FRP>(sh, c);
        }
        __syncthreads();                                                        // the next tile's load overwrites the sums
    }
#pragma unroll
    for (uint32_t j = 0; j < KZG_FOLD_PER_LANE; j++) {
        const uint32_t c = t + j * KZG_FOLD_LANES;
        if (c < l) part[(size_t)blockIdx.x * l + c] = acc[j];
    }
}

template <class FRP>
__global__ void __launch_bounds__(KZG_FOLD_LANES) kzg_cosets_fold_reduce_kernel(const Fe<FRP>* __restrict__ part, uint32_t nb_parts, uint32_t l,
                                                                                Fe<FRP>* __restrict__ out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= l) return;
    Fe<FRP> acc = Fe<FRP>::zero();
    for (uint32_t p = 0; p < nb_parts; p++) acc = acc + part[(size_t)p * l + c];
    out[c] = acc;
}

// host arrays in and out; 1 <= log_l <= 10 (the C-ABI checks), tw = KZG_FOLD_TILE / 2 Fr.  count = 0: the device is opened
// (APK_ERR_HIP where there is none) and nothing runs - the caller folds on the host.
template <class FRP>
int kzg_cosets_fold_impl(int device, int log_l, uint32_t count, const void* values, const void* scale, const void* step, const void* tw,
                         void* out) {
    using Fr = Fe<FRP>;
    if (count && (log_l < 1 || log_l > KZG_FOLD_LOG_TILE)) { set_error("kzg: the fold kernel takes cosets of 2..%u points", KZG_FOLD_TILE); return APK_ERR_ARG; }
    const uint32_t l = count ? 1u << log_l : 0, rows_tile = count ? KZG_FOLD_TILE >> log_l : 1;
    const uint32_t nb_tiles = (count + rows_tile - 1) / rows_tile;
    const uint32_t grid = nb_tiles < KZG_FOLD_GRID_MAX ? nb_tiles : KZG_FOLD_GRID_MAX;
    const size_t nv = (size_t)count << log_l;
    const size_t o_val = 0, o_scale = o_val + lc_align(nv * sizeof(Fr)), o_step = o_scale + lc_align(count * sizeof(Fr)),
                 o_tw = o_step + lc_align(count * sizeof(Fr)), o_part = o_tw + lc_align(KZG_FOLD_TILE / 2 * sizeof(Fr)),
                 o_out = o_part + lc_align((size_t)grid * l * sizeof(Fr)), bytes = o_out + lc_align(l * sizeof(Fr));
    LincombScope sc;
    const int rc = sc.open(device, bytes);
    if (rc != APK_OK || count == 0) return rc;
    uint8_t* base = (uint8_t*)sc.mem;
    LC_HIP(hipMemcpyAsync(base + o_val, values, nv * sizeof(Fr), hipMemcpyHostToDevice, sc.st));
    LC_HIP(hipMemcpyAsync(base + o_scale, scale, count * sizeof(Fr), hipMemcpyHostToDevice, sc.st));
    LC_HIP(hipMemcpyAsync(base + o_step, step, count * sizeof(Fr), hipMemcpyHostToDevice, sc.st));
    LC_HIP(hipMemcpyAsync(base + o_tw, tw, KZG_FOLD_TILE / 2 * sizeof(Fr), hipMemcpyHostToDevice, sc.st));
    kzg_cosets_fold_kernel<FRP><<<grid, KZG_FOLD_LANES, 0, sc.st>>>((const Fr*)(base + o_val), (const Fr*)(base + o_scale), (const Fr*)(base + o_step),
                                                                     (const Fr*)(base + o_tw), count, log_l, nb_tiles, (Fr*)(base + o_part));
    LC_HIP(hipGetLastError());
    kzg_cosets_fold_reduce_kernel<FRP><<<(l + KZG_FOLD_LANES - 1) / KZG_FOLD_LANES, KZG_FOLD_LANES, 0, sc.st>>>((const Fr*)(base + o_part), grid, l,
                                                                                                                 (Fr*)(base + o_out));
    LC_HIP(hipGetLastError());
    LC_HIP(hipMemcpyAsync(out, base + o_out, l * sizeof(Fr), hipMemcpyDeviceToHost, sc.st));
    LC_HIP(hipStreamSynchronize(sc.st));
    return APK_OK;
}

}  // namespace apk

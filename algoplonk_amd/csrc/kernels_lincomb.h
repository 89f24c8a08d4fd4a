// Segmented variable-base G1 sums and per-point checks: the device half of the batch verifier (verify_host.h BatchVerifier,
// include/apk.h apk_verify_batch / apk_g1_lincomb_segments).
//
//     out[s] = sum over i in [seg[s], seg[s+1]) of k_i * P_i        P_i arbitrary affine points, k_i Fr (Montgomery)
//
// There is no table to amortise (every point is fresh) and the work is a few thousand dependent chains of ~254 doublings, so
// lanes are scarce: a scalar is cut into four 64-bit windows ACROSS lanes.
//
//   lincomb_partial_kernel   one lane per (term, window): lane 4i + w computes  part[4i + w] = k_i[64w .. 64w + 63] * P_i
//                            (64 doublings, <= 64 mixed additions); 352 stage-1 terms of a 32-proof batch are 22 waves, not 6.
//   lincomb_reduce_kernel    one workgroup of 256 lanes per segment: lane 64w + l adds part[4i + w] for i = seg[s] + l, + 64, ..,
//                            the 64 partial sums of a window meet in a six-step LDS tree, then ONE lane shifts the four window
//                            sums together (Horner: 3 x 64 doublings - the shift is paid once per segment, not once per term)
//                            and leaves the segment's sum in affine form.
//   g1_check_kernel          one lane per point: bit 0 = not on the curve, bit 1 = [r]P != infinity (BLS12-381 only; BN254's
//                            G1 has cofactor 1).
//
// Every addition is the COMPLETE form of ec.h (add / madd / dbl fall through to doubling or infinity): equal and opposite
// operands do occur (the same key point in every segment, L = R in tiny circuits, P and -P in the tests).  The special cases are
// branches inside one lane; no lane waits for another outside the __syncthreads() of the tree, which every lane of the
// workgroup reaches (the loop bounds are workgroup-uniform).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <string.h>
#include <vector>

#include "backend.h"
#include "ec.h"

namespace apk {

constexpr int LINCOMB_WINDOWS = 4;        // 64-bit windows of a 256-bit scalar
constexpr int LINCOMB_TREE = 64;          // lanes per window in the reduction workgroup

template <class FRP, class FPP>
__global__ void __launch_bounds__(256) lincomb_partial_kernel(const Affine<FPP>* __restrict__ points, const Fe<FRP>* __restrict__ scalars,
                                                              uint32_t terms, XYZZ<FPP>* __restrict__ part) {
    using Pt = XYZZ<FPP>;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = t >> 2, w = t & 3u;
    if (i >= terms) return;
    const Affine<FPP> p = points[i];
    const Fe<FRP> k = Fe<FRP>::from_mont(scalars[i]);
    const uint64_t chunk = (uint64_t)k.l[2 * w] | (uint64_t)k.l[2 * w + 1] << 32;
    Pt acc = Pt::inf();
    for (int b = 63; b >= 0; b--) {
        acc = Pt::dbl(acc);
        if ((chunk >> b) & 1ull) acc.madd(p);
    }
    part[t] = acc;
}

template <class FPP>
__global__ void __launch_bounds__(256) lincomb_reduce_kernel(const XYZZ<FPP>* __restrict__ part, const uint64_t* __restrict__ seg,
                                                             uint32_t nb_segments, Affine<FPP>* __restrict__ out) {
    using Pt = XYZZ<FPP>;
    __shared__ Pt sh[LINCOMB_WINDOWS * LINCOMB_TREE];
    const uint32_t s = blockIdx.x;
    if (s >= nb_segments) return;                       // workgroup-uniform
    const uint32_t tid = threadIdx.x, w = tid / LINCOMB_TREE, l = tid % LINCOMB_TREE;
    const uint64_t lo = seg[s], hi = seg[s + 1];
    Pt acc = Pt::inf();
    for (uint64_t i = lo + l; i < hi; i += LINCOMB_TREE) acc.add(part[i * LINCOMB_WINDOWS + w]);
    sh[tid] = acc;
    __syncthreads();
    for (uint32_t stride = LINCOMB_TREE / 2; stride >= 1; stride >>= 1) {
        if (l < stride) {
            Pt a = sh[tid];
            a.add(sh[tid + stride]);
            sh[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) {
        Pt r = sh[(LINCOMB_WINDOWS - 1) * LINCOMB_TREE];
        for (int ww = LINCOMB_WINDOWS - 2; ww >= 0; ww--) {
            for (int b = 0; b < 64; b++) r = Pt::dbl(r);
            r.add(sh[ww * LINCOMB_TREE]);
        }
        out[s] = r.to_affine();
    }
}

template <class FRP, class FPP, bool SUBGROUP>
__global__ void __launch_bounds__(256) g1_check_kernel(const Affine<FPP>* __restrict__ points, uint32_t count, uint8_t* __restrict__ flags) {
    using F = Fe<FPP>;
    using Pt = XYZZ<FPP>;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Affine<FPP> p = points[i];
    uint8_t f = 0;
    if (!p.is_inf()) {
        F b = F::zero();
        b.l[0] = FPP::CURVE_B;
        if (!(F::sqr(p.y) == F::sqr(p.x) * p.x + F::to_mont(b))) f |= 1;
        if (SUBGROUP && !f) {
            const Fe<FRP> q = Fe<FRP>::modulus();
            Pt acc = Pt::inf();
            for (int wd = Fe<FRP>::N - 1; wd >= 0; wd--)
                for (int bit = 31; bit >= 0; bit--) {
                    acc = Pt::dbl(acc);
                    if ((q.l[wd] >> bit) & 1u) acc.madd(p);
                }
            if (!acc.is_inf()) f |= 2;
        }
    }
    flags[i] = f;
}

#define LC_HIP(x)                                                                           \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                             \
            set_error("%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__);     \
            return APK_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

// One call's device state: a stream of its own (non-blocking: a verifier never waits for, or holds up, a proving context's
// streams) and one allocation.  Both are kept for the next call in a small per-process pool instead of being released: a batch is
// three calls, and hipFree waits for the whole device - for every prover running beside the verifier.  A buffer is only replaced
// when a call needs a larger one; at most LINCOMB_POOL_MAX idle entries are kept, the rest is released as before.
constexpr size_t LINCOMB_POOL_MAX = 8;
struct LincombRes {
    int device = -1;
    hipStream_t st = nullptr;
    void* mem = nullptr;
    size_t bytes = 0;
    void release() {
        if (mem) (void)hipFree(mem);
        if (st) (void)hipStreamDestroy(st);
        mem = nullptr; st = nullptr; bytes = 0;
    }
};
struct LincombPool {
    std::mutex mu;
    std::vector<LincombRes> idle;
    static LincombPool& get() { static LincombPool* p = new LincombPool(); return *p; }   // never destroyed: no HIP call at exit
};
struct LincombScope {
    LincombRes r;
    hipStream_t st = nullptr;
    void* mem = nullptr;
    ~LincombScope() {
        if (r.device < 0) return;
        LincombPool& pool = LincombPool::get();
        {
            std::lock_guard<std::mutex> lk(pool.mu);
            if (r.st && r.mem && pool.idle.size() < LINCOMB_POOL_MAX) { pool.idle.push_back(r); return; }
        }
        (void)hipSetDevice(r.device);
        r.release();
    }
    int open(int device, size_t bytes) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); set_error("no HIP device available; libapk has no CPU fallback"); return APK_ERR_HIP; }
        if (device < 0 || device >= ndev) { set_error("device %d out of range", device); return APK_ERR_HIP; }
        LC_HIP(hipSetDevice(device));
        if (bytes == 0) bytes = 16;
        {
            LincombPool& pool = LincombPool::get();
            std::lock_guard<std::mutex> lk(pool.mu);
            size_t best = pool.idle.size();
            for (size_t i = 0; i < pool.idle.size(); i++)       // the largest idle buffer of this device
                if (pool.idle[i].device == device && (best == pool.idle.size() || pool.idle[i].bytes > pool.idle[best].bytes)) best = i;
            if (best < pool.idle.size()) { r = pool.idle[best]; pool.idle.erase(pool.idle.begin() + best); }
        }
        r.device = device;
        if (!r.st) LC_HIP(hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking));
        if (r.bytes < bytes) {
            if (r.mem) { (void)hipFree(r.mem); r.mem = nullptr; r.bytes = 0; }
            const size_t want = bytes + bytes / 4;              // headroom: the next batch of about this size fits as well
            LC_HIP(hipMalloc(&r.mem, want));
            r.bytes = want;
        }
        st = r.st;
        mem = r.mem;
        return APK_OK;
    }
};
static inline size_t lc_align(size_t n) { return (n + 255) & ~(size_t)255; }

// host arrays in and out; seg = nb_segments + 1 offsets, seg[0] = 0, non-decreasing (the C-ABI checks)
template <class FRP, class FPP>
int g1_lincomb_segments_impl(int device, const void* points, const void* scalars, const uint64_t* seg, uint32_t nb_segments, void* out) {
    using Aff = Affine<FPP>;
    using Fr = Fe<FRP>;
    using Pt = XYZZ<FPP>;
    if (nb_segments == 0) return APK_OK;
    const uint64_t terms = seg[nb_segments];
    const size_t o_pts = 0, o_sc = o_pts + lc_align(terms * sizeof(Aff)), o_part = o_sc + lc_align(terms * sizeof(Fr)),
                 o_seg = o_part + lc_align(terms * LINCOMB_WINDOWS * sizeof(Pt)), o_out = o_seg + lc_align((nb_segments + 1) * 8),
                 total = o_out + lc_align(nb_segments * sizeof(Aff));
    LincombScope sc;
    int rc = sc.open(device, total);
    if (rc != APK_OK) return rc;
    uint8_t* base = (uint8_t*)sc.mem;
    if (terms) {
        LC_HIP(hipMemcpyAsync(base + o_pts, points, terms * sizeof(Aff), hipMemcpyHostToDevice, sc.st));
        LC_HIP(hipMemcpyAsync(base + o_sc, scalars, terms * sizeof(Fr), hipMemcpyHostToDevice, sc.st));
    }
    LC_HIP(hipMemcpyAsync(base + o_seg, seg, (nb_segments + 1) * 8, hipMemcpyHostToDevice, sc.st));
    if (terms) {
        // one wave per workgroup: the chains are latency-bound, so the waves are spread over as many CUs as there are
        const uint32_t lanes = (uint32_t)terms * LINCOMB_WINDOWS;
        lincomb_partial_kernel<FRP, FPP><<<(lanes + 63) / 64, 64, 0, sc.st>>>((const Aff*)(base + o_pts), (const Fr*)(base + o_sc), (uint32_t)terms,
                                                                                  (Pt*)(base + o_part));
        LC_HIP(hipGetLastError());
    }
    lincomb_reduce_kernel<FPP><<<nb_segments, 256, 0, sc.st>>>((const Pt*)(base + o_part), (const uint64_t*)(base + o_seg), nb_segments,
                                                                (Aff*)(base + o_out));
    LC_HIP(hipGetLastError());
    LC_HIP(hipMemcpyAsync(out, base + o_out, nb_segments * sizeof(Aff), hipMemcpyDeviceToHost, sc.st));
    LC_HIP(hipStreamSynchronize(sc.st));
    return APK_OK;
}

template <class FRP, class FPP, bool SUBGROUP>
int g1_check_points_impl(int device, const void* points, uint64_t count, uint8_t* flags) {
    using Aff = Affine<FPP>;
    if (count == 0) return APK_OK;
    const size_t o_flags = lc_align(count * sizeof(Aff));
    LincombScope sc;
    int rc = sc.open(device, o_flags + lc_align(count));
    if (rc != APK_OK) return rc;
    uint8_t* base = (uint8_t*)sc.mem;
    LC_HIP(hipMemcpyAsync(base, points, count * sizeof(Aff), hipMemcpyHostToDevice, sc.st));
    g1_check_kernel<FRP, FPP, SUBGROUP><<<(uint32_t)((count + 63) / 64), 64, 0, sc.st>>>((const Aff*)base, (uint32_t)count, base + o_flags);
    LC_HIP(hipGetLastError());
    LC_HIP(hipMemcpyAsync(flags, base + o_flags, count, hipMemcpyDeviceToHost, sc.st));
    LC_HIP(hipStreamSynchronize(sc.st));
    return APK_OK;
}

}  // namespace apk

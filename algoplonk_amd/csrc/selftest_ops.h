// One field / curve operation per call, for the test seams of include/apk.h (apk_host_* / apk_device_*): the SAME op bodies run
// on the host (apk_api.cpp, the portable C branches of ff.h / ffu.h / ec.h) and in a kernel (seam_run.h, the device branches:
// MacChain, the generated ffu_asm.h chains, the four-lane DPP point forms).  Nothing on the prove / MSM / NTT path calls these.
// Status codes instead of set_error(): the bodies are host+device; the C-ABI turns a non-zero status into its message.
#pragma once
#include <string.h>
#include <type_traits>

#include "ec.h"

namespace apk {

enum { SELFTEST_OK = 0, SELFTEST_UNKNOWN_OP = 1, SELFTEST_NO_UNSAT = 2 };

template <class P, class = void> struct HasUnsat : std::false_type {};
template <class P> struct HasUnsat<P, std::void_t<decltype(P::UL)>> : std::true_type {};

// field ops on gnark-radix Fe (include/apk.h apk_host_fe_op lists the codes)
template <class P>
APK_HD int fe_op_t(int op, const void* a, const void* b, void* out) {
    using F = Fe<P>;
    F x, y, r;
    memcpy(&x, a, sizeof x);
    if (b) memcpy(&y, b, sizeof y); else y = F::zero();
    switch (op) {
        case 0: r = F::add(x, y); break;
        case 1: r = F::sub(x, y); break;
        case 2: r = F::mul(x, y); break;
        case 3: r = F::inv(x); break;
        case 4: r = F::neg(x); break;
        // 10..13: the same operation carried out in the unsaturated-limb MSM field (ffu.h), converted in and out
        case 10: case 11: case 12: case 13:
            if constexpr (HasUnsat<P>::value) {
                using U = FeU<P>;
                U ux = U::from_fe(x), uy = U::from_fe(y);
                r = (op == 10 ? U::mul(ux, uy) : op == 11 ? U::add(ux, uy) : op == 12 ? U::sub(ux, uy) : U::neg(ux)).to_fe();
                break;
            } else {
                return SELFTEST_NO_UNSAT;
            }
        // 14: ten lazy butterfly stages as the NTT tile runs them (kernels_ntt.h): (u, v) <- (u + w v, u - w v + 2p) with the
        // twiddle w = y in the R' radix, no comparison until the final canon<16>; returns u
        case 14:
            if constexpr (HasUnsat<P>::value) {
                using U = FeU<P>;
                F ratio = F::zero();
                ratio.l[0] = 1u << (U::B * U::L - 32 * F::N);          // R'/R (2^5 for the 9 x 29-bit fields)
                const U w = U::unpack(F::mul(y, F::to_mont(ratio)).l);  // y * R'/R: gnark's radix -> R'
                U u = U::unpack(x.l), v = U::unpack(y.l);
                for (int i = 0; i < 10; i++) {
                    const U t = U::mul_nr(w, v);
                    const U nu = U::add_n(u, t);
                    v = U::template sub_k<2>(u, t);
                    u = nu;
                }
                U::template canon<16>(u).pack(r.l);
                break;
            } else {
                return SELFTEST_NO_UNSAT;
            }
        default: return SELFTEST_UNKNOWN_OP;
    }
    memcpy(out, &r, sizeof r);
    return SELFTEST_OK;
}

// Raw unsaturated-limb ops (FeU, ffu.h): no conversion, no packing.  A record is 4 operands of UL words (a, b, c, d) in, one
// record of UL words out (words past what the op writes are zero).  Codes: include/apk.h apk_host_feu_op.
template <class P>
APK_HD int feu_op_t(int op, const uint32_t* in, uint32_t* out) {
    if constexpr (HasUnsat<P>::value) {
        using U = FeU<P>;
        constexpr int L = U::L;
        U a, b, c, d, r = U::zero();
        for (int i = 0; i < L; i++) { a.l[i] = in[i]; b.l[i] = in[L + i]; c.l[i] = in[2 * L + i]; d.l[i] = in[3 * L + i]; }
        switch (op) {
            case 0: r = U::reduce_once(a); break;
            case 1: r = U::add(a, b); break;
            case 2: r = U::sub(a, b); break;
            case 3: r = U::neg(a); break;
            case 4: r = U::mul_nr(a, b); break;
            case 5: r = U::mul(a, b); break;
            case 6: r = U::sqr_nr(a); break;
            case 7: r = U::sqr(a); break;
            case 8: r = U::mul2_nr(a, b, c, d); break;
            case 9: r = U::add_n(a, b); break;
            case 10: r = U::triple_n(a); break;
            case 11: r = U::template sub2_k<4>(a, b, c); break;
            case 12: r = U::template sub_k<1>(a, b); break;
            case 13: r = U::template sub_k<2>(a, b); break;
            case 14: r = U::template sub_k<4>(a, b); break;
            case 15: r = U::template sub_k<6>(a, b); break;
            case 16: r = U::template neg_k<1>(a); break;
            case 17: r = U::template neg_k<2>(a); break;
            case 18: r = U::template neg_k<4>(a); break;
            case 19: r = U::template canon<1>(a); break;
            case 20: r = U::template canon<2>(a); break;
            case 21: r = U::template canon<4>(a); break;
            case 22: r = U::template canon<8>(a); break;
            case 23: r = U::template canon<16>(a); break;
            case 24: r = U::template canon<32>(a); break;
            case 25: r.l[0] = a.is_zero_mod_p() ? 1u : 0u; break;
            case 26: r = U::unpack(in); break;                   // in: N packed words
            case 27: a.pack(r.l); break;                          // out: N packed words
            case 28: { Fe<P> x; memcpy(&x, in, sizeof x); r = U::from_fe(x); break; }
            case 29: { const Fe<P> x = a.to_fe(); memcpy(r.l, &x, sizeof x); break; }
            // 40..47: the carry-save forms and the quotient-estimate reduction; 48: the limb factors the products accept
            case 40: r = U::add_s(a, b); break;
            case 41: r = U::template sub_s<2>(a, b); break;
            case 42: r = U::template neg_s<2>(a); break;
            case 43: r = U::template sub_n<2>(a, b); break;
            case 44: r = U::template reduce_2p<4>(a); break;
            case 45: r = U::template reduce_2p<8>(a); break;
            case 46: r = U::template reduce_2p<32>(a); break;
            case 47: r = U::template canon<1>(U::template reduce_2p<32>(a)); break;
            case 48:   // a.l[0..3] = limb factors fa, fb, fc, fd -> mul_takes(fa, fb), mul2_takes(fa, fb, fc, fd), sqr_takes(fa), COLUMN_ROOM
                r.l[0] = U::mul_takes(a.l[0], a.l[1]) ? 1u : 0u;
                r.l[1] = U::mul2_takes(a.l[0], a.l[1], a.l[2], a.l[3]) ? 1u : 0u;
                r.l[2] = U::sqr_takes(a.l[0]) ? 1u : 0u;
                r.l[3] = (uint32_t)U::COLUMN_ROOM;
                break;
            default: return SELFTEST_UNKNOWN_OP;
        }
        for (int i = 0; i < L; i++) out[i] = r.l[i];
        return SELFTEST_OK;
    } else {
        return SELFTEST_NO_UNSAT;
    }
}

// sv * v <= k * p for a limb-form value v (any limb sizes): the lazy point class's bounds as integers (5.1 p: sv = 10, k = 51)
template <class U>
APK_HD bool feu_scaled_le(const U& v, uint32_t sv, uint32_t k) {
    constexpr int L = U::L;
    uint64_t x[U::L], y[U::L], cx = 0, cy = 0;
    for (int i = 0; i < L; i++) {
        const uint64_t tx = (uint64_t)sv * v.l[i] + cx, ty = (uint64_t)k * U::template kp<1>(i) + cy;
        x[i] = i == L - 1 ? tx : (tx & U::MASK); cx = tx >> U::B;
        y[i] = i == L - 1 ? ty : (ty & U::MASK); cy = ty >> U::B;
    }
    for (int i = L - 1; i >= 0; i--)
        if (x[i] != y[i]) return x[i] < y[i];
    return true;
}
// ec.h's lazy class: X < 5.1p, Y <= 4p, ZZ, ZZZ < 1.4p, every limb but the top one normalised
template <class XU>
APK_HD bool in_lazy_class(const XU& pt) {
    using U = decltype(pt.X);
    for (int i = 0; i < U::L - 1; i++)
        if ((pt.X.l[i] | pt.Y.l[i] | pt.ZZ.l[i] | pt.ZZZ.l[i]) > U::MASK) return false;
    return feu_scaled_le(pt.X, 10, 51) && feu_scaled_le(pt.Y, 1, 4) && feu_scaled_le(pt.ZZ, 10, 14) && feu_scaled_le(pt.ZZZ, 10, 14);
}

constexpr int LAZY_CHAIN_STEPS = 320;

template <class FRP, class FPP>
APK_HD int g1_op_t(int op, const void* p, const void* q, void* out) {
    using A = Affine<FPP>;
    using X = XYZZ<FPP>;
    A a, b, r;
    memcpy(&a, p, sizeof a);
    switch (op) {
        case 0: {  // mixed add
            memcpy(&b, q, sizeof b);
            X acc = X::from_affine(a);
            acc.madd(b);
            r = acc.to_affine();
            break;
        }
        case 1: {  // full add through a non-trivial ZZ: (2a - a) + b
            memcpy(&b, q, sizeof b);
            X acc = X::dbl_affine(a);
            acc.madd(a, true);
            X other = X::dbl_affine(b);
            other.madd(b, true);
            acc.add(other);
            r = acc.to_affine();
            break;
        }
        case 2: r = X::dbl(X::from_affine(a)).to_affine(); break;
        case 3: {  // scalar multiplication, q = Fr scalar (Montgomery)
            Fe<FRP> s;
            memcpy(&s, q, sizeof s);
            s = Fe<FRP>::from_mont(s);
            X acc = X::inf();
            for (int w = Fe<FRP>::N - 1; w >= 0; w--)
                for (int bit = 31; bit >= 0; bit--) {
                    acc = X::dbl(acc);
                    if ((s.l[w] >> bit) & 1u) acc.madd(a);
                }
            r = acc.to_affine();
            break;
        }
        case 12: case 13: {  // a fixed chain of signed mixed additions through every special case: lazy (12) / plain (13)
            using XU = XYZZ<FPP, FeU<FPP>>;
            memcpy(&b, q, sizeof b);
            const Affine<FPP, FeU<FPP>> pa = unpack_affine<FPP>(to_table_record<FPP>(a)), pb = unpack_affine<FPP>(to_table_record<FPP>(b)),
                                        pinf = Affine<FPP, FeU<FPP>>::inf();
            // a, 2a (doubling), a, inf (cancellation), b, 2b, 2b+a, 3b+a, 3b, 2b, b, skip, a+b, a+2b, a+3b, 3b, a+3b
            constexpr int script[17][2] = {{0, 0}, {0, 0}, {0, 1}, {0, 1}, {1, 0}, {1, 0}, {0, 0}, {1, 0}, {0, 1}, {1, 1}, {1, 1},
                                           {2, 0}, {0, 0}, {1, 0}, {1, 0}, {0, 1}, {0, 0}};
            XU acc = XU::inf();
            bool flipped = false, unit_z = false;
            for (const auto& st : script) {
                const auto& pt = st[0] == 0 ? pa : st[0] == 1 ? pb : pinf;
                if (op == 12) acc.madd_lazy(pt, st[1] != 0, flipped, unit_z); else acc.madd(pt, st[1] != 0);
            }
            if (op == 12) { acc.lazy_fix_sign(flipped); acc.canonicalize(); }
            r = to_fe_point<FPP>(acc).to_affine();
            break;
        }
        case 14: {  // lazy full addition / doubling through the special cases: ends at 4p + 6q
            using XU = XYZZ<FPP, FeU<FPP>>;
            memcpy(&b, q, sizeof b);
            const Affine<FPP, FeU<FPP>> pa = unpack_affine<FPP>(to_table_record<FPP>(a)), pb = unpack_affine<FPP>(to_table_record<FPP>(b));
            XU x1 = XU::dbl_lazy(XU::from_affine(pa));          // 2a
            x1.add_lazy(XU::from_affine(pb));                    // 2a + b
            XU x2 = XU::dbl_lazy(XU::dbl_lazy(XU::from_affine(pb)));   // 4b
            x2.add_lazy(x1);                                     // 2a + 5b
            XU x3 = x2;
            x3.add_lazy(x2);                                     // equal operands: 4a + 10b
            XU x4 = x2; x4.lazy_neg();
            x3.add_lazy(x4);                                     // 2a + 5b
            XU x5 = x3; x5.lazy_neg();
            x3.add_lazy(x5);                                     // cancellation: infinity
            x3.add_lazy(XU::inf());
            x3.add_lazy(x1);                                     // 2a + b
            x3.add_lazy(x2);                                     // 4a + 6b
            r = to_fe_point<FPP>(x3).to_affine();
            break;
        }
        case 15: {  // LAZY_CHAIN_STEPS signed mixed additions through madd_lazy, the lazy class checked after every step
            // Step i adds +-q_i, q_i = a + i b, with the sign alternating for i < 160 and in runs of 16 after that, except:
            //   i = 0, 2, 3: +a (3: a doubling under unit_z);  i = 1: -a (a cancellation under unit_z);
            //   i = 200: minus the state itself (cancellation with ZZ != 1);  i = 260: plus the state itself (doubling, ZZ != 1).
            // Returns the final point; an all-ones record if a state left the lazy class, or was infinite when the plain chain
            // (XYZZ::madd on canonical values) was not.
            using XU = XYZZ<FPP, FeU<FPP>>;
            memcpy(&b, q, sizeof b);
            A cur = a;
            XU acc = XU::inf(), plain = XU::inf();
            bool flipped = false, unit_z = false, ok = true;
            for (int i = 0; i < LAZY_CHAIN_STEPS; i++) {
                A pt = cur;
                bool negate = i < 160 ? (i & 1) != 0 : ((i >> 4) & 1) != 0;
                if (i < 4) { pt = a; negate = i == 1; }
                if ((i == 200 || i == 260) && !plain.is_inf()) { pt = to_fe_point<FPP>(plain).to_affine(); negate = i == 200; }
                const Affine<FPP, FeU<FPP>> pu = unpack_affine<FPP>(to_table_record<FPP>(pt));
                acc.madd_lazy(pu, negate, flipped, unit_z);
                plain.madd(pu, negate);
                ok = ok && in_lazy_class(acc) && acc.is_inf() == plain.is_inf();
                X nx = X::from_affine(cur);
                nx.madd(b);
                cur = nx.to_affine();
            }
            acc.lazy_fix_sign(flipped);
            r = to_fe_point<FPP>(acc).to_affine();
            if (!ok) memset(&r, 0xff, sizeof r);
            break;
        }
        case 10: case 11: {  // mixed (10) / full (11) addition in the unsaturated-limb representation
            using XU = XYZZ<FPP, FeU<FPP>>;
            memcpy(&b, q, sizeof b);
            Affine<FPP> ra = to_table_record<FPP>(a), rb = to_table_record<FPP>(b);
            XU acc = op == 10 ? XU::from_affine(unpack_affine<FPP>(ra)) : XU::dbl_affine(unpack_affine<FPP>(ra));
            if (op == 11) acc.madd(unpack_affine<FPP>(ra), true);
            if (op == 10) {
                acc.madd(unpack_affine<FPP>(rb));
            } else {
                XU other = XU::dbl_affine(unpack_affine<FPP>(rb));
                other.madd(unpack_affine<FPP>(rb), true);
                acc.add(other);
            }
            r = to_fe_point<FPP>(acc).to_affine();
            break;
        }
        default: return SELFTEST_UNKNOWN_OP;
    }
    memcpy(out, &r, sizeof r);
    return SELFTEST_OK;
}

#if defined(__HIPCC__)
// ops 20 / 21 (device only): the four-lane point forms of the MSM tails (ec.h add_quad_general / dbl_quad_general), called by the
// four lanes (q = 0..3) of a quad together; every lane writes its own result.  The operands enter the lazy class through lazy
// operations (2a - a: dbl_lazy, lazy_neg, add_lazy), so ZZ != 1 and Y may exceed p.  The caller's rules are kept: an infinite
// operand is a copy (the quad forms never see it); a degenerate pair (a = +-b) is REPORTED as an all-ones record, never a point.
template <class FRP, class FPP>
__device__ __forceinline__ int g1_quad_op_t(int op, int q, const void* p, const void* qq, void* out) {
    using A = Affine<FPP>;
    using XU = XYZZ<FPP, FeU<FPP>>;
    A a, b, r;
    memcpy(&a, p, sizeof a);
    auto lazy = [](const A& pt) -> XU {
        const XU one = XU::from_affine(unpack_affine<FPP>(to_table_record<FPP>(pt)));
        XU x = XU::dbl_lazy(one), m = one;
        m.lazy_neg();
        x.add_lazy(m);
        return x;
    };
    XU acc = lazy(a);
    if (op == 20) {
        memcpy(&b, qq, sizeof b);
        const XU o = lazy(b);
        if (acc.is_inf()) acc = o;
        else if (!o.is_inf()) {
            bool degenerate;
            acc.add_quad_general(o, q, degenerate);
            if (degenerate) { memset(out, 0xff, sizeof r); return SELFTEST_OK; }
        }
    } else if (op == 21) {
        if (!acc.is_inf()) acc = XU::dbl_quad_general(acc, q);
    } else {
        return SELFTEST_UNKNOWN_OP;
    }
    r = to_fe_point<FPP>(acc).to_affine();
    memcpy(out, &r, sizeof r);
    return SELFTEST_OK;
}
#endif

}  // namespace apk

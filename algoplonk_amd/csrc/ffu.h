// Base-field arithmetic on UNSATURATED limbs for the MSM point arithmetic (gfx950).
//
// Why: with saturated 32-bit limbs every 32x32 partial product needs a v_mad_u64_u32 (4.6 cycles per wave) AND a
// v_addc_co_u32 (4.0 cycles) to keep the carry out of the 64-bit column accumulator (tools/ubench/valu_rates.hip).
// With UL limbs of UB < 32 bits (BN254: 9 x 29, BLS12-381: 14 x 28) a whole column of 2*UL partial products fits a
// 64-bit accumulator, so the Montgomery product is a bare chain of v_mad_u64_u32 plus one 64-bit shift per column:
// ~35 % fewer issue cycles per product, and plain C++ (the same code runs on the host for the CPU-only tests).
//
// Three tiers of operations, each closed under its own contract:
//   * canonical (add, sub, neg, mul, sqr): 0 <= x < p and every limb < 2^UB after every operation, so the plain point formulas
//     and their special-case tests are unchanged;
//   * lazy ("lazy forms" below: *_nr, *_k, *_n, canon<K>, reduce_2p<K>): values only congruent mod p and bounded by a stated
//     multiple of p, limbs still normalised (every limb but the top one < 2^UB) - no conditional subtraction;
//   * carry-save ("carry-save forms" below: add_s, sub_s, neg_s): limbs up to a stated small multiple of 2^UB, for values whose
//     only readers are products (which absorb the carries in their 64-bit columns) or a swept sum.  The limb factors a product
//     accepts are mul_takes / mul2_takes / sqr_takes, derived from UL and UB.
// The Montgomery radix is R' = 2^(UB*UL), not gnark's R = 2^(32N): FeU values never leave the MSM pipeline (windowed
// tables are internal data; results are converted back with to_fe()).
//
// Replaces (device side) gnark-crypto v0.20.1 ecc/<curve>/fp element arithmetic inside G1Affine.MultiExp
// [UPSTREAM, not vendored; reached from /root/reference/algoplonk.go:89 via kzg.Commit].
#pragma once
#include "ff.h"
#include "ffu_asm.h"

template <class P>
struct FeU {
    static constexpr int L = P::UL;
    static constexpr int B = P::UB;
    static constexpr uint32_t MASK = (1u << B) - 1u;
    static constexpr int N = P::N;  // saturated 32-bit words of the packed form
    uint32_t l[L];

    APK_HD static FeU zero() {
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) r.l[i] = 0;
        return r;
    }
    APK_HD static FeU one() {
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) r.l[i] = P::uone(i);
        return r;
    }
    APK_HD bool is_zero() const {
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < L; i++) acc |= l[i];
        return acc == 0;
    }
    APK_HD bool operator==(const FeU& o) const {
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < L; i++) acc |= l[i] ^ o.l[i];
        return acc == 0;
    }
    APK_HD bool operator!=(const FeU& o) const { return !(*this == o); }

    // x in [0, 2p) with normalised limbs -> [0, p)
    APK_HD static FeU reduce_once(const FeU& a) {
        FeU d;
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = a.l[i] - P::umod(i) - borrow;  // wraps when negative: bit 31 set (operands < 2^30)
            borrow = t >> 31;
            d.l[i] = t & MASK;
        }
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) r.l[i] = borrow ? a.l[i] : d.l[i];
        return r;
    }

    APK_HD static FeU add(const FeU& a, const FeU& b) {
        FeU s;
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = a.l[i] + b.l[i] + carry;
            carry = t >> B;
            s.l[i] = t & MASK;
        }
        // a + b < 2p < 2^(B*L): the last carry is zero (top limb keeps its spare bits)
        return reduce_once(s);
    }

    APK_HD static FeU sub(const FeU& a, const FeU& b) {
        FeU d;
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = a.l[i] - b.l[i] - borrow;
            borrow = t >> 31;
            d.l[i] = t & MASK;
        }
        // negative: add p back (the wrapped limbs represent a - b + 2^(B*L); adding p and dropping the top carry fixes it)
        const uint32_t m = 0u - borrow;
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = d.l[i] + (P::umod(i) & m) + carry;
            carry = t >> B;
            d.l[i] = t & MASK;
        }
        return d;
    }

    APK_HD static FeU neg(const FeU& a) {
        if (a.is_zero()) return a;
        FeU d;
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = P::umod(i) - a.l[i] - borrow;
            borrow = t >> 31;
            d.l[i] = t & MASK;
        }
        return d;
    }

    APK_HD static FeU dbl(const FeU& a) { return add(a, a); }

    // Montgomery product a*b/R' mod p, product scanning.  Column k collects a_i*b_(k-i) and m_i*p_(k-i): at most 2L
    // products below 2^(2B) plus a carry below 2^(64-B) - no overflow, no carry flag.  For canonical inputs the result
    // is below p + p*p/R' < 2p and is brought to [0, p) by one conditional subtraction (left out by mul_nr, see the
    // lazy forms below; operands with larger limbs: mul_takes, "carry-save forms").  The generated chain (UMulAsm, BN254 Fp)
    // multiplies the operand words as they are, full 32 bits each, like this code: it accepts the same limb factors.  Its
    // square doubles the operand with a 32-bit shift, like sqr_nr: sqr_takes.
    APK_HD static FeU mul_nr(const FeU& a, const FeU& b) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (UMulAsm<P>::available) { FeU r; UMulAsm<P>::mul(r.l, a.l, b.l); return r; }   // one strict mad chain (ffu_asm.h)
#endif
        uint32_t m[L];
        FeU r;
        uint64_t acc = 0;
#pragma unroll
        for (int k = 0; k < L; k++) {
#pragma unroll
            for (int i = 0; i <= k; i++) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
            for (int i = 0; i < k; i++) acc += (uint64_t)m[i] * P::umod(k - i);
            m[k] = ((uint32_t)acc * P::UINV) & MASK;
            acc += (uint64_t)m[k] * P::umod(0);
            acc >>= B;
        }
#pragma unroll
        for (int k = L; k < 2 * L - 1; k++) {
#pragma unroll
            for (int i = k - L + 1; i < L; i++) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
            for (int i = k - L + 1; i < L; i++) acc += (uint64_t)m[i] * P::umod(k - i);
            r.l[k - L] = (uint32_t)acc & MASK;
            acc >>= B;
        }
        r.l[L - 1] = (uint32_t)acc;
        return r;
    }
    APK_HD static FeU mul(const FeU& a, const FeU& b) { return reduce_once(mul_nr(a, b)); }

    // a*a/R': the off-diagonal partial products are taken once against 2a (L*(L+1)/2 mads instead of L*L)
    APK_HD static FeU sqr_nr(const FeU& a) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (UMulAsm<P>::available) { FeU r; UMulAsm<P>::sqr(r.l, a.l); return r; }
#endif
        uint32_t m[L], d[L];
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) d[i] = a.l[i] << 1;   // < 2^(B+1): products stay below 2^(2B+1), column sums below 2^63
        uint64_t acc = 0;
#pragma unroll
        for (int k = 0; k < L; k++) {
#pragma unroll
            for (int i = 0; 2 * i < k; i++) acc += (uint64_t)d[i] * a.l[k - i];
            if ((k & 1) == 0) acc += (uint64_t)a.l[k / 2] * a.l[k / 2];
#pragma unroll
            for (int i = 0; i < k; i++) acc += (uint64_t)m[i] * P::umod(k - i);
            m[k] = ((uint32_t)acc * P::UINV) & MASK;
            acc += (uint64_t)m[k] * P::umod(0);
            acc >>= B;
        }
#pragma unroll
        for (int k = L; k < 2 * L - 1; k++) {
#pragma unroll
            for (int i = k - L + 1; 2 * i < k; i++) acc += (uint64_t)d[i] * a.l[k - i];
            if ((k & 1) == 0) acc += (uint64_t)a.l[k / 2] * a.l[k / 2];
#pragma unroll
            for (int i = k - L + 1; i < L; i++) acc += (uint64_t)m[i] * P::umod(k - i);
            r.l[k - L] = (uint32_t)acc & MASK;
            acc >>= B;
        }
        r.l[L - 1] = (uint32_t)acc;
        return r;
    }
    APK_HD static FeU sqr(const FeU& a) { return reduce_once(sqr_nr(a)); }

    // ---- lazy forms: the bucket-accumulation inner loop (ec.h XYZZ::madd_lazy) --------------------------------------
    // R'/p is large (BN254: 169, BLS12-381: 2520), so a Montgomery product of operands below A*p and C*p comes out
    // below p*(1 + A*C*p/R') < 2p without the conditional subtraction as long as A*C <= HEADROOM = R'/p, and a difference can
    // be kept positive by adding a multiple of p instead of testing for a borrow.  Values are then only congruent mod p
    // (still with every limb but the top one below 2^B); canon<K>() brings them back.  Column sums stay below 2^64:
    // 2L products of limbs below 2^B plus L of m*p, or L products with one operand's limbs below 2^(B+1).
    static constexpr uint32_t HEADROOM = (uint32_t)((1ull << B) / ((uint64_t)P::umod(L - 1) + 1));   // <= R'/p; users assert what they need
    static_assert((uint64_t)(3 * L + 1) <= (1ull << (64 - 2 * B)), "column sums of mul2_nr must fit 64 bits");

    // limb i of K*p, normalised (the top limb keeps the excess)
    template <uint32_t K>
    APK_HD static constexpr uint32_t kp(int i) {
        uint64_t carry = 0;
        uint32_t limb = 0;
        for (int j = 0; j <= i; j++) {
            uint64_t t = (uint64_t)K * P::umod(j) + carry;
            limb = j == L - 1 ? (uint32_t)t : (uint32_t)(t & MASK);
            carry = t >> B;
        }
        return limb;
    }

    // a - b + K*p through a signed carry sweep: no comparison, limbs come out normalised.  Needs b <= K*p as values and
    // limbs below 2^30; the result is below a + K*p.
    template <uint32_t K>
    APK_HD static FeU sub_k(const FeU& a, const FeU& b) {
        FeU r;
        int32_t carry = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            int32_t t = (int32_t)(a.l[i] - b.l[i] + kp<K>(i)) + carry;
            carry = t >> B;   // arithmetic shift: a negative limb borrows from the next one
            r.l[i] = i == L - 1 ? (uint32_t)t : ((uint32_t)t & MASK);
        }
        return r;
    }
    // K*p - a
    template <uint32_t K>
    APK_HD static FeU neg_k(const FeU& a) {
        FeU r;
        int32_t carry = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            int32_t t = (int32_t)(kp<K>(i) - a.l[i]) + carry;
            carry = t >> B;
            r.l[i] = i == L - 1 ? (uint32_t)t : ((uint32_t)t & MASK);
        }
        return r;
    }
    // a + b and 3a with an unsigned carry sweep (limbs normalised again; values just add up)
    APK_HD static FeU add_n(const FeU& a, const FeU& b) {
        FeU r;
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = a.l[i] + b.l[i] + carry;
            carry = t >> B;
            r.l[i] = i == L - 1 ? t : (t & MASK);
        }
        return r;
    }
    APK_HD static FeU triple_n(const FeU& a) {
        FeU r;
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = (a.l[i] << 1) + a.l[i] + carry;
            carry = t >> B;
            r.l[i] = i == L - 1 ? t : (t & MASK);
        }
        return r;
    }
    // a - b - 2c + K*p, same conventions (needs b + 2c <= K*p)
    template <uint32_t K>
    APK_HD static FeU sub2_k(const FeU& a, const FeU& b, const FeU& c) {
        FeU r;
        int32_t carry = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            int32_t t = (int32_t)(a.l[i] - ((c.l[i] << 1) + b.l[i]) + kp<K>(i)) + carry;
            carry = t >> B;
            r.l[i] = i == L - 1 ? (uint32_t)t : ((uint32_t)t & MASK);
        }
        return r;
    }

    // ---- carry-save forms: sums and differences whose ONLY readers absorb the carries ---------------------------------
    // A product does not need normalised limbs.  Column k of mul_nr sums at most L terms a_i * b_(k-i), L terms m_i * p_(k-i)
    // (m and p always below 2^B) and the carry of the column before.  With every limb of a below fa * 2^B and every limb of b
    // below fb * 2^B the column stays below (L fa fb + L + 1) * 2^(2B), the carry of a column below (L fa fb + L + 1) * 2^B,
    // so the 64-bit accumulator holds it as long as L fa fb + L + 1 <= 2^(64 - 2B) = COLUMN_ROOM.  The product is then
    // (a b + m p) / R' with m = -a b / p mod R' - a function of the VALUES a and b only, limbs normalised below the top one:
    // bit for bit what the swept operands give.  BN254 (L = 9, B = 29) has room for 64, BLS12-381 Fp (14, 28) for 256.
    // A "limb factor" f below means: every limb is below f * 2^B (1 = normalised; the top limb of a value below HEADROOM * p
    // is below 2^B in any form, because the lower limbs are never negative).  The swept forms (add_n, sub_k, ...) take
    // carry-save operands as long as their 32-bit limb sums fit, which their callers state.
    static constexpr uint64_t COLUMN_ROOM = 1ull << (64 - 2 * B);
    APK_HD static constexpr bool mul_takes(uint64_t fa, uint64_t fb) {
        return (uint64_t)L * fa * fb + L + 1 <= COLUMN_ROOM && (fa << B) <= (1ull << 32) && (fb << B) <= (1ull << 32);
    }
    APK_HD static constexpr bool mul2_takes(uint64_t fa, uint64_t fb, uint64_t fc, uint64_t fd) {
        return (uint64_t)L * (fa * fb + fc * fd) + L + 1 <= COLUMN_ROOM && mul_takes(fa, fb) && mul_takes(fc, fd);
    }
    // the squares read both factors from one value (f * f per term) and double it into 32 bits: they keep swept inputs
    APK_HD static constexpr bool sqr_takes(uint64_t f) { return mul_takes(f, f) && (f << (B + 1)) <= (1ull << 32); }
    static_assert(mul_takes(1, 1) && mul2_takes(1, 1, 1, 1) && sqr_takes(1), "normalised operands must fit");

    APK_HD static constexpr uint32_t add_s_factor(uint32_t fa, uint32_t fb) { return fa + fb; }
    APK_HD static constexpr uint32_t sub_s_factor(uint32_t fa, uint32_t fb) { return fa + fb + 1; }
    APK_HD static constexpr uint32_t neg_s_factor(uint32_t fb) { return fb + 1; }

    // limb i of K*p in the REDUNDANT form the carry-save differences subtract from: every limb lends FB units to the limb below
    // it, so each lower limb is at least FB * 2^B - 1 - the largest limb of a subtrahend of limb factor FB - and limb-wise
    // differences never go negative.  The top limb is FB short of K*p's; see sub_s for why that is enough.
    template <uint32_t K, uint32_t FB>
    APK_HD static constexpr uint32_t kp_s(int i) {
        uint32_t v = kp<K>(i);
        if (i < L - 1) v += FB << B;
        if (i > 0) v -= FB;
        return v;
    }
    template <uint32_t K, uint32_t FB>
    APK_HD static constexpr bool kp_s_valid() {
        for (int i = 1; i < L - 1; i++)
            if (kp<K>(i) + 1u < FB) return false;       // kp_s(i) >= FB * 2^B - 1
        return kp<K>(L - 1) >= FB && ((uint64_t)(FB + 1) << B) <= (1ull << 32);
    }

    // a + b, limb by limb: limb factor add_s_factor(fa, fb)
    APK_HD static FeU add_s(const FeU& a, const FeU& b) {
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) r.l[i] = a.l[i] + b.l[i];
        return r;
    }
    // a - b + K*p, limb by limb, for b of limb factor FB (and b <= K*p as values): limb factor sub_s_factor(fa, FB).
    // The lower limbs cannot go negative (kp_s).  The top limb is (value - lower limbs) / 2^(B(L-1)) and the lower limbs
    // weigh less than (fa + FB + 1) * 2^(B(L-1)) = (fa + FB + 1) * p / (top limb of p): it cannot go negative where the VALUE
    // a - b + K*p is at least that small fraction of p (BN254: p / 2^19), which every call site states.
    template <uint32_t K, uint32_t FB = 1>
    APK_HD static FeU sub_s(const FeU& a, const FeU& b) {
        static_assert(kp_s_valid<K, FB>(), "K*p has a limb too small to lend FB units");
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) r.l[i] = a.l[i] - b.l[i] + kp_s<K, FB>(i);
        return r;
    }
    // K*p - a, same conventions: limb factor neg_s_factor(FB); needs K*p - a >= (FB + 1) * p / (top limb of p)
    template <uint32_t K, uint32_t FB = 1>
    APK_HD static FeU neg_s(const FeU& a) {
        static_assert(kp_s_valid<K, FB>(), "K*p has a limb too small to lend FB units");
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) r.l[i] = kp_s<K, FB>(i) - a.l[i];
        return r;
    }
    // a - b + K*p with normalised limbs for a CARRY-SAVE a: sub_s followed by an unsigned sweep (sub_k's signed 32-bit limb
    // sums overflow from limb factor 3 on at B = 29; this form takes a limb factor up to 2^(32-B) - 3).  b normalised; same
    // value condition as sub_s.
    template <uint32_t K>
    APK_HD static FeU sub_n(const FeU& a, const FeU& b) {
        static_assert(kp_s_valid<K, 1>(), "K*p has a limb too small to lend one unit");
        FeU r;
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = a.l[i] - b.l[i] + kp_s<K, 1>(i) + carry;    // < (fa + 2) * 2^B + carry <= 2^32 for fa <= 2^(32-B) - 3
            carry = t >> B;
            r.l[i] = i == L - 1 ? t : (t & MASK);
        }
        return r;
    }

    // (a*b + c*d)/R' with ONE Montgomery reduction; below p + (a*b + c*d)/R'
    APK_HD static FeU mul2_nr(const FeU& a, const FeU& b, const FeU& c, const FeU& d) {
        uint32_t m[L];
        FeU r;
        uint64_t acc = 0;
#pragma unroll
        for (int k = 0; k < L; k++) {
#pragma unroll
            for (int i = 0; i <= k; i++) {
                acc += (uint64_t)a.l[i] * b.l[k - i];
                acc += (uint64_t)c.l[i] * d.l[k - i];
            }
#pragma unroll
            for (int i = 0; i < k; i++) acc += (uint64_t)m[i] * P::umod(k - i);
            m[k] = ((uint32_t)acc * P::UINV) & MASK;
            acc += (uint64_t)m[k] * P::umod(0);
            acc >>= B;
        }
#pragma unroll
        for (int k = L; k < 2 * L - 1; k++) {
#pragma unroll
            for (int i = k - L + 1; i < L; i++) {
                acc += (uint64_t)a.l[i] * b.l[k - i];
                acc += (uint64_t)c.l[i] * d.l[k - i];
            }
#pragma unroll
            for (int i = k - L + 1; i < L; i++) acc += (uint64_t)m[i] * P::umod(k - i);
            r.l[k - L] = (uint32_t)acc & MASK;
            acc >>= B;
        }
        r.l[L - 1] = (uint32_t)acc;
        return r;
    }

    // value below 2K*p (K a power of two), limbs normalised -> [0, p)
    template <uint32_t K>
    APK_HD static FeU canon(const FeU& a) {
        FeU d;
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            uint32_t t = a.l[i] - kp<K>(i) - borrow;
            borrow = t >> 31;
            d.l[i] = i == L - 1 ? t : (t & MASK);
        }
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) r.l[i] = borrow ? a.l[i] : d.l[i];
        if constexpr (K > 1) return canon<K / 2>(r);
        else return r;
    }
    // limb i of 2^(B L) - p, every limb normalised (the subtraction below adds multiples of it and drops the carry out)
    APK_HD static constexpr uint32_t cmod(int i) {
        uint32_t carry = 1, limb = 0;
        for (int j = 0; j <= i; j++) {
            const uint32_t t = (MASK - P::umod(j)) + carry;
            limb = t & MASK;
            carry = t >> B;
        }
        return limb;
    }
    // value below 2K*p, limbs normalised -> the same value mod p in [0, 2p), limbs normalised: one estimate of the multiple of
    // p from the top limb, one multiply-add per limb, one sweep.  With W = 2^(B(L-1)), T = (top limb of p) + 1 and a = t W + low:
    //   q = floor(t * floor(2^S / T) / 2^S) <= t / T <= t W / p <= a / p           (p < T W): q never overestimates,
    //   a / p - q < 1 + (2K + 1) / (T - 1) + 2K T / 2^S <= 2                        (a < (t + 1) W, p >= (T - 1) W, t < 2K T),
    // so a - q p is in [0, 2p).  It is computed as a + q (2^(BL) - p) with the carry out of the top limb dropped - all unsigned;
    // the top limb of a value below 2p has B bits.  canon<1> after it gives canon<K>(a).
    template <uint32_t K>
    APK_HD static FeU reduce_2p(const FeU& a) {
        constexpr uint32_t T = P::umod(L - 1) + 1;
        constexpr int S = 62 - __builtin_clz(T);               // 31 + floor(log2 T): 2^S / T fits 32 bits
        constexpr uint32_t C = (uint32_t)((1ull << S) / T);
        static_assert(4ull * (2 * K + 1) <= T - 1 && (uint64_t)2 * K * T <= (1ull << (S - 2)), "the estimate must stay within one of the quotient");
        static_assert((uint64_t)2 * K * T <= (1ull << 32), "the top limb of the input must fit its word");
        const uint32_t q = (uint32_t)(((uint64_t)a.l[L - 1] * C) >> S);
        FeU r;
        uint64_t acc = 0;
#pragma unroll
        for (int i = 0; i < L; i++) {
            acc += (uint64_t)q * cmod(i) + a.l[i];
            r.l[i] = (uint32_t)acc & MASK;
            acc >>= B;
        }
        return r;
    }
    // for a value below 2p with normalised limbs: is it 0 mod p?
    APK_HD bool is_zero_mod_p() const {
        uint32_t z = 0, e = 0;
#pragma unroll
        for (int i = 0; i < L; i++) { z |= l[i]; e |= l[i] ^ P::umod(i); }
        return z == 0 || e == 0;
    }

    // ---- packed (saturated, N x 32-bit) <-> limbs.  The packed form is what sits in HBM (tables, results). ----
    APK_HD static FeU unpack(const uint32_t* w) {
        FeU r;
#pragma unroll
        for (int i = 0; i < L; i++) {
            const int bit = i * B, j = bit >> 5, s = bit & 31;
            uint32_t v = j < N ? (w[j] >> s) : 0u;
            if (s + B > 32 && j + 1 < N) v |= w[j + 1] << (32 - s);
            r.l[i] = v & MASK;
        }
        return r;
    }
    APK_HD void pack(uint32_t* w) const {
#pragma unroll
        for (int j = 0; j < N; j++) {
            uint32_t v = 0;
#pragma unroll
            for (int i = 0; i < L; i++) {
                const int lo = i * B - j * 32;  // position of limb i's bit 0 inside word j
                if (lo > -B && lo < 32) v |= lo >= 0 ? (l[i] << lo) : (l[i] >> (-lo));
            }
            w[j] = v;
        }
    }

    // gnark-Montgomery Fe (x*R, R = 2^(32N))  <->  FeU (x*R')
    APK_HD static FeU from_fe(const Fe<P>& x) {
        FeU c;
#pragma unroll
        for (int i = 0; i < L; i++) c.l[i] = P::uconv_in(i);
        return mul(unpack(x.l), c);
    }
    APK_HD Fe<P> to_fe() const {
        FeU c;
#pragma unroll
        for (int i = 0; i < L; i++) c.l[i] = P::uconv_out(i);
        FeU y = mul(*this, c);
        Fe<P> r;
        y.pack(r.l);
        return r;
    }
};

template <class P> APK_HD FeU<P> operator+(const FeU<P>& a, const FeU<P>& b) { return FeU<P>::add(a, b); }
template <class P> APK_HD FeU<P> operator-(const FeU<P>& a, const FeU<P>& b) { return FeU<P>::sub(a, b); }
template <class P> APK_HD FeU<P> operator*(const FeU<P>& a, const FeU<P>& b) { return FeU<P>::mul(a, b); }

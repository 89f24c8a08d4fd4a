"""Big-integer reference model of the unsaturated-limb field arithmetic (algoplonk_amd/csrc/ffu.h FeU) and its contracts.

A FeU value is L limbs of B bits, radix 2^B, Montgomery radix R' = 2^(B*L); every limb but the top one is below 2^B, the top
one may carry the excess of a lazily reduced value.  For each op of the raw-limb seam (include/apk.h apk_host_feu_op) this
module states the PRECONDITION - the input class the comment in ffu.h / ec.h / kernels_ntt.h gives - as a generator of edge
and random operands, and the POSTCONDITION as three checks on the result:
  1. its value is congruent to the exact big-integer result mod p (or equal to it, for the exact limb-wise forms);
  2. its value is below the bound the comment states;
  3. every limb but the top one is below 2^B.
"""
from __future__ import annotations

import ctypes as C
import random
from dataclasses import dataclass
from math import isqrt
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from algoplonk_amd import _lib


@dataclass(frozen=True)
class Field:
    curve: int          # C-ABI curve id
    field: int          # 0 = Fr, 1 = Fp
    p: int
    L: int              # limbs
    B: int              # bits per limb
    H: int              # HEADROOM as the library states it (ffu.h)
    N: int              # 32-bit words of the packed / gnark form

    @property
    def Rp(self) -> int:            # R' = 2^(B L), the limb form's Montgomery radix
        return 1 << (self.B * self.L)

    @property
    def R(self) -> int:             # R = 2^(32 N), gnark's radix (ff.h Fe)
        return 1 << (32 * self.N)

    @property
    def mask(self) -> int:
        return (1 << self.B) - 1

    def __str__(self) -> str:
        return "%s.%s" % ({0: "bn254", 1: "bls12-381"}[self.curve], "Fp" if self.field else "Fr")


def field(cv, fld: int) -> Field:
    ul, ub, hr = C.c_int(), C.c_int(), C.c_uint32()
    _lib.check(_lib.lib.apk_feu_shape(cv.abi, fld, C.byref(ul), C.byref(ub), C.byref(hr)))
    p = cv.p if fld else cv.r
    n = (cv.fp_bytes if fld else 32) // 4
    return Field(cv.abi, fld, p, ul.value, ub.value, hr.value, n)


# ---- limb codec (vectorised over records) ----------------------------------------------------------------------------------
def encode(f: Field, values: Sequence[int]) -> np.ndarray:
    """values -> (n, L) uint32 limbs; lower limbs below 2^B, the top limb takes the rest (must fit 32 bits)."""
    lo_bits = f.B * (f.L - 1)
    nbytes = (lo_bits + 32 + 7) // 8
    for v in values:
        assert 0 <= v and v >> lo_bits < 1 << 32, "value does not fit the limb form"
    raw = np.frombuffer(b"".join(v.to_bytes(nbytes, "little") for v in values), dtype=np.uint8).reshape(len(values), nbytes)
    bits = np.unpackbits(raw, axis=1, bitorder="little").astype(np.uint64)
    out = np.zeros((len(values), f.L), dtype=np.uint32)
    for i in range(f.L):
        w = f.B if i < f.L - 1 else 32
        out[:, i] = (bits[:, f.B * i: f.B * i + w] << np.arange(w, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return out


def random_limbs(f: Field, hi: int, n: int, rng: np.random.Generator) -> np.ndarray:
    """n values drawn inside [0, hi] directly as limbs (no big integers): the random bulk of the bit-for-bit comparisons."""
    lo_bits = f.B * (f.L - 1)
    top = hi >> lo_bits
    out = rng.integers(0, 1 << f.B, size=(n, f.L), dtype=np.uint64).astype(np.uint32)
    out[:, f.L - 1] = rng.integers(0, max(top, 1), size=n, dtype=np.uint64).astype(np.uint32)
    return out


def decode(f: Field, limbs: np.ndarray) -> List[int]:
    """(n, L) limbs -> values (limb i weighs 2^(B i), whatever its size)."""
    limbs = np.asarray(limbs, dtype=np.uint64)
    weights = [1 << (f.B * i) for i in range(f.L)]
    cols = [limbs[:, i].tolist() for i in range(f.L)]
    return [sum(c[j] * w for c, w in zip(cols, weights)) for j in range(limbs.shape[0])]


def words(f: Field, values: Sequence[int]) -> np.ndarray:
    """values below 2^(32 N) -> (n, L) records holding the N little-endian 32-bit words (the packed / gnark form)."""
    out = np.zeros((len(values), f.L), dtype=np.uint32)
    for j, v in enumerate(values):
        out[j, : f.N] = np.frombuffer(v.to_bytes(4 * f.N, "little"), dtype="<u4")
    return out


def unwords(f: Field, recs: np.ndarray) -> List[int]:
    return [int.from_bytes(np.ascontiguousarray(r[: f.N]).astype("<u4").tobytes(), "little") for r in recs]


# ---- the ops: precondition (input class), exact result, stated bound --------------------------------------------------------
@dataclass
class Op:
    name: str
    code: int
    arity: int
    # classes(f) -> list of operand bounds tuples: each operand i is drawn from [0, bound_i]  (inclusive maxima)
    classes: Callable[[Field], List[Tuple[int, ...]]]
    # expect(f, operands) -> (target, exact, bound): the result must equal target (exact) or be congruent to it mod p,
    # and be below `bound`
    expect: Callable[[Field, Tuple[int, ...]], Tuple[int, bool, int]]
    io: str = "limbs"         # "limbs" | "words_in" (operand a is N packed words) | "words_out" | "flag"
    valid: Optional[Callable[[Field, Tuple[int, ...]], bool]] = None   # extra joint precondition


def _canon(f):   # canonical operands
    return [(f.p - 1,) * 4]


def _prod_classes(f: Field, arity: int) -> List[Tuple[int, ...]]:
    """mul_nr / mul: a < A p, b < C p with A C <= HEADROOM - the class maximum and the splits in between."""
    H = f.H
    out = []
    for A in sorted({1, 2, 4, 7, isqrt(H), H // 7, H // 4, H // 2, H}):
        Cc = H // A
        if A >= 1 and Cc >= 1:
            out.append((A * f.p - 1, Cc * f.p - 1, 0, 0))
    return out


def _sqr_classes(f: Field, arity: int) -> List[Tuple[int, ...]]:
    A = isqrt(f.H)
    return [(1 * f.p - 1, 0, 0, 0), (2 * f.p - 1, 0, 0, 0), (A * f.p - 1, 0, 0, 0)]


def _mul2_classes(f: Field, arity: int) -> List[Tuple[int, ...]]:
    H, p = f.H, f.p
    # A1 C1 + A2 C2 <= H: the lazy class's uses (R < 3.1p, T < 7.1p, Y <= 4p, PPP < 1.1p) and the extremes
    return [(p - 1, (H - 1) * p - 1, p - 1, p - 1), (3 * p, 7 * p, 4 * p, 2 * p - 1),
            ((H // 2) * p - 1, p - 1, (H // 2) * p - 1, p - 1), (isqrt(H // 2) * p - 1,) * 4]


def _lazy_cap(f: Field) -> int:
    """largest value the exact limb-wise forms take as an operand: H p (< R'), limbs normalised."""
    return f.H * f.p - 1


def _exact(v, bound):
    return v, True, bound


OPS: List[Op] = [
    Op("reduce_once", 0, 1, lambda f: [(2 * f.p - 1,)], lambda f, x: (x[0], False, f.p)),
    Op("add", 1, 2, _canon, lambda f, x: (x[0] + x[1], False, f.p)),
    Op("sub", 2, 2, _canon, lambda f, x: (x[0] - x[1], False, f.p)),
    Op("neg", 3, 1, _canon, lambda f, x: (-x[0], False, f.p)),
    # below p + a b / R' (< 2p in the class): bound checked exactly as (result - p) R' < a b
    Op("mul_nr", 4, 2, lambda f: _prod_classes(f, 2),
       lambda f, x: (x[0] * x[1] * pow(f.Rp, -1, f.p), False, min(2 * f.p, f.p + -(-x[0] * x[1] // f.Rp)))),
    Op("mul", 5, 2, lambda f: _prod_classes(f, 2), lambda f, x: (x[0] * x[1] * pow(f.Rp, -1, f.p), False, f.p)),
    Op("sqr_nr", 6, 1, lambda f: _sqr_classes(f, 1),
       lambda f, x: (x[0] * x[0] * pow(f.Rp, -1, f.p), False, min(2 * f.p, f.p + -(-x[0] * x[0] // f.Rp)))),
    Op("sqr", 7, 1, lambda f: _sqr_classes(f, 1), lambda f, x: (x[0] * x[0] * pow(f.Rp, -1, f.p), False, f.p)),
    Op("mul2_nr", 8, 4, lambda f: _mul2_classes(f, 4),
       lambda f, x: ((x[0] * x[1] + x[2] * x[3]) * pow(f.Rp, -1, f.p), False,
                     min(2 * f.p, f.p + -(-(x[0] * x[1] + x[2] * x[3]) // f.Rp))),
       valid=lambda f, x: x[0] * x[1] + x[2] * x[3] <= f.H * f.p * f.p),
    Op("add_n", 9, 2, lambda f: [(_lazy_cap(f), _lazy_cap(f))], lambda f, x: _exact(x[0] + x[1], x[0] + x[1] + 1)),
    Op("triple_n", 10, 1, lambda f: [(_lazy_cap(f),)], lambda f, x: _exact(3 * x[0], 3 * x[0] + 1)),
    # a - b - 2c + 4p, needs b + 2c <= 4p
    Op("sub2_k<4>", 11, 3, lambda f: [((f.H - 4) * f.p - 1, 4 * f.p, 0), ((f.H - 4) * f.p - 1, 2 * f.p, f.p),
                                      ((f.H - 4) * f.p - 1, 0, 2 * f.p)],
       lambda f, x: _exact(x[0] - x[1] - 2 * x[2] + 4 * f.p, x[0] + 4 * f.p + 1), valid=lambda f, x: x[1] + 2 * x[2] <= 4 * f.p),
] + [
    # a - b + K p, needs b <= K p; below a + K p
    Op("sub_k<%d>" % K, code, 2, (lambda K: lambda f: [((f.H - K) * f.p - 1, K * f.p)])(K),
       (lambda K: lambda f, x: _exact(x[0] - x[1] + K * f.p, x[0] + K * f.p + 1))(K))
    for K, code in ((1, 12), (2, 13), (4, 14), (6, 15))
] + [
    Op("neg_k<%d>" % K, code, 1, (lambda K: lambda f: [(K * f.p,)])(K), (lambda K: lambda f, x: _exact(K * f.p - x[0], K * f.p + 1))(K))
    for K, code in ((1, 16), (2, 17), (4, 18))
] + [
    # a value below 2 K p -> [0, p)
    Op("canon<%d>" % K, code, 1, (lambda K: lambda f: [(2 * K * f.p - 1,)])(K), lambda f, x: (x[0], False, f.p))
    for K, code in ((1, 19), (2, 20), (4, 21), (8, 22), (16, 23), (32, 24))
] + [
    Op("is_zero_mod_p", 25, 1, lambda f: [(2 * f.p - 1,)], lambda f, x: (int(x[0] % f.p == 0), True, 2), io="flag"),
    Op("unpack", 26, 1, lambda f: [(min(f.R, f.Rp) - 1,)], lambda f, x: _exact(x[0], f.Rp), io="words_in"),
    Op("pack", 27, 1, lambda f: [(min(f.R, f.Rp) - 1,)], lambda f, x: _exact(x[0], f.R), io="words_out"),
    # gnark radix (x = X R) in, X R' out; and back (the operand may be anywhere in the lazy class: to_fe_point takes it as it is)
    Op("from_fe", 28, 1, lambda f: [(f.p - 1,)], lambda f, x: (x[0] * pow(f.R, -1, f.p) * f.Rp, False, f.p), io="words_in"),
    Op("to_fe", 29, 1, lambda f: [(_lazy_cap(f),)], lambda f, x: (x[0] * pow(f.Rp, -1, f.p) * f.R, False, f.p), io="words_out"),
]
OPS_BY_NAME: Dict[str, Op] = {o.name: o for o in OPS}


# ---- input generator --------------------------------------------------------------------------------------------------------
def edge_values(f: Field, hi: int) -> List[int]:
    """Edges of [0, hi]: 0, 1, k p - 1, k p, k p + 1 for every k the class allows, hi itself, the largest value <= hi whose
    lower limbs are all MASK, and 2^(B i), 2^(B i) - 1."""
    p, lo_bits = f.p, f.B * (f.L - 1)
    vals = {0, 1, 2, hi, hi - 1}
    kmax = (hi + 1) // p
    # every k up to 64 (the NTT's and the lazy point class's multiples), then powers of two and the top three
    ks = set(range(1, min(kmax, 64) + 1)) | {1 << j for j in range(kmax.bit_length())} | {kmax - 2, kmax - 1, kmax, kmax + 1}
    for k in ks:
        if k >= 1:
            vals.update({k * p - 1, k * p, k * p + 1})
    top = hi >> lo_bits
    for t in (top, top - 1):
        v = (t << lo_bits) | ((1 << lo_bits) - 1)
        if 0 <= v <= hi:
            vals.add(v)
            break
    for i in range(1, f.L + 1):
        vals.update({(1 << (f.B * i)) - 1, 1 << (f.B * i)})
    if hi >= 32 * p:       # the top limb at the extremes of a wide class
        vals.update({hi - p, hi // 2, hi // 2 + 1})
    return sorted(v for v in vals if 0 <= v <= hi)


def _key_edges(f: Field, edges: List[int]) -> List[int]:
    """a handful of an operand's edges: both ends, p - 1, p, the all-MASK value and the middle"""
    hi = edges[-1]
    pick = [0, 1, f.p - 1, f.p, hi, hi - 1, hi // 2]
    lo_bits = f.B * (f.L - 1)
    pick += [v for v in edges if v & ((1 << lo_bits) - 1) == (1 << lo_bits) - 1][-1:]
    return sorted({v for v in pick if 0 <= v <= hi})


def _fits(f: Field, op: Op, x: Tuple[int, ...]) -> bool:
    return op.valid is None or op.valid(f, x)


def operands(f: Field, op: Op, n_random: int, seed: int) -> List[Tuple[int, ...]]:
    """Edge operands of every class of the op (cross products of the per-operand edges, thinned for 3- and 4-ary ops) plus
    `n_random` uniform draws from the classes."""
    rnd = random.Random(seed)
    out: List[Tuple[int, ...]] = []
    for cls in op.classes(f):
        bounds = cls[: op.arity]
        edges = [edge_values(f, b) for b in bounds]
        if op.arity == 1:
            out += [(a,) for a in edges[0]]
        else:
            # every edge of each operand against the key edges of the others (the full cross product is too large)
            keys = [_key_edges(f, e) for e in edges]
            for i in range(op.arity):
                for v in edges[i]:
                    for j in range(len(keys[0])):
                        out.append(tuple(v if k == i else keys[k][(j + k) % len(keys[k])] for k in range(op.arity)))
            out += [tuple(e[-1] for e in edges), tuple(e[0] for e in edges)]
    per = max(1, n_random // max(1, len(op.classes(f))))
    for cls in op.classes(f):
        bounds = cls[: op.arity]
        for _ in range(per):
            out.append(tuple(rnd.randint(0, b) for b in bounds))
    # joint preconditions (mul2_nr's sum of products, sub2_k's b + 2c): scale the draws that leave the class back into it
    fixed = []
    for x in out:
        while not _fits(f, op, x):
            x = tuple(v // 2 for v in x)
        fixed.append(x)
    return fixed


def pack_records(f: Field, op: Op, xs: List[Tuple[int, ...]]) -> np.ndarray:
    """operands -> the seam's input records: (n, 4 L) uint32"""
    rec = np.zeros((len(xs), 4, f.L), dtype=np.uint32)
    for i in range(op.arity):
        col = [x[i] for x in xs]
        rec[:, i, :] = words(f, col) if op.io == "words_in" and i == 0 else encode(f, col)
    return rec.reshape(len(xs), 4 * f.L)


def run(f: Field, op: Op, recs: np.ndarray, device: Optional[int] = None) -> np.ndarray:
    """one seam call over all records: host (device None) or GPU `device`; returns (n, L) uint32"""
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    out = np.zeros((recs.shape[0], f.L), dtype=np.uint32)
    if device is None:
        rc = _lib.lib.apk_host_feu_op(f.curve, f.field, op.code, recs.shape[0], recs.ctypes.data, out.ctypes.data)
    else:
        rc = _lib.lib.apk_device_feu_op(f.curve, f.field, op.code, device, recs.shape[0], recs.ctypes.data, out.ctypes.data)
    _lib.check(rc)
    return out


def violations(f: Field, op: Op, xs: List[Tuple[int, ...]], out: np.ndarray, limit: int = 5) -> List[str]:
    """The postcondition on every record; returns (at most `limit`) descriptions of the records that break it."""
    bad: List[str] = []
    if op.io == "words_out":
        vals = unwords(f, out)
        limbs_ok = [True] * len(xs)
    elif op.io == "flag":
        vals = [int(r[0]) for r in out]
        limbs_ok = [not r[1:].any() for r in out]
    else:
        vals = decode(f, out)
        limbs_ok = (out[:, : f.L - 1] <= f.mask).all(axis=1).tolist()
    for x, v, lok in zip(xs, vals, limbs_ok):
        target, exact, bound = op.expect(f, x)
        why = None
        if exact and v != target:
            why = "value %#x != exact result %#x" % (v, target)
        elif not exact and (v - target) % f.p:
            why = "value %#x is not congruent to the result mod p" % v
        elif not v < bound:
            why = "value %#x = %.4f p is not below the stated bound %.4f p" % (v, v / f.p, bound / f.p)
        elif not lok:
            why = "a lower limb is not below 2^%d" % f.B
        if why:
            bad.append("%s %s(%s): %s" % (f, op.name, ", ".join("%#x" % a for a in x[: op.arity]), why))
            if len(bad) >= limit:
                break
    return bad


# ---- the NTT tile's lazy butterflies (kernels_ntt.h) ------------------------------------------------------------------------
def _mont_nr(a: int, b: int, p: int, Rp: int, pinv: int) -> int:
    """mul_nr as a value: (a b + m p) / R' with m = -a b p^-1 mod R' (what the limb-serial product computes)"""
    t = a * b
    return (t + (t * pinv % Rp) * p) // Rp


def lazy_ntt(ov, log_n: int, words: Sequence[int], inverse: bool = False) -> List[int]:
    """The radix-2 pass kernel's values before its final canon<K>, for a natural-order input of gnark-radix words (forward
    or inverse, no coset / scaling): bit-reversed gather, stage 0 without a product, then u + mul_nr(w R', v) and
    u - mul_nr(w R', v) + 2p.  Values only - the limb layout does not change them."""
    p, Rp, n = ov.r, 1 << 261, 1 << log_n
    pinv = -pow(p, -1, Rp) % Rp
    w = ov.omega(n)
    if inverse:
        w = pow(w, -1, p)
    tw = [pow(w, j, p) * Rp % p for j in range(n // 2)]
    a = [words[int(format(i, "0%db" % log_n)[::-1], 2)] for i in range(n)]
    for t in range(log_n):
        h = 1 << t
        for blk in range(0, n, 2 * h):
            for j in range(h):
                u, v = a[blk + j], a[blk + j + h]
                if t:
                    v = _mont_nr(tw[j * (n // (2 * h))], v, p, Rp, pinv)
                a[blk + j], a[blk + j + h] = u + v, u - v + 2 * p
    return a


def ntt_top_growth_input(ov, log_n: int, inverse: bool = False) -> List[int]:
    """gnark-radix words that drive the LAST output of the lazy NTT as close to its stated bound as the arithmetic allows.

    That output takes the difference u - t + 2p at every stage, its u chain starting at input 0, and t at stage s is the
    product of the stage's twiddle w_s with the top value V_s of the size-2^s sub-transform over bit-reversed block
    [2^s, 2^(s+1)) - disjoint blocks, so each t is set on its own: a block holding one word c (a delta) has V_s = c mod p, and
    c = delta_s / w_s makes t = delta_s when delta_s exceeds w_s R' V_s / R' (mul_nr returns a value below p + w_s R' V_s / R',
    so delta_s + p is out of reach); delta_s is taken just above that for any V_s below (2 + 2s) p.  (A product of a value
    congruent to 0 returns p, not 0: zeros do not do it.)  The output grows by ~2p - delta_s per stage and passes 32p from
    2^17 on; a plain input grows by ~p per stage, a random one by ~1.5p."""
    p, Rp, n = ov.r, 1 << 261, 1 << log_n
    w = ov.omega(n)
    if inverse:
        w = pow(w, -1, p)
    x = [0] * n
    x[0] = p - 1
    for s in range(1, log_n):
        ws = pow(w, ((1 << s) - 1) * (n >> (s + 1)), p)
        delta = -(-(ws * Rp % p) * (2 + 2 * s) * p // Rp) + 1     # > w_s R' V_s / R' for any V_s below (2 + 2s) p
        x[n >> (s + 1)] = delta * pow(ws, -1, p) % p                 # lands at bit-reversed position 2^s
    return x

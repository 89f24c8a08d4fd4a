"""Big-integer model of the carry-save forms of algoplonk_amd/csrc/ffu.h (add_s, sub_s, neg_s, sub_n, reduce_2p) and of the
column budget that says which limb sizes a product accepts.  Limbs are plain Python integers here: a value is a list of L limbs,
limb i weighing 2^(B i), of any size.  tests/limb_model.py holds the Field description and the seam plumbing.

Limb factor f of a value: every limb is below f * 2^B (1 = normalised)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

import limb_model as lm

# seam codes (include/apk.h apk_host_feu_op)
OP_MUL_NR, OP_SQR_NR, OP_MUL2_NR, OP_ADD_N = 4, 6, 8, 9
OP_CANON = {1: 19, 2: 20, 4: 21, 8: 22, 16: 23, 32: 24}
OP_ADD_S, OP_SUB_S2, OP_NEG_S2, OP_SUB_N2 = 40, 41, 42, 43
OP_REDUCE_2P = {4: 44, 8: 45, 32: 46}
OP_REDUCE_CANON32, OP_TAKES = 47, 48


# ---- the column budget --------------------------------------------------------------------------------------------------------
def column_room(f: lm.Field) -> int:
    """how many terms of 2^(2B) a 64-bit column accumulator holds"""
    return 1 << (64 - 2 * f.B)


def _fits_word(f: lm.Field, fa: int) -> bool:
    return (fa << f.B) <= 1 << 32


def mul_takes(f: lm.Field, fa: int, fb: int) -> bool:
    """L terms a_i b_j below fa fb 2^(2B), L terms m_i p_j below 2^(2B), and a carry below the column count * 2^B"""
    return f.L * fa * fb + f.L + 1 <= column_room(f) and _fits_word(f, fa) and _fits_word(f, fb)


def mul2_takes(f: lm.Field, fa: int, fb: int, fc: int, fd: int) -> bool:
    return f.L * (fa * fb + fc * fd) + f.L + 1 <= column_room(f) and mul_takes(f, fa, fb) and mul_takes(f, fc, fd)


def sqr_takes(f: lm.Field, fa: int) -> bool:
    return mul_takes(f, fa, fa) and (fa << (f.B + 1)) <= 1 << 32


def add_s_factor(fa: int, fb: int) -> int:
    return fa + fb


def sub_s_factor(fa: int, fb: int) -> int:
    return fa + fb + 1


def neg_s_factor(fb: int) -> int:
    return fb + 1


# ---- limbs ------------------------------------------------------------------------------------------------------------------------
def value(f: lm.Field, limbs: Sequence[int]) -> int:
    return sum(int(v) << (f.B * i) for i, v in enumerate(limbs))


def normalised(f: lm.Field, v: int) -> List[int]:
    """the swept form: lower limbs below 2^B, the top limb takes the rest"""
    assert v >= 0
    return [(v >> (f.B * i)) & f.mask for i in range(f.L - 1)] + [v >> (f.B * (f.L - 1))]


def kp_s(f: lm.Field, K: int, FB: int = 1) -> List[int]:
    """K p in the redundant form the differences subtract from: every limb lends FB units to the limb below it"""
    out = normalised(f, K * f.p)
    for i in range(f.L):
        if i < f.L - 1:
            out[i] += FB << f.B
        if i > 0:
            out[i] -= FB
    assert value(f, out) == K * f.p
    assert all(out[i] >= (FB << f.B) - 1 for i in range(f.L - 1)) and out[-1] >= 0, "K p has a limb too small to lend FB units"
    return out


def add_s(f: lm.Field, a: Sequence[int], b: Sequence[int]) -> List[int]:
    return [x + y for x, y in zip(a, b)]


def sub_s(f: lm.Field, K: int, a: Sequence[int], b: Sequence[int], FB: int = 1) -> List[int]:
    return [x - y + k for x, y, k in zip(a, b, kp_s(f, K, FB))]


def neg_s(f: lm.Field, K: int, a: Sequence[int], FB: int = 1) -> List[int]:
    return [k - x for x, k in zip(a, kp_s(f, K, FB))]


def sub_n(f: lm.Field, K: int, a: Sequence[int], b: Sequence[int]) -> List[int]:
    return normalised(f, value(f, a) - value(f, b) + K * f.p)


def min_value_for_top(f: lm.Field, factor: int) -> int:
    """A limb-wise difference of limb factor `factor` keeps its top limb non-negative when its VALUE is at least this: the lower
    limbs weigh less than factor * 2^(B (L-1))."""
    return factor << (f.B * (f.L - 1))


# ---- the quotient-estimate reduction ------------------------------------------------------------------------------------------------
def estimate_constants(f: lm.Field):
    T = (f.p >> (f.B * (f.L - 1))) + 1
    S = 31 + T.bit_length() - 1
    return T, S, (1 << S) // T


def estimate(f: lm.Field, top: int) -> int:
    _, S, Cst = estimate_constants(f)
    return (top * Cst) >> S


def reduce_2p(f: lm.Field, limbs: Sequence[int]) -> List[int]:
    """a - q p for the estimate q taken from the top limb; normalised"""
    v = value(f, limbs)
    r = v - estimate(f, int(limbs[-1])) * f.p
    assert 0 <= r
    return normalised(f, r)


def estimate_boundaries(f: lm.Field, K: int) -> List[int]:
    """top limbs at which the estimate steps: for every q up to 2K the smallest top limb with estimate q, and the one below it"""
    T, S, Cst = estimate_constants(f)
    out = set()
    for q in range(1, 2 * K + 1):
        t = -(-(q << S) // Cst)             # smallest t with t * Cst >= q 2^S
        assert estimate(f, t) == q and estimate(f, t - 1) == q - 1
        out.update({t - 1, t})
    return sorted(out)


# ---- seam plumbing ------------------------------------------------------------------------------------------------------------------
def records(f: lm.Field, rows: Sequence[Sequence[Sequence[int]]]) -> np.ndarray:
    """rows of up to four limb vectors -> the seam's (n, 4 L) input records"""
    rec = np.zeros((len(rows), 4, f.L), dtype=np.uint32)
    for j, ops in enumerate(rows):
        for i, limbs in enumerate(ops):
            assert all(0 <= v < 1 << 32 for v in limbs), "a limb does not fit its word"
            rec[j, i, :] = np.array(list(limbs), dtype=np.uint64).astype(np.uint32)
    return rec.reshape(len(rows), 4 * f.L)


def run(f: lm.Field, code: int, recs: np.ndarray, device=None) -> np.ndarray:
    op = lm.Op("op%d" % code, code, 4, lambda f: [], lambda f, x: (0, True, 0))
    return lm.run(f, op, recs, device=device)


def all_max(f: lm.Field, factor: int, top: int) -> List[int]:
    """every lower limb at the largest size of limb factor `factor`, the top limb as given"""
    return [(factor << f.B) - 1] * (f.L - 1) + [top]


def top_only(f: lm.Field, top: int) -> List[int]:
    return [0] * (f.L - 1) + [top]


def top_below(f: lm.Field, bound: int, lower: int) -> int:
    """largest top limb for which a value with `lower` as its lower part stays below `bound`"""
    return (bound - 1 - lower) >> (f.B * (f.L - 1))

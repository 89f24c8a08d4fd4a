"""Big-integer model of the recovery of a polynomial from a sufficient set of its cells (include/apk.h apk_kzg_recover_cosets;
csrc/kernels_kzg_recover.h), over any prime r with a domain of n points.

The domain has n points and generator w; l = 2^k is the coset size, n' = n / l, a_i = w^(i l); coset i < n' holds
x_(i,j) = w^(i + n' j), j < l.  g is the coset shift, g^n != 1.  K = the known coset indices, rows[r] = the l values of coset K[r]
(row r of apk_kzg_open_cosets' out_values), M = the other m = n' - k cosets.

  steps()       (1) zH[t] = prod_{i in M} (a_t - a_i),  zG[t] = prod_{i in M} (g^l a_t - a_i)
                (2) E[i + n' j] = rows_i[j] zH[i] for i in K, 0 for i in M
                (3) P = IDFT_n(E)        (4) PG[q] = P(g w^q)        (5) Q[q] = PG[q] / zG[q mod n']
                (6) f_c = g^(-c) IDFT_n(Q)_c                                             - all n coefficients
  recover()     the first len of them, or None when one in [len, k l) is non-zero (APK_ERR_VERIFY)
  lagrange()    the independent witness: the polynomial below degree k l through the k l points, by Lagrange's formula
  plan()        the integer rules of csrc/kzg_recover_plan.h restated: the verdict, the row map, the missing cosets, the launches
"""
from __future__ import annotations

from typing import List, Optional, Sequence

OK, ERR_ARG, ERR_VERIFY = 0, 1, 5       # include/apk.h
THREADS = TILE = 256                    # csrc/kzg_recover_plan.h
MAX_COSETS = 1 << 16


def ntt(vec: Sequence[int], w: int, r: int) -> List[int]:
    """out[i] = sum_c vec[c] w^(i c); len(vec) a power of two, w a generator of that domain"""
    n = len(vec)
    if n == 1:
        return list(vec)
    even, odd = ntt(vec[0::2], w * w % r, r), ntt(vec[1::2], w * w % r, r)
    out, tw = [0] * n, 1
    for i in range(n // 2):
        x = odd[i] * tw % r
        out[i], out[i + n // 2] = (even[i] + x) % r, (even[i] - x) % r
        tw = tw * w % r
    return out


def intt(vec: Sequence[int], w: int, r: int) -> List[int]:
    n_inv = pow(len(vec), -1, r)
    return [x * n_inv % r for x in ntt(vec, pow(w, -1, r), r)]


def cells(f: Sequence[int], n: int, l: int, w: int, r: int) -> List[List[int]]:
    """the n' cells of f: cells[i][j] = f(w^(i + n' j))"""
    v = ntt(list(f) + [0] * (n - len(f)), w, r)
    return [[v[i + (n // l) * j] for j in range(l)] for i in range(n // l)]


def steps(n: int, l: int, known: Sequence[int], rows: Sequence[Sequence[int]], w: int, g: int, r: int) -> List[int]:
    np = n // l
    missing = [i for i in range(np) if i not in set(known)]
    a = [pow(w, i * l, r) for i in range(np)]
    gl = pow(g, l, r)
    zh, zg = [1] * np, [1] * np
    for t in range(np):
        for i in missing:
            zh[t] = zh[t] * (a[t] - a[i]) % r
            zg[t] = zg[t] * (gl * a[t] - a[i]) % r
    assert all(zg) and [t for t in range(np) if zh[t] == 0] == missing
    e = [0] * n
    for row, i in zip(rows, known):
        for j in range(l):
            e[i + np * j] = row[j] * zh[i] % r
    p = intt(e, w, r)
    pg = ntt([c * pow(g, k, r) % r for k, c in enumerate(p)], w, r)
    q = [x * pow(zg[k % np], -1, r) % r for k, x in enumerate(pg)]
    g_inv = pow(g, -1, r)
    return [c * pow(g_inv, k, r) % r for k, c in enumerate(intt(q, w, r))]


def recover(n: int, l: int, known: Sequence[int], rows: Sequence[Sequence[int]], length: int, w: int, g: int, r: int) -> Optional[List[int]]:
    f = steps(n, l, known, rows, w, g, r)
    return None if any(f[length:len(known) * l]) else f[:length]


def lagrange(n: int, l: int, known: Sequence[int], rows: Sequence[Sequence[int]], w: int, r: int) -> List[int]:
    """k l coefficients, by the plain formula: sum_p y_p prod_{q != p} (X - x_q) / (x_p - x_q)"""
    np = n // l
    xs = [pow(w, i + np * j, r) for i in known for j in range(l)]
    ys = [v for row in rows for v in row]
    full = [1]                                   # prod_q (X - x_q)
    for x in xs:
        full = [((full[c - 1] if c else 0) - x * (full[c] if c < len(full) else 0)) % r for c in range(len(full) + 1)]
    out = [0] * len(xs)
    for x, y in zip(xs, ys):
        quo, carry = [0] * len(xs), 0            # full / (X - x), synthetic division from the top
        for c in reversed(range(len(xs))):
            carry = (full[c + 1] + carry * x) % r
            quo[c] = carry
        den = 1
        for x2 in xs:
            if x2 != x:
                den = den * (x - x2) % r
        s = y * pow(den, -1, r) % r
        out = [(o + s * c) % r for o, c in zip(out, quo)]
    return out


def plan(n: int, l: int, indices: Sequence[int], length: int) -> dict:
    """csrc/kzg_recover_plan.h: recover_check_call, then recover_plan - the first rule that fails decides"""
    count = len(indices)
    bad = {"rc": ERR_ARG}
    if count == 0 or length == 0 or l < 2 or l & (l - 1):
        return bad
    if l > n // 2:
        return bad
    np = n // l
    if count > np or any(i >= np for i in indices) or len(set(indices)) != count or length > count * l or np > MAX_COSETS:
        return bad
    row_of = [-1] * np
    for row, i in enumerate(indices):
        row_of[i] = row
    m = np - count

    def launch(lanes, lds):
        return [lanes, -(-lanes // THREADS), THREADS, lds]

    return {"rc": OK, "np": np, "k": count, "m": m, "row_of": row_of, "missing": [i for i in range(np) if row_of[i] < 0],
            "vanish": launch(2 * np, TILE * 32), "scatter": launch(n, 0), "divide": launch(n, 0), "tiles": -(-m // TILE),
            "check": [length, count * l]}

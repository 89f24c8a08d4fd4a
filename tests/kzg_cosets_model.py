"""Big-integer model of the openings of one polynomial on every coset of its domain (include/apk.h apk_kzg_open_cosets;
csrc/kernels_kzg_cosets.h), in the exponent with a known tau: a G1 point [x]G1 is the scalar x.

The domain has n points and generator w; l = 2^k is the coset size, 2 <= l <= n / 2, n' = n / l; w_2n generates the size-2n
domain and w_2n' = w_2n^l; s_j = tau^j; f has len <= n coefficients, padded with zeros.  Coset i < n' holds
x_(i,j) = w^(i + n' j), j < l, which all satisfy x^l = a_i = w^(i l).

  (1) direct()        H_i = (f - I_i)(tau) / (tau^l - a_i),  I_i = f mod (X^l - a_i) = sum_{c<l} X^c sum_m a_i^m f_(c + l m)
  (2) by_transform()  H_i = sum_{m <= n'-2} (w^l)^(i m) h_m,  h_m = sum_j f_(j + l(m+1)) s_j,  h_(n'-1) = 0        (h_terms)
  (3) arrangement()   for c < l:  a_c = (f_(c+l), f_(c+2l) .. f_(c+l(n'-1)), 0 x (n'+1)),
                                  t_c = (s_(c+l(n'-2)) .. s_(c+l), s_c, 0 x (n'+1))                     (length 2n' each)
                      P^_i = sum_c DFT_2n'(a_c)_i DFT_2n'(t_c)_i,  cc = IDFT_2n'(P^),  h_m = cc[m + n' - 2]
                      (the highest SRS index used is n - l - 1)
  (4) a_hat_split()   DFT_2n'(a_c)_(2i) = NTT_n'(a_c)_i,  DFT_2n'(a_c)_(2i+1) = NTT_n'(a_c[u] w_2n'^u)_i     (first n' entries of a_c)
  (5) composition()   H_i = sum_{j<l} x_(i,j) / (l a_i) H^(1)_(i + n' j),  H^(1) = the single-point openings (kzg_all_model.direct)
  (6) accepts()       (C - I_i(tau) + a_i H_i) - tau^l H_i == 0,  I_i's coefficient c = w^(-i c) IDFT_l(values)_c
                      (IDFT_l with generator w^(n'), the values in the order j = 0 .. l-1)                 (interpolate)
"""
from __future__ import annotations

from typing import List, Sequence

from kzg_all_model import dft, direct as direct_single, horner, idft, padded


def coset_points(n: int, l: int, i: int, w: int, r: int) -> List[int]:
    return [pow(w, i + (n // l) * j, r) for j in range(l)]


def values_by_coset(f: Sequence[int], n: int, l: int, w: int, r: int) -> List[int]:
    """out[i l + j] = f(w^(i + n' j)): the layout of apk_kzg_open_cosets' out_values"""
    v = [horner(f, pow(w, k, r), r) for k in range(n)]
    return [v[i + (n // l) * j] for i in range(n // l) for j in range(l)]


def remainder(f: Sequence[int], n: int, l: int, a: int, r: int) -> List[int]:
    """f mod (X^l - a): l coefficients"""
    f = padded(f, n)
    out = []
    for c in range(l):
        acc = 0
        for m in reversed(range(n // l)):
            acc = (acc * a + f[c + l * m]) % r
        out.append(acc)
    return out


def direct(f: Sequence[int], n: int, l: int, w: int, tau: int, r: int) -> List[int]:
    ft, tl = horner(f, tau, r), pow(tau, l, r)
    out = []
    for i in range(n // l):
        a = pow(w, i * l, r)
        assert (tl - a) % r
        out.append((ft - horner(remainder(f, n, l, a, r), tau, r)) * pow((tl - a) % r, -1, r) % r)
    return out


def h_terms(f: Sequence[int], n: int, l: int, tau: int, r: int) -> List[int]:
    """h_m = sum_j f_(j + l(m+1)) tau^j for m <= n' - 2, and h_(n'-1) = 0"""
    f = padded(f, n)
    return [horner(f[l * (m + 1):], tau, r) for m in range(n // l - 1)] + [0]


def by_transform(f: Sequence[int], n: int, l: int, w: int, tau: int, r: int) -> List[int]:
    return dft(h_terms(f, n, l, tau, r), pow(w, l, r), r)


def sequences(f: Sequence[int], n: int, l: int, c: int, tau: int, r: int):
    """(a_c, t_c): the two sequences of length 2n'"""
    f = padded(f, n)
    np = n // l
    a = [f[c + l * (u + 1)] for u in range(np - 1)] + [0] * (np + 1)
    t = [pow(tau, c + l * (np - 2 - u), r) for u in range(np - 1)] + [0] * (np + 1)
    assert all(c + l * (np - 2 - u) <= n - l - 1 for u in range(np - 1))
    return a, t


def t_hat(n: int, l: int, c: int, w_2n: int, tau: int, r: int) -> List[int]:
    """T^_c = DFT_2n'(t_c), in the exponent: what apk_kzg_cosets_prepare keeps"""
    np = n // l
    t = [pow(tau, c + l * (np - 2 - u), r) for u in range(np - 1)] + [0] * (np + 1)
    return dft(t, pow(w_2n, l, r), r)


def p_hat(f: Sequence[int], n: int, l: int, w_2n: int, tau: int, r: int) -> List[int]:
    np2 = 2 * (n // l)
    w_2np = pow(w_2n, l, r)
    acc = [0] * np2
    for c in range(l):
        a, t = sequences(f, n, l, c, tau, r)
        a_hat, th = dft(a, w_2np, r), dft(t, w_2np, r)
        acc = [(x + y * z) % r for x, y, z in zip(acc, a_hat, th)]
    return acc


def arrangement(f: Sequence[int], n: int, l: int, w_2n: int, tau: int, r: int) -> List[int]:
    np = n // l
    cc = idft(p_hat(f, n, l, w_2n, tau, r), pow(w_2n, l, r), r)
    h = [cc[m + np - 2] for m in range(np - 1)] + [0]
    assert h == h_terms(f, n, l, tau, r)
    return dft(h, pow(w_2n, 2 * l, r), r)


def a_hat_split(f: Sequence[int], n: int, l: int, c: int, w_2n: int, r: int):
    """(even, odd) entries of DFT_2n'(a_c) from two transforms of size n'"""
    f = padded(f, n)
    np = n // l
    a = [f[c + l * (u + 1)] for u in range(np - 1)] + [0]
    w_2np = pow(w_2n, l, r)
    twisted = [x * pow(w_2np, u, r) % r for u, x in enumerate(a)]
    w_np = w_2np * w_2np % r
    return dft(a, w_np, r), dft(twisted, w_np, r)


def composition(f: Sequence[int], n: int, l: int, w: int, tau: int, r: int, h1: Sequence[int] = None) -> List[int]:
    h1 = direct_single(f, n, w, tau, r) if h1 is None else h1
    np = n // l
    out = []
    for i in range(np):
        inv = pow(l * pow(w, i * l, r) % r, -1, r)
        out.append(sum(pow(w, i + np * j, r) * inv % r * h1[i + np * j] for j in range(l)) % r)
    return out


def composition_weights(n: int, l: int, w: int, r: int) -> List[int]:
    """weight[i l + j] of H^(1)_(i + n' j) in H_i"""
    np = n // l
    return [pow(w, i + np * j, r) * pow(l * pow(w, i * l, r) % r, -1, r) % r for i in range(np) for j in range(l)]


def interpolate(values: Sequence[int], n: int, l: int, i: int, w: int, r: int) -> List[int]:
    """the l coefficients of I_i from its values at x_(i,j), j = 0 .. l-1"""
    co = idft(list(values), pow(w, n // l, r), r)
    return [x * pow(w, -i * c, r) % r for c, x in enumerate(co)]


def accepts(commitment: int, values: Sequence[int], h: int, n: int, l: int, i: int, w: int, tau: int, r: int) -> bool:
    a = pow(w, i * l, r)
    it = horner(interpolate(values, n, l, i, w, r), tau, r)
    return (commitment - it + a * h - pow(tau, l, r) * h) % r == 0

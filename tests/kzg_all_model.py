"""Big-integer model of the openings of one polynomial at every point of its domain (include/apk.h apk_kzg_open_all;
csrc/kernels_kzg_all.h), in the exponent with a known tau: a G1 point [x]G1 is the scalar x.

  direct()       H_i = (f(tau) - f(w^i)) / (tau - w^i): what apk_kzg_open(f, w^i) commits
  arrangement()  the same through the cyclic convolution of size 2n the kernels run: a = (f_1 .. f_(n-1), 0 ..),
                 t = (tau^(n-2) .. tau^0, 0 ..), c = IDFT_2n(DFT_2n(a) DFT_2n(t)), h_k = c[k + n - 2], H = DFT_n(h)
  a_hat_split()  DFT_2n(a) from two size-n transforms: even entries NTT_n(a), odd entries NTT_n(a_m w_2n^m)
"""
from __future__ import annotations

from typing import List, Sequence


def dft(vec: Sequence[int], w: int, r: int) -> List[int]:
    """out[i] = sum_m vec[m] w^(i m), the plain sum (the sizes here are small)"""
    n = len(vec)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % r
    return [sum(v * pw[i * m % n] for m, v in enumerate(vec) if v) % r for i in range(n)]


def idft(vec: Sequence[int], w: int, r: int) -> List[int]:
    n_inv = pow(len(vec), -1, r)
    return [x * n_inv % r for x in dft(vec, pow(w, -1, r), r)]


def horner(f: Sequence[int], z: int, r: int) -> int:
    acc = 0
    for c in reversed(f):
        acc = (acc * z + c) % r
    return acc


def padded(f: Sequence[int], n: int) -> List[int]:
    assert 1 <= len(f) <= n
    return list(f) + [0] * (n - len(f))


def direct(f: Sequence[int], n: int, w: int, tau: int, r: int) -> List[int]:
    ft = horner(f, tau, r)
    out, z = [], 1
    for _ in range(n):
        assert (tau - z) % r
        out.append((ft - horner(f, z, r)) * pow((tau - z) % r, -1, r) % r)
        z = z * w % r
    return out


def h_terms(f: Sequence[int], n: int, tau: int, r: int) -> List[int]:
    """h_k = sum_{j <= n-2-k} f_(k+1+j) tau^j for k <= n - 2, and h_(n-1) = 0"""
    f = padded(f, n)
    return [horner(f[k + 1:], tau, r) for k in range(n - 1)] + [0]


def sequences(f: Sequence[int], n: int, tau: int, r: int):
    """(a, t): the two sequences of length 2n"""
    f = padded(f, n)
    a = f[1:] + [0] * (n + 1)
    t = [pow(tau, n - 2 - i, r) for i in range(n - 1)] + [0] * (n + 1)
    return a, t


def arrangement(f: Sequence[int], n: int, w_2n: int, tau: int, r: int) -> List[int]:
    a, t = sequences(f, n, tau, r)
    a_hat, t_hat = dft(a, w_2n, r), dft(t, w_2n, r)
    c = idft([x * y % r for x, y in zip(a_hat, t_hat)], w_2n, r)
    h = [c[k + n - 2] for k in range(n - 1)] + [0]
    assert h == h_terms(f, n, tau, r)
    return dft(h, w_2n * w_2n % r, r)


def a_hat_split(f: Sequence[int], n: int, w_2n: int, r: int):
    """(even, odd) entries of DFT_2n(a) from two transforms of size n"""
    a = padded(f, n)[1:] + [0]
    w = w_2n * w_2n % r
    twisted = [x * pow(w_2n, m, r) % r for m, x in enumerate(a)]
    return dft(a, w, r), dft(twisted, w, r)


def meeting_points(n: int, tau: int, r: int, tail: Sequence[int], opposite: bool) -> List[int]:
    """f with f_2 .. f_(n/2) = 0, f_(n/2+1) .. = tail, and f_1 chosen so that h_0 = h_(n/2) (or h_0 = -h_(n/2)): the two points the
    first butterfly of the size-n transform adds are equal (opposite)."""
    assert len(tail) == n - 1 - n // 2
    h_half = horner(tail, tau, r)
    tn = pow(tau, n // 2, r)
    f1 = (-(1 + tn) if opposite else (1 - tn)) * h_half % r
    return [5, f1] + [0] * (n // 2 - 1) + list(tail)

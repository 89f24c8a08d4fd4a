"""KZG in evaluation form in big integers, over a synthetic SRS whose tau is known (the model of tests/kzg_model.py): what
apk_kzg_open_lagrange / apk_kzg_batch_open_lagrange must produce.

The polynomial f of degree < n is given by its values f_i = f(omega^i).  Both f(tau) and f(z) come from the barycentric formula
    f(x) = (x^n - 1)/n * sum_i f_i omega^i / (x - omega^i)          (x off the domain;  f(omega^m) = f_m)
and the opening is one scalar multiple, H = [(f(tau) - f(z)) / (tau - z)] G1: no quotient, no interpolation, no MSM - nothing
shared with the kernels under test.  tau is taken off the domain, and the point must differ from tau."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import kzg_model as km


def batch_inverse(xs: Sequence[int], r: int) -> List[int]:
    """1/x for every x (none zero), with one modular inversion"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % r
    inv = pow(acc, -1, r)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % r
        inv = inv * xs[i] % r
    return out


class Domain:
    """<omega> of size n in F_r, natural order."""

    def __init__(self, omega: int, n: int, r: int):
        assert pow(omega, n, r) == 1 and pow(omega, n // 2, r) == r - 1
        self.n, self.r, self.omega = n, r, omega
        self.pts = [1] * n
        for i in range(1, n):
            self.pts[i] = self.pts[i - 1] * omega % r
        self.index = None

    def find(self, x: int) -> Optional[int]:
        """m with omega^m == x, or None"""
        if pow(x, self.n, self.r) != 1:
            return None
        if self.index is None:
            self.index = {p: i for i, p in enumerate(self.pts)}
        return self.index[x % self.r]

    def weights(self, x: int) -> List[int]:
        """L_i(x) for every i"""
        n, r = self.n, self.r
        m = self.find(x)
        if m is not None:
            return [1 if i == m else 0 for i in range(n)]
        scale = (pow(x, n, r) - 1) * pow(n, -1, r) % r
        inv = batch_inverse([(x - p) % r for p in self.pts], r)
        return [scale * p % r * q % r for p, q in zip(self.pts, inv)]

    def evaluate(self, values: Sequence[int], x: int) -> int:
        """f(x) by the barycentric formula"""
        m = self.find(x)
        if m is not None:
            return values[m] % self.r
        return dot(values, self.weights(x), self.r)

    def interpolate(self, values: Sequence[int]) -> List[int]:
        """the n coefficients of f (an O(n^2) inverse DFT: for the small sizes of the cross-checks)"""
        n, r = self.n, self.r
        ninv = pow(n, -1, r)
        return [sum(v * self.pts[(-i * j) % n] for i, v in enumerate(values)) % r * ninv % r for j in range(n)]


def dot(a: Sequence[int], b: Sequence[int], r: int) -> int:
    return sum(x * y for x, y in zip(a, b)) % r


class Srs:
    """The known-tau side: L_i(tau) once per domain, so f(tau) is one dot product per vector."""

    def __init__(self, dom: Domain, tau: int):
        assert dom.find(tau) is None, "tau on the domain: draw another"
        self.dom, self.tau = dom, tau
        self.at_tau_w = dom.weights(tau)

    def at_tau(self, values: Sequence[int]) -> int:
        return dot(values, self.at_tau_w, self.dom.r)


def commit(ov, srs: Srs, values: Sequence[int]):
    """[f(tau)] G1: what the MSM over the Lagrange SRS gives"""
    return ov.mul(ov.g1, srs.at_tau(values))


def open_at(ov, srs: Srs, values: Sequence[int], z: int) -> Tuple[object, int]:
    """(H, f(z))"""
    r = srs.dom.r
    assert (srs.tau - z) % r != 0, "draw another point"
    v = srs.dom.evaluate(values, z)
    return ov.mul(ov.g1, (srs.at_tau(values) - v) * pow((srs.tau - z) % r, -1, r) % r), v


def batch_open_at(ov, srs: Srs, vectors: Sequence[Sequence[int]], z: int, extra: bytes = b"", digests: Optional[Sequence] = None):
    """(digests, values, gamma, H) of kzg.BatchOpenSinglePoint on the interpolants"""
    r = srs.dom.r
    assert (srs.tau - z) % r != 0, "draw another point"
    digests = list(digests) if digests is not None else [commit(ov, srs, f) for f in vectors]
    w = srs.dom.weights(z)
    values = [dot(f, w, r) for f in vectors]
    gamma = km.fold_challenge(ov, z, digests, values, extra)
    k, g = 0, 1
    for f, v in zip(vectors, values):
        k = (k + g * (srs.at_tau(f) - v)) % r
        g = g * gamma % r
    return digests, values, gamma, ov.mul(ov.g1, k * pow((srs.tau - z) % r, -1, r) % r)


def vector(kind: str, dom: Domain, rng, m: int = 0) -> List[int]:
    """The value vectors the tests open: random, all zero, all equal, one-hot at m, every value r - 1, the values of X^(n-1)."""
    n, r = dom.n, dom.r
    if kind == "random":
        return [rng.fr(r) for _ in range(n)]
    if kind == "zero":
        return [0] * n
    if kind == "constant":
        c = rng.fr(r) or 1
        return [c] * n
    if kind == "one-hot":
        return [(rng.fr(r) or 1) if i == m else 0 for i in range(n)]
    if kind == "max":
        return [r - 1] * n
    if kind == "top":       # X^(n-1) at omega^i = omega^(-i)
        return [dom.pts[(-i) % n] for i in range(n)]
    raise ValueError(kind)

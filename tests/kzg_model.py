"""The KZG primitives in big integers, over a synthetic SRS whose tau is known: what apk_kzg_open / apk_kzg_batch_open must
produce and what apk_kzg_verify / apk_kzg_batch_verify must accept.

With tau known a commitment is ONE scalar multiple, [f(tau)] G1, and so is an opening: H = [(f(tau) - f(z)) / (tau - z)] G1 -
no polynomial division, no MSM, nothing shared with the kernels under test.  The point must differ from tau (the caller draws
another one)."""
from __future__ import annotations

import ctypes as C
import hashlib
from typing import List, Optional, Sequence, Tuple

from algoplonk_amd import _lib
from algoplonk_amd._lib import lib


def horner(coeffs: Sequence[int], z: int, r: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % r
    return acc


def commit(ov, coeffs: Sequence[int], tau: int):
    return ov.mul(ov.g1, horner(coeffs, tau, ov.r))


def open_at(ov, coeffs: Sequence[int], z: int, tau: int) -> Tuple[object, int]:
    """(H, f(z))"""
    r = ov.r
    assert (tau - z) % r != 0, "draw another point"
    v = horner(coeffs, z, r)
    k = (horner(coeffs, tau, r) - v) * pow((tau - z) % r, -1, r) % r
    return ov.mul(ov.g1, k), v


def fold_challenge(ov, z: int, digests: Sequence, values: Sequence[int], extra: bytes = b"") -> int:
    """gnark-crypto's deriveGamma: sha256("gamma" || z || digests || values || extra) mod r"""
    h = hashlib.sha256(b"gamma")
    h.update(z.to_bytes(32, "big"))
    for d in digests:
        h.update(ov.raw_bytes(d))
    for v in values:
        h.update(v.to_bytes(32, "big"))
    h.update(extra)
    return int.from_bytes(h.digest(), "big") % ov.r


def batch_open_at(ov, polys: Sequence[Sequence[int]], z: int, tau: int, extra: bytes = b"",
                  digests: Optional[Sequence] = None):
    """(digests, values, gamma, H) of kzg.BatchOpenSinglePoint"""
    r = ov.r
    digests = list(digests) if digests is not None else [commit(ov, f, tau) for f in polys]
    values = [horner(f, z, r) for f in polys]
    gamma = fold_challenge(ov, z, digests, values, extra)
    assert (tau - z) % r != 0, "draw another point"
    k, g = 0, 1
    for f, v in zip(polys, values):
        k = (k + g * (horner(f, tau, r) - v)) % r
        g = g * gamma % r
    return digests, values, gamma, ov.mul(ov.g1, k * pow((tau - z) % r, -1, r) % r)


# ---- the C-ABI's side -----------------------------------------------------------------------------------------------------------
def kzg_vk(cv, g2: bytes) -> _lib.KzgVk:
    """apk_kzg_vk from the curve's generator and ([1]G2, [tau]G2) in gnark's in-memory form (setup.g2_from_tau)."""
    vk = _lib.KzgVk()
    vk.curve = cv.abi
    g1 = cv.g1_to_bytes(cv.g1)
    C.memmove(vk.g1, g1, len(g1))
    w = 4 * cv.fp_bytes
    for j in range(2):
        C.memmove(vk.g2[j], g2[j * w:(j + 1) * w], w)
    return vk


def verify(cv, vk, digest, z: int, value: int, H) -> int:
    return lib.apk_kzg_verify(C.byref(vk), cv.g1_to_bytes(digest), cv.fr_vector([z]), cv.fr_vector([value]), cv.g1_to_bytes(H))


def batch_verify(cv, vk, digests: Sequence, values: Sequence[int], z: int, extra: bytes, H) -> int:
    return lib.apk_kzg_batch_verify(C.byref(vk), len(digests), cv.g1_vector(digests), cv.fr_vector(values), cv.fr_vector([z]),
                                    extra if extra else None, len(extra), cv.g1_to_bytes(H))


def polynomial(kind: str, length: int, r: int, rng) -> List[int]:
    """The shapes the tests open: random, all-zero, constant, every coefficient r - 1, a single non-zero top coefficient."""
    if kind == "random":
        return [rng.fr(r) for _ in range(length)]
    if kind == "zero":
        return [0] * length
    if kind == "constant":
        return [rng.fr(r)] + [0] * (length - 1)
    if kind == "max":
        return [r - 1] * length
    if kind == "top":
        return [0] * (length - 1) + [rng.fr(r) or 1]
    raise ValueError(kind)

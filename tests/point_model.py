"""The G1 point kernels that run outside the MSM, in big integers: which compressed encodings apk_g1_decompress must accept and
what they decode to, where the sign compare of that decoding has its boundary, and what apk_g1_to_lagrange must produce for
inputs that are known multiples of the generator.

Everything here is arithmetic on Python ints over oracle/curves.py (`mul`, `add`, `neg`, `is_on_curve`, `sqrt_mod`); nothing is
shared with ec.h or the kernels under test (tests/test_gpu_point_kernels.py), and tests/test_point_model.py holds this file to
`oracle.compress`, to the rejections tests/test_gpu_setup.py already pins and to the reference's known answers."""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

from oracle.curves import sqrt_mod

REJECT = "reject"          # accepts(): not a valid compressed G1 encoding (None is a valid one: the point at infinity)


def flag_bits(ov) -> int:
    """Width of the flag field at the top of byte 0: 2 bits on BN254, 3 on BLS12-381."""
    return 3 if ov.name == "bls12-381" else 2


def payload_mask(ov) -> int:
    """The largest x the flag mask leaves."""
    return (1 << (8 * ov.fp_bytes - flag_bits(ov))) - 1


def flag_patterns(ov) -> List[int]:
    return list(range(1 << flag_bits(ov)))


def encode(ov, flags: int, x: int) -> bytes:
    """`flags` (a value of the 2- or 3-bit field) over the payload x, whatever either means."""
    assert 0 <= x <= payload_mask(ov) and 0 <= flags < (1 << flag_bits(ov))
    return (flags << (8 * ov.fp_bytes - flag_bits(ov)) | x).to_bytes(ov.fp_bytes, "big")


def _meaning(ov, flags: int) -> Optional[str]:
    """gnark-crypto's mask constants.  BN254: 10 smallest y, 11 largest y, 01 infinity, 00 uncompressed.  BLS12-381: 100 / 101 /
    110 for the same three, 000 and 010 uncompressed, 001 / 011 / 111 nothing at all.  An uncompressed pattern announces an
    encoding of twice the length, which a compressed slot cannot hold: SetBytes refuses it as a short buffer."""
    if ov.name == "bls12-381":
        return {0b100: "smallest", 0b101: "largest", 0b110: "infinity"}.get(flags)
    return {0b10: "smallest", 0b11: "largest", 0b01: "infinity"}.get(flags)


def in_subgroup(ov, P) -> bool:
    """[r]P = infinity, as (r-1)P + P: the oracle's mul reduces its scalar mod r."""
    return P is None or ov.add(ov.mul(P, ov.r - 1), P) is None


def accepts(ov, encoding: bytes):
    """gnark's G1Affine.SetBytes on one compressed encoding: the decoded point, None for the point at infinity, REJECT otherwise.

      * the flag pattern must be one of the curve's three compressed ones (_meaning);
      * the infinity flag must carry an all-zero payload;
      * x < p (SetBytesCanonical);
      * x^3 + b must be a square in Fp;
      * of the two roots the flag picks the one with y > (p-1)/2 ("largest") or the other;
      * on BLS12-381, whose G1 has a cofactor, the point must be in the order-r subgroup.  BN254's curve has prime order."""
    assert len(encoding) == ov.fp_bytes
    v = int.from_bytes(encoding, "big")
    flags, x = v >> (8 * ov.fp_bytes - flag_bits(ov)), v & payload_mask(ov)
    what = _meaning(ov, flags)
    if what is None:
        return REJECT
    if what == "infinity":
        return None if x == 0 else REJECT
    if x >= ov.p:
        return REJECT
    y = sqrt_mod((x * x * x + ov.b) % ov.p, ov.p)
    if y is None:
        return REJECT
    if (y > (ov.p - 1) // 2) != (what == "largest"):
        y = (ov.p - y) % ov.p
    P = (x, y)
    if ov.name == "bls12-381" and not in_subgroup(ov, P):
        return REJECT
    return P


def wrong_sign(ov, P) -> bytes:
    """The compressed encoding of P with its sign flag flipped: a valid encoding of -P."""
    b = bytearray(ov.compress(P))
    b[0] ^= 0x20 if ov.name == "bls12-381" else 0x40
    return bytes(b)


# ---- the sign compare's boundary ------------------------------------------------------------------------------------------------
def cube_roots(a: int, p: int) -> List[int]:
    """Every x with x^3 = a in Fp, p = 1 mod 3 (sorted; empty when a is no cube).  p - 1 = 3^s t: a^(1/3 mod t) is right up to
    an element of the 3-Sylow subgroup, which is small (s = 2 for both base fields) and searched."""
    a %= p
    if a == 0:
        return [0]
    assert p % 3 == 1
    if pow(a, (p - 1) // 3, p) != 1:
        return []
    s, t = 0, p - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    assert 3 ** s < 1 << 16
    g = 2
    while pow(g, (p - 1) // 3, p) == 1:
        g += 1
    c = pow(g, t, p)                                  # generates the 3-Sylow subgroup
    x0 = pow(a, pow(3, -1, t), p)
    roots = sorted({x0 * pow(c, j, p) % p for j in range(3 ** s) if pow(x0 * pow(c, j, p), 3, p) == a})
    assert len(roots) == 3
    return roots


def points_with_y(ov, y: int) -> List[Tuple[int, int]]:
    """The (up to three) curve points with this y."""
    return [(x, y % ov.p) for x in cube_roots((y * y - ov.b) % ov.p, ov.p)]


@functools.lru_cache(maxsize=None)
def boundary_point(ov):
    """The point with y = (p-1)/2 - the largest y that is still "smallest" - with its negation (x, (p+1)/2), or None.

    It exists when ((p-1)/2)^2 - b is a cube in Fp, about one residue in three.  It is a cube for NEITHER curve:
      * BN254:     ((p-1)/2)^2 - 3 is not a cube mod p: no such point;
      * BLS12-381: ((p-1)/2)^2 - 4 is not a cube mod p: no such point
    (tests/test_point_model.py pins both).  near_boundary() gives the points that do exist closest to the boundary."""
    h = (ov.p - 1) // 2
    pts = points_with_y(ov, h)
    if not pts:
        return None
    P = pts[0]
    return P, ov.neg(P)


@functools.lru_cache(maxsize=None)
def near_boundary(ov):
    """(P, Q): the curve points whose y is the closest to the boundary from below (y <= (p-1)/2, "smallest") and from above
    (y >= (p+1)/2, "largest").  Their y agree with (p-1)/2 in every 32-bit word but the lowest, so a word-by-word compare walks
    all the way down.  On BLS12-381 such points are (almost surely) outside G1 and decode to REJECT under either flag."""
    h = (ov.p - 1) // 2
    below = next(pts[0] for d in range(1 << 12) for pts in [points_with_y(ov, h - d)] if pts)
    above = next(pts[0] for d in range(1 << 12) for pts in [points_with_y(ov, h + 1 + d)] if pts)
    return below, above


# ---- ToLagrangeG1 ---------------------------------------------------------------------------------------------------------------
def lagrange_of(scalars: Sequence[int], n: int, r: int, omega: int) -> List[int]:
    """kzg.ToLagrangeG1 in the exponent.  For inputs a_j G, j < n, the outputs are c_i G with
        c_i = (1/n) * sum_j omega^(-ij) a_j      (an inverse DFT of size n over Fr)
    since sum_i c_i omega^(ik) = a_k: committing evaluations under c equals committing coefficients under a.  With a_j = tau^j
    this is L_i(tau); nothing here needs the a_j to be powers of anything.  Plain n x n modular sum; returns the c_i."""
    assert len(scalars) == n and pow(omega, n, r) == 1 and (n == 1 or pow(omega, n // 2, r) == r - 1)
    winv = pow(omega, -1, r)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * winv % r
    n_inv = pow(n, -1, r)
    nz = [(j, a % r) for j, a in enumerate(scalars) if a % r]
    return [sum(a * pw[i * j % n] for j, a in nz) % r * n_inv % r for i in range(n)]


def lagrange_points(ov, scalars: Sequence[int], n: int) -> list:
    """The n expected output points: n group multiplications."""
    return [ov.mul(ov.g1, c) for c in lagrange_of(scalars, n, ov.r, ov.omega(n))]

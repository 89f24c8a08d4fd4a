"""gnark-crypto's `kzg` package over libapk (include/apk.h apk_kzg_*): Commit, Open, BatchOpenSinglePoint and OpenMultiPoints (one
Open per (polynomial, point) pair, batched) on the GPU, Verify and BatchVerifySinglePoint on the host, BatchVerifyMultiPoints on
the host or with its fold on a GPU; OpenAllDomain and OpenCosets open one polynomial at every point, or on every coset, of its
domain in one call (VerifyCoset checks one coset's proof on the host), OpenCosetsMulti up to 64 polynomials on every coset.

The `key` of the GPU calls is anything that owns a libapk context over a canonical SRS: a `plonk.ProvingKey` (polynomials of up to
n + 3 coefficients) or an `MsmContext` made here (as many coefficients as it has bases).  Polynomials are coefficient lists,
lowest degree first.  There is no CPU fallback for Commit / Open / BatchOpenSinglePoint.

The `...Lagrange` calls take a polynomial of degree < n by its n values on the domain of a `plonk.ProvingKey` (index i belongs to
omega^i) and work over the Lagrange SRS: the commitment, H and the value are those of the interpolant's coefficients, so `Verify`
and `BatchVerifySinglePoint` take them as they are; `OpenMultiPointsLagrange` is `OpenMultiPoints` in this form, for
`BatchVerifyMultiPoints`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

from . import _lib, ecc
from ._lib import check, lib


class VerificationError(RuntimeError):
    pass


@dataclass
class OpeningProof:
    """kzg.OpeningProof"""
    H: ecc.Point
    ClaimedValue: int


@dataclass
class BatchOpeningProof:
    """kzg.BatchOpeningProof"""
    H: ecc.Point
    ClaimedValues: List[int]


@dataclass
class VerifyingKey:
    """kzg.VerifyingKey: G1 = SRS G1[0], G2 = ([1]G2, [tau]G2) in gnark's in-memory form (setup.SRS.g2)."""
    curve: ecc.ID
    G1: ecc.Point
    G2: bytes

    def raw(self) -> "_lib.KzgVk":
        cv = self.curve
        w = 4 * cv.fp_bytes
        if self.G1 is None or len(self.G2) != 2 * w:
            raise ValueError("kzg verifying key: need G1 and two G2 points")
        v = _lib.KzgVk()
        v.curve = cv.abi
        g1 = cv.g1_to_bytes(self.G1)
        C.memmove(v.g1, g1, len(g1))
        for j in range(2):
            C.memmove(v.g2[j], self.G2[j * w:(j + 1) * w], w)
        return v


class MsmContext:
    """An MSM-only libapk context over `bases` (G1 affine bytes, gnark in-memory form): kzg.ProvingKey without a circuit."""

    def __init__(self, curve: ecc.ID, bases: bytes, device: int = 0, msm_window: int = 0):
        self.curve = curve
        self.count = len(bases) // (2 * curve.fp_bytes)
        self._ctx = C.c_void_p()
        check(lib.apk_msm_ctx_create(curve.abi, device, bases, self.count, msm_window, C.byref(self._ctx)))

    @property
    def ctx(self) -> C.c_void_p:
        if not self._ctx:
            raise RuntimeError("kzg context was closed")
        return self._ctx

    def close(self) -> None:
        if self._ctx:
            lib.apk_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p(None)

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass


def Commit(p: Sequence[int], key) -> ecc.Point:
    """kzg.Commit(p, pk)"""
    cv = key.curve
    if len(p) == 0:
        raise ValueError("invalid polynomial size (no coefficients)")
    out = C.create_string_buffer(2 * cv.fp_bytes)
    check(lib.apk_msm_g1(key.ctx, 0, cv.fr_vector(p), len(p), out))
    return cv.g1_from_bytes(out.raw)


def Open(p: Sequence[int], point: int, key) -> OpeningProof:
    """kzg.Open(p, point, pk)"""
    cv = key.curve
    if len(p) == 0:
        raise ValueError("invalid polynomial size (no coefficients)")
    h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    check(lib.apk_kzg_open(key.ctx, cv.fr_vector(p), len(p), cv.fr_vector([point]), h, v))
    return OpeningProof(cv.g1_from_bytes(h.raw), cv.fr_from_mont_bytes(v.raw))


def BatchOpenSinglePoint(polynomials: Sequence[Sequence[int]], digests: Optional[Sequence[ecc.Point]], point: int, key,
                         dataTranscript: bytes = b"") -> BatchOpeningProof:
    """kzg.BatchOpenSinglePoint(polynomials, digests, point, hf, pk, dataTranscript...) with sha256 as the hash; digests = None
    commits the polynomials first."""
    cv = key.curve
    k = len(polynomials)
    if k == 0 or any(len(p) == 0 for p in polynomials):
        raise ValueError("invalid polynomial size (no polynomials, or one without coefficients)")
    if digests is not None and len(digests) != k:
        raise ValueError("invalid number of digests, got %d, expected %d" % (len(digests), k))
    bufs = [C.create_string_buffer(cv.fr_vector(p), 32 * len(p)) for p in polynomials]
    ptrs = (C.c_void_p * k)(*[C.addressof(b) for b in bufs])
    lens = (C.c_uint64 * k)(*[len(p) for p in polynomials])
    h, vals = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32 * k)
    check(lib.apk_kzg_batch_open(key.ctx, k, ptrs, lens, cv.g1_vector(digests) if digests is not None else None, cv.fr_vector([point]),
                                 dataTranscript or None, len(dataTranscript), h, vals, None))
    return BatchOpeningProof(cv.g1_from_bytes(h.raw), cv.fr_vector_decode(vals.raw))


def OpenMultiPoints(polynomials: Sequence[Sequence[int]], points: Sequence[int], key) -> List[OpeningProof]:
    """One kzg.Open per (polynomials[i], points[i]) pair in one call: the quotients of up to four pairs are committed as one MSM
    batch.  A polynomial that occurs several times (the same list object) is uploaded once."""
    cv = key.curve
    k = len(polynomials)
    if k == 0 or any(len(p) == 0 for p in polynomials):
        raise ValueError("invalid polynomial size (no polynomials, or one without coefficients)")
    if len(points) != k:
        raise ValueError("invalid number of points, got %d, expected %d" % (len(points), k))
    bufs = {}
    for p in polynomials:
        if id(p) not in bufs:
            bufs[id(p)] = C.create_string_buffer(cv.fr_vector(p), 32 * len(p))
    ptrs = (C.c_void_p * k)(*[C.addressof(bufs[id(p)]) for p in polynomials])
    lens = (C.c_uint64 * k)(*[len(p) for p in polynomials])
    w = 2 * cv.fp_bytes
    h, vals = C.create_string_buffer(w * k), C.create_string_buffer(32 * k)
    check(lib.apk_kzg_open_multi(key.ctx, k, ptrs, lens, cv.fr_vector(list(points)), h, vals))
    values = cv.fr_vector_decode(vals.raw)
    return [OpeningProof(cv.g1_from_bytes(h.raw[i * w:(i + 1) * w]), values[i]) for i in range(k)]


def _domain_size(key) -> int:
    n = getattr(key, "n", None)
    if n is None:
        raise ValueError("openings in evaluation form need a key with a domain (a plonk.ProvingKey)")
    return int(n)


def CommitLagrange(values: Sequence[int], key) -> ecc.Point:
    """kzg.Commit(values, pk) over the Lagrange SRS: the commitment of the polynomial with these n values on the domain"""
    cv = key.curve
    if len(values) != _domain_size(key):
        raise ValueError("invalid number of values, got %d, the domain has %d" % (len(values), _domain_size(key)))
    out = C.create_string_buffer(2 * cv.fp_bytes)
    check(lib.apk_msm_g1(key.ctx, 1, cv.fr_vector(values), len(values), out))
    return cv.g1_from_bytes(out.raw)


def OpenLagrange(values: Sequence[int], point: int, key) -> OpeningProof:
    """kzg.Open of the polynomial with these n values on the domain, without leaving the evaluation form"""
    cv = key.curve
    if len(values) != _domain_size(key):
        raise ValueError("invalid number of values, got %d, the domain has %d" % (len(values), _domain_size(key)))
    h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    check(lib.apk_kzg_open_lagrange(key.ctx, cv.fr_vector(values), len(values), cv.fr_vector([point]), h, v))
    return OpeningProof(cv.g1_from_bytes(h.raw), cv.fr_from_mont_bytes(v.raw))


def BatchOpenSinglePointLagrange(vectors: Sequence[Sequence[int]], digests: Optional[Sequence[ecc.Point]], point: int, key,
                                 dataTranscript: bytes = b"") -> BatchOpeningProof:
    """kzg.BatchOpenSinglePoint of the polynomials with these values on the domain; digests = None commits the vectors first
    (CommitLagrange)."""
    cv = key.curve
    k, n = len(vectors), _domain_size(key)
    if k == 0 or any(len(p) != n for p in vectors):
        raise ValueError("invalid vectors (none, or one that has not the domain's %d values)" % n)
    if digests is not None and len(digests) != k:
        raise ValueError("invalid number of digests, got %d, expected %d" % (len(digests), k))
    bufs = [C.create_string_buffer(cv.fr_vector(p), 32 * n) for p in vectors]
    ptrs = (C.c_void_p * k)(*[C.addressof(b) for b in bufs])
    h, vals = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32 * k)
    check(lib.apk_kzg_batch_open_lagrange(key.ctx, k, ptrs, cv.g1_vector(digests) if digests is not None else None, cv.fr_vector([point]),
                                          dataTranscript or None, len(dataTranscript), h, vals, None))
    return BatchOpeningProof(cv.g1_from_bytes(h.raw), cv.fr_vector_decode(vals.raw))


def OpenMultiPointsLagrange(vectors: Sequence[Sequence[int]], points: Sequence[int], key) -> List[OpeningProof]:
    """One OpenLagrange per (vectors[i], points[i]) pair in one call: the quotients of up to four pairs are committed as one MSM
    batch over the Lagrange SRS.  A vector that occurs several times (the same list object) is uploaded once."""
    cv = key.curve
    k, n = len(vectors), _domain_size(key)
    if k == 0 or k > 32 or any(len(p) != n for p in vectors):
        raise ValueError("invalid vectors (none, more than 32, or one that has not the domain's %d values)" % n)
    if len(points) != k:
        raise ValueError("invalid number of points, got %d, expected %d" % (len(points), k))
    bufs = {}
    for p in vectors:
        if id(p) not in bufs:
            bufs[id(p)] = C.create_string_buffer(cv.fr_vector(p), 32 * n)
    ptrs = (C.c_void_p * k)(*[C.addressof(bufs[id(p)]) for p in vectors])
    w = 2 * cv.fp_bytes
    h, vals = C.create_string_buffer(w * k), C.create_string_buffer(32 * k)
    check(lib.apk_kzg_open_multi_lagrange(key.ctx, k, ptrs, cv.fr_vector(list(points)), h, vals))
    values = cv.fr_vector_decode(vals.raw)
    return [OpeningProof(cv.g1_from_bytes(h.raw[i * w:(i + 1) * w]), values[i]) for i in range(k)]


def PrepareAllDomain(key, srs) -> None:
    """What OpenAllDomain needs of the canonical SRS the key was made over (`srs`: a setup.SRS, or its G1 bytes): the context keeps
    the transform of the reversed SRS.  Once per key; calling it again changes nothing."""
    cv = key.curve
    n = _domain_size(key)
    g1 = srs if isinstance(srs, (bytes, bytearray)) else srs.g1
    count = len(g1) // (2 * cv.fp_bytes)
    if count < n - 1:
        raise ValueError("invalid SRS, got %d points, the domain needs %d" % (count, n - 1))
    check(lib.apk_kzg_all_prepare(key.ctx, bytes(g1), count))


def OpenAllDomain(p: Sequence[int], key) -> List[OpeningProof]:
    """kzg.Open(p, omega^i, pk) for every i < n in one call (Feist - Khovratovich: O(n log n) group operations, not n MSMs);
    entry i belongs to omega^i.  p has at most n coefficients; PrepareAllDomain(key, srs) comes first."""
    cv = key.curve
    n = _domain_size(key)
    if len(p) == 0 or len(p) > n:
        raise ValueError("invalid polynomial size, got %d coefficients, the domain takes 1..%d" % (len(p), n))
    w = 2 * cv.fp_bytes
    h, vals = C.create_string_buffer(w * n), C.create_string_buffer(32 * n)
    check(lib.apk_kzg_open_all(key.ctx, cv.fr_vector(p), len(p), h, vals))
    values = cv.fr_vector_decode(vals.raw)
    return [OpeningProof(cv.g1_from_bytes(h.raw[i * w:(i + 1) * w]), values[i]) for i in range(n)]


@dataclass
class CosetOpeningProof:
    """One proof for the l points omega^(i + (n / l) j), j < l, of coset i: H = [(f - I_i) / (X^l - omega^(i l))] and the l values in
    the order j = 0 .. l-1"""
    H: ecc.Point
    ClaimedValues: List[int]


def _coset_size(n: int, coset_size: int) -> int:
    l = int(coset_size)
    if l < 2 or l & (l - 1) or l > n // 2:
        raise ValueError("invalid coset size %d, the domain of %d points takes a power of two in 2..%d" % (l, n, n // 2))
    return l


def PrepareCosets(key, srs, coset_size: int) -> None:
    """What OpenCosets needs of the canonical SRS the key was made over (`srs`: a setup.SRS, or its G1 bytes): the context keeps a
    table of 8n points for ONE coset size.  Once per key; the same size again changes nothing, another size is an error."""
    cv = key.curve
    n = _domain_size(key)
    l = _coset_size(n, coset_size)
    g1 = srs if isinstance(srs, (bytes, bytearray)) else srs.g1
    count = len(g1) // (2 * cv.fp_bytes)
    if count < n - l:
        raise ValueError("invalid SRS, got %d points, cosets of %d points need %d" % (count, l, n - l))
    check(lib.apk_kzg_cosets_prepare(key.ctx, bytes(g1), count, l))
    key.kzg_coset_size = l


def OpenCosets(p: Sequence[int], key) -> List[CosetOpeningProof]:
    """One proof per coset of the size PrepareCosets(key, srs, coset_size) chose, n / coset_size of them in one call (Feist -
    Khovratovich); entry i belongs to the points omega^(i + (n / l) j).  p has at most n coefficients."""
    cv = key.curve
    n = _domain_size(key)
    if len(p) == 0 or len(p) > n:
        raise ValueError("invalid polynomial size, got %d coefficients, the domain takes 1..%d" % (len(p), n))
    l = getattr(key, "kzg_coset_size", None)
    if l is None:
        raise ValueError("PrepareCosets(key, srs, coset_size) comes first")
    w, np = 2 * cv.fp_bytes, n // l
    h, vals = C.create_string_buffer(w * np), C.create_string_buffer(32 * n)
    check(lib.apk_kzg_open_cosets(key.ctx, cv.fr_vector(p), len(p), h, vals))
    values = cv.fr_vector_decode(vals.raw)
    return [CosetOpeningProof(cv.g1_from_bytes(h.raw[i * w:(i + 1) * w]), values[i * l:(i + 1) * l]) for i in range(np)]


COSETS_MULTI_MAX = 64      # include/apk.h APK_KZG_COSETS_MULTI_MAX


def OpenCosetsMulti(polynomials: Sequence[Sequence[int]], key) -> List[List[CosetOpeningProof]]:
    """OpenCosets for up to 64 polynomials in one call (the blobs of a block): result[b] is what OpenCosets(polynomials[b], key)
    returns, the same bytes, while the polynomials share the launches of the transforms in the exponent.  The lengths may differ; a
    list object that occurs several times is encoded once and handed over as one pointer, which the call uploads once per group of
    up to 16 polynomials."""
    cv = key.curve
    n = _domain_size(key)
    count = len(polynomials)
    if count == 0 or count > COSETS_MULTI_MAX:
        raise ValueError("invalid number of polynomials, got %d, one call takes 1..%d" % (count, COSETS_MULTI_MAX))
    for b, p in enumerate(polynomials):
        if len(p) == 0 or len(p) > n:
            raise ValueError("invalid size of polynomial %d, got %d coefficients, the domain takes 1..%d" % (b, len(p), n))
    l = getattr(key, "kzg_coset_size", None)
    if l is None:
        raise ValueError("PrepareCosets(key, srs, coset_size) comes first")
    w, np = 2 * cv.fp_bytes, n // l
    encoded = {}
    for p in polynomials:
        if id(p) not in encoded:
            encoded[id(p)] = C.create_string_buffer(bytes(cv.fr_vector(p)), 32 * len(p))
    ptrs = (C.c_void_p * count)(*[C.addressof(encoded[id(p)]) for p in polynomials])
    lens = (C.c_uint64 * count)(*[len(p) for p in polynomials])
    h, vals = C.create_string_buffer(w * np * count), C.create_string_buffer(32 * n * count)
    check(lib.apk_kzg_open_cosets_multi(key.ctx, count, ptrs, lens, h, vals))
    values = cv.fr_vector_decode(vals.raw)
    return [[CosetOpeningProof(cv.g1_from_bytes(h.raw[(b * np + i) * w:(b * np + i + 1) * w]), values[b * n + i * l:b * n + (i + 1) * l])
             for i in range(np)] for b in range(count)]


def VerifyCoset(commitment: ecc.Point, proof: CosetOpeningProof, index: int, coset_size: int, vk: "VerifyingKey", g2_tau_l: bytes,
                srs, n: Optional[int] = None) -> None:
    """One pairing check for the coset_size openings of coset `index`: raises VerificationError when they are rejected.  g2_tau_l:
    [tau^coset_size]G2 in the form of VerifyingKey.G2's points; srs: a setup.SRS or its G1 bytes (the first coset_size points are
    read); n: the domain's size (default: len(srs) rounded down to a power of two - a setup.SRS made for the domain)."""
    cv = vk.curve
    g1 = srs if isinstance(srs, (bytes, bytearray)) else srs.g1
    w = 2 * cv.fp_bytes
    count = len(g1) // w
    if n is None:
        n = 1 << (count.bit_length() - 1) if count else 0
    l = int(coset_size)
    if len(proof.ClaimedValues) != l or count < l:
        raise VerificationError("invalid coset opening, got %d values and %d SRS points for cosets of %d" % (len(proof.ClaimedValues), count, l))
    if len(g2_tau_l) != 4 * cv.fp_bytes:
        raise ValueError("invalid G2 point, got %d bytes" % len(g2_tau_l))
    rv = vk.raw()
    _verdict(lib.apk_kzg_verify_coset(C.byref(rv), bytes(g2_tau_l), bytes(g1[:l * w]), n, l, index, cv.g1_to_bytes(commitment),
                                      cv.fr_vector(list(proof.ClaimedValues)), cv.g1_to_bytes(proof.H)))


def _cosets_args(digests, digest_of, indices, proofs, coset_size, vk, g2_tau_l, n):
    """The argument list apk_kzg_batch_verify_cosets and apk_kzg_cosets_weights share, after the checks Python can make"""
    cv = vk.curve
    k, l = len(proofs), int(coset_size)
    if k == 0 or len(digests) == 0:
        raise VerificationError("invalid batch (no digest, or no proof)")
    if len(digest_of) != k or len(indices) != k:
        raise VerificationError("invalid number of digest_of / indices, got %d / %d, expected %d" % (len(digest_of), len(indices), k))
    if any(len(p.ClaimedValues) != l for p in proofs):
        raise VerificationError("invalid coset opening (a proof has not %d values)" % l)
    if any(not 0 <= int(d) < len(digests) for d in digest_of):
        raise VerificationError("invalid digest_of (an entry is not below the %d digests)" % len(digests))
    if len(g2_tau_l) != 4 * cv.fp_bytes:
        raise ValueError("invalid G2 point, got %d bytes" % len(g2_tau_l))
    values = cv.fr_vector([v for p in proofs for v in p.ClaimedValues])
    return (bytes(g2_tau_l), int(n), l, len(digests), cv.g1_vector(list(digests)), k, (C.c_uint32 * k)(*[int(d) for d in digest_of]),
            (C.c_uint64 * k)(*[int(i) for i in indices]), values, cv.g1_vector([p.H for p in proofs]))


def BatchVerifyCosets(digests: Sequence[ecc.Point], digest_of: Sequence[int], indices: Sequence[int], proofs: Sequence[CosetOpeningProof],
                      coset_size: int, vk: "VerifyingKey", g2_tau_l: bytes, srs, n: Optional[int] = None, device: int = -1) -> None:
    """One pairing check for many coset openings: proofs[k] opens digests[digest_of[k]] on coset indices[k] (OpenCosets' entry
    indices[k]).  Rows may repeat.  The fold runs on the host (device = -1) or on that GPU.  g2_tau_l, srs and n as for VerifyCoset.
    Raises VerificationError when the batch is rejected - it does not say which row is wrong."""
    cv = vk.curve
    g1 = srs if isinstance(srs, (bytes, bytearray)) else srs.g1
    w = 2 * cv.fp_bytes
    count = len(g1) // w
    if n is None:
        n = 1 << (count.bit_length() - 1) if count else 0
    if count < int(coset_size):
        raise VerificationError("invalid SRS, got %d points for cosets of %d" % (count, int(coset_size)))
    a = _cosets_args(digests, digest_of, indices, proofs, coset_size, vk, g2_tau_l, n)
    rv = vk.raw()
    _verdict(lib.apk_kzg_batch_verify_cosets(C.byref(rv), device, a[0], bytes(g1[:int(coset_size) * w]), *a[1:]))


def CosetsWeights(digests: Sequence[ecc.Point], digest_of: Sequence[int], indices: Sequence[int], proofs: Sequence[CosetOpeningProof],
                  coset_size: int, vk: "VerifyingKey", g2_tau_l: bytes, n: int) -> List[int]:
    """The weights BatchVerifyCosets folds the rows with: hashed from the statement, so that a verdict can be reproduced"""
    cv = vk.curve
    a = _cosets_args(digests, digest_of, indices, proofs, coset_size, vk, g2_tau_l, n)
    out = C.create_string_buffer(32 * len(proofs))
    rv = vk.raw()
    check(lib.apk_kzg_cosets_weights(C.byref(rv), *a, out))
    return cv.fr_vector_decode(out.raw)


def _recover_args(indices, proofs_or_rows, coset_size, length, key):
    """(l, count, indices as uint64[], the rows' bytes, length) after the checks Python can make; a row is a CosetOpeningProof or its
    coset_size values"""
    n = _domain_size(key)
    l = _coset_size(n, coset_size)
    rows = [list(r.ClaimedValues) if isinstance(r, CosetOpeningProof) else list(r) for r in proofs_or_rows]
    k = len(rows)
    if k == 0 or len(indices) != k:
        raise ValueError("invalid cells, got %d rows for %d indices" % (k, len(indices)))
    if any(len(r) != l for r in rows):
        raise ValueError("invalid cells (a row has not %d values)" % l)
    if not 1 <= int(length) <= k * l:
        raise ValueError("invalid polynomial size %d, %d cells of %d points give 1..%d coefficients" % (int(length), k, l, k * l))
    return l, k, (C.c_uint64 * k)(*[int(i) for i in indices]), key.curve.fr_vector([v for r in rows for v in r]), int(length)


def RecoverCosets(indices: Sequence[int], proofs_or_rows, coset_size: int, length: int, key) -> List[int]:
    """The `length` coefficients of the polynomial whose cells - OpenCosets' entries indices[r], or just their values - are given:
    any k cells of coset_size points determine a polynomial of up to k * coset_size coefficients.  Needs no PrepareCosets.  Raises
    VerificationError when the rows are not cells of one polynomial of `length` coefficients."""
    cv = key.curve
    l, k, idx, rows, length = _recover_args(indices, proofs_or_rows, coset_size, length, key)
    out = C.create_string_buffer(32 * length)
    _verdict(lib.apk_kzg_recover_cosets(key.ctx, l, k, idx, rows, length, out))
    return cv.fr_vector_decode(out.raw)


def RecoverCosetsAndProofs(indices: Sequence[int], proofs_or_rows, coset_size: int, length: int, key) -> List[CosetOpeningProof]:
    """recover_cells_and_kzg_proofs: every cell and proof of the polynomial - OpenCosets' answer - from a sufficient set of cells.  The
    polynomial is recovered into device memory and opened there; PrepareCosets(key, srs, coset_size) comes first."""
    cv = key.curve
    l, k, idx, rows, length = _recover_args(indices, proofs_or_rows, coset_size, length, key)
    if getattr(key, "kzg_coset_size", None) != l:
        raise ValueError("PrepareCosets(key, srs, %d) comes first" % l)
    n = _domain_size(key)
    w, np = 2 * cv.fp_bytes, n // l
    d_rows, d_poly = C.c_void_p(), C.c_void_p()
    try:
        check(lib.apk_device_alloc(key.ctx, len(rows), C.byref(d_rows)))
        check(lib.apk_device_alloc(key.ctx, 32 * length, C.byref(d_poly)))
        check(lib.apk_device_upload(key.ctx, d_rows, rows, len(rows)))
        _verdict(lib.apk_kzg_recover_cosets_device(key.ctx, l, k, idx, d_rows, length, d_poly))
        h, vals = C.create_string_buffer(w * np), C.create_string_buffer(32 * n)
        check(lib.apk_kzg_open_cosets_device(key.ctx, d_poly, length, h, vals))
    finally:
        for d in (d_rows, d_poly):
            if d:
                lib.apk_device_free(key.ctx, d)
    values = cv.fr_vector_decode(vals.raw)
    return [CosetOpeningProof(cv.g1_from_bytes(h.raw[i * w:(i + 1) * w]), values[i * l:(i + 1) * l]) for i in range(np)]


def _verdict(rc: int) -> None:
    if rc == _lib.APK_ERR_VERIFY:
        raise VerificationError((lib.apk_last_error() or b"").decode())
    check(rc)


def Verify(commitment: ecc.Point, proof: OpeningProof, point: int, vk: VerifyingKey) -> None:
    """kzg.Verify(&commitment, &proof, point, vk): raises VerificationError when the opening is rejected."""
    cv = vk.curve
    rv = vk.raw()
    _verdict(lib.apk_kzg_verify(C.byref(rv), cv.g1_to_bytes(commitment), cv.fr_vector([point]), cv.fr_vector([proof.ClaimedValue]),
                                cv.g1_to_bytes(proof.H)))


def BatchVerifyMultiPoints(digests: Sequence[ecc.Point], proofs: Sequence[OpeningProof], points: Sequence[int], vk: VerifyingKey,
                           device: int = -1) -> None:
    """kzg.BatchVerifyMultiPoints(digests, proofs, points, vk): one pairing check for all the openings; the fold runs on the host
    (device = -1) or on that GPU.  Raises VerificationError when the batch is rejected - it does not say which opening is wrong."""
    cv = vk.curve
    k = len(digests)
    if k == 0:
        raise VerificationError("invalid number of digests (none)")
    if len(proofs) != k or len(points) != k:
        raise VerificationError("invalid number of proofs / points, got %d / %d, expected %d" % (len(proofs), len(points), k))
    rv = vk.raw()
    _verdict(lib.apk_kzg_batch_verify_multi(C.byref(rv), device, k, cv.g1_vector(digests), cv.fr_vector(list(points)),
                                            cv.fr_vector([p.ClaimedValue for p in proofs]), cv.g1_vector([p.H for p in proofs])))


def BatchVerifySinglePoint(digests: Sequence[ecc.Point], batchOpeningProof: BatchOpeningProof, point: int, vk: VerifyingKey,
                           dataTranscript: bytes = b"") -> None:
    """kzg.BatchVerifySinglePoint(digests, &proof, point, hf, vk, dataTranscript...)"""
    cv = vk.curve
    if len(digests) != len(batchOpeningProof.ClaimedValues):
        raise VerificationError("invalid number of digests, got %d, expected %d" % (len(digests), len(batchOpeningProof.ClaimedValues)))
    rv = vk.raw()
    _verdict(lib.apk_kzg_batch_verify(C.byref(rv), len(digests), cv.g1_vector(digests), cv.fr_vector(batchOpeningProof.ClaimedValues),
                                      cv.fr_vector([point]), dataTranscript or None, len(dataTranscript), cv.g1_to_bytes(batchOpeningProof.H)))

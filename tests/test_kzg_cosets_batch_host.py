"""CPU tier of the batched coset verifier (include/apk.h apk_kzg_batch_verify_cosets, apk_kzg_cosets_weights, apk_kzg_cosets_fold;
csrc/kzg_protocol.h cosets_*), device -1 throughout: the weights against a restatement of their hash, the fold against the
big-integer interpolation of tests/kzg_cosets_model.py, the rule on proofs the model makes (accepted batches, every rejection,
errors that cancel under equal weights), the argument errors and their place before the device check, the rule stand-alone under
ASAN + UBSAN, the exports and the Python wrapper."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess

import pytest

import kzg_cosets_model as kcm
import kzg_model as km
from algoplonk_amd import _lib, kzg as ap_kzg
from algoplonk_amd._lib import lib
from helpers import CURVES
from oracle.prng import SplitMix64
from test_kzg_cosets_host import made

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
NAMES = ["bn254", "bls12-381"]
OK, ERR_ARG, ERR_HIP, ERR_VERIFY = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_HIP, _lib.APK_ERR_VERIFY
NEW = ["apk_kzg_batch_verify_cosets", "apk_kzg_cosets_weights", "apk_kzg_cosets_fold"]
RULE_SHAPES = [(8, 2), (8, 4), (64, 8)]


def u32s(xs):
    return (C.c_uint32 * len(xs))(*xs)


def u64s(xs):
    return (C.c_uint64 * len(xs))(*xs)


# ---- the fold -------------------------------------------------------------------------------------------------------------------------
def lib_fold(cv, n, l, indices, weights, rows, device=-1):
    """(code, the l coefficients) of apk_kzg_cosets_fold"""
    out = C.create_string_buffer(32 * l)
    rc = lib.apk_kzg_cosets_fold(cv.abi, device, n, l, len(rows), u64s(indices), cv.fr_vector(weights), cv.fr_vector([v for row in rows for v in row]), out)
    return rc, cv.fr_vector_decode(out.raw)


def model_fold(cv, n, l, indices, weights, rows):
    r, w = cv.r, cv.omega(n)
    q = [0] * l
    for i, wt, row in zip(indices, weights, rows):
        if wt == 0 or not any(row):
            continue
        q = [(a + wt * b) % r for a, b in zip(q, kcm.interpolate(row, n, l, i, w, r))]
    return q


def fold_rows(cv, n, l, count, g):
    """`count` rows for a fold: structured weights (0, 1, r - 1, random), values (zeros, all r - 1, a few entries, random; ONE dense
    random row at most - the model's transform is quadratic) and indices (0, n / l - 1, repeated)"""
    r, np = cv.r, n // l
    weights = [[1, 0, r - 1][k] if k < 3 else g.fr(r) for k in range(count)] if count > 1 else [g.fr(r)]
    indices = [[np - 1, 0, np - 1][k] if k < 3 else g.fr(r) % np for k in range(count)]
    rows = []
    for k in range(count):
        if k == 0:
            rows.append([g.fr(r) for _ in range(l)])
        elif k == 1:
            rows.append([0] * l)
        elif k == 2:
            rows.append([r - 1] * l if l <= 64 else [r - 1 if j % 97 == 0 else 0 for j in range(l)])
        else:
            rows.append([g.fr(r) if l <= 64 or j % 131 == k else 0 for j in range(l)])
    return indices, weights, rows


@pytest.mark.parametrize("shape", [(8, 2), (8, 4), (64, 8), (4096, 1024), (1 << 20, 2)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cname", NAMES)
def test_fold_is_the_weighted_sum_of_the_interpolants(cname, shape):
    cv, _ = CURVES[cname]
    n, l = shape
    g = SplitMix64(0xF01D + cv.abi + n + l)
    for count in (1, 3, 7):
        indices, weights, rows = fold_rows(cv, n, l, count, g)
        rc, got = lib_fold(cv, n, l, indices, weights, rows)
        assert rc == OK, lib.apk_last_error()
        assert got == model_fold(cv, n, l, indices, weights, rows), (shape, count)
    # weight r - 1 on a row of r - 1 at the last coset; the same row with weights that cancel
    rows = [[cv.r - 1] * min(l, 64) + [0] * (l - min(l, 64))] * 2
    rc, got = lib_fold(cv, n, l, [n // l - 1] * 2, [cv.r - 1, 0], rows)
    assert rc == OK and got == model_fold(cv, n, l, [n // l - 1] * 2, [cv.r - 1, 0], rows)
    rc, got = lib_fold(cv, n, l, [n // l - 1] * 2, [5, cv.r - 5], rows)
    assert rc == OK and got == [0] * l


@pytest.mark.parametrize("cname", NAMES)
def test_fold_argument_errors_come_before_the_device(cname):
    cv, _ = CURVES[cname]
    n, l = 8, 2
    good = dict(curve=cv.abi, device=-1, n=n, l=l, count=2, indices=u64s([0, 3]), weights=cv.fr_vector([1, 2]), values=cv.fr_vector([1, 2, 3, 4]))
    mark = b"\xa5" * (32 * l)

    def call(**kw):
        a = dict(good, **kw)
        out = a.pop("out", None) or C.create_string_buffer(mark, len(mark))
        rc = lib.apk_kzg_cosets_fold(a["curve"], a["device"], a["n"], a["l"], a["count"], a["indices"], a["weights"], a["values"],
                                     None if kw.get("out") is False else out)
        return rc, out.raw

    assert call()[0] == OK
    over = b"\xff" * 32
    bad = [dict(curve=7), dict(device=-2), dict(n=0), dict(n=12), dict(n=2), dict(l=0), dict(l=1), dict(l=3), dict(l=8), dict(n=1 << 40),
           dict(count=0), dict(count=(1 << 20) + 1), dict(indices=u64s([0, 4])), dict(indices=u64s([1 << 63, 0])),
           dict(weights=cv.fr_vector([1]) + over), dict(values=cv.fr_vector([1, 2, 3]) + over),
           dict(indices=None), dict(weights=None), dict(values=None), dict(out=False)]
    for kw in bad:
        for device in (-1, 0):
            rc, raw = call(**dict(dict(device=device), **kw))
            assert rc == ERR_ARG, kw
            assert lib.apk_last_error(), kw
            assert raw == mark, kw
    if _lib.device_count() == 0:
        rc, raw = call(device=0)
        assert rc == ERR_HIP and b"no CPU fallback" in lib.apk_last_error() and raw == mark
        assert lib.apk_kzg_cosets_fold(cv.abi, 0, 1 << 12, 1 << 11, 1, u64s([1]), cv.fr_vector([1]), cv.fr_vector([1] * 2048),
                                       C.create_string_buffer(32 << 11)) == ERR_HIP         # a coset size the host interpolates


# ---- the weights --------------------------------------------------------------------------------------------------------------------
def model_weights(cv, ov, g2_0: bytes, g2_tau_l: bytes, n, l, digests, digest_of, indices, rows, hs):
    """The rule, restated:  r_k = sha256(be32(digest_of[k]) || be64(index[k]) || the row's l values || H_k),
    D = sha256(be32(curve) || g1 || g2[0] || g2_tau_l || be64(n) || be32(l) || be32(nb_digests) || the digests || be32(count) || r_0 ..),
    lambda_0 = 1, lambda_j = the low 128 bits of sha256("apk-kzg-cosets" || D || be32(j))"""
    h = hashlib.sha256()
    h.update(cv.abi.to_bytes(4, "big") + ov.raw_bytes(ov.g1) + g2_0 + g2_tau_l + n.to_bytes(8, "big") + l.to_bytes(4, "big"))
    h.update(len(digests).to_bytes(4, "big"))
    for d in digests:
        h.update(ov.raw_bytes(d))
    h.update(len(rows).to_bytes(4, "big"))
    for d, i, row, H in zip(digest_of, indices, rows, hs):
        h.update(hashlib.sha256(d.to_bytes(4, "big") + i.to_bytes(8, "big") + b"".join(v.to_bytes(32, "big") for v in row) + ov.raw_bytes(H)).digest())
    D = h.digest()
    return [1] + [int.from_bytes(hashlib.sha256(b"apk-kzg-cosets" + D + j.to_bytes(4, "big")).digest()[16:], "big") for j in range(1, len(rows))]


class Pair:
    """Two polynomials over one tau, every coset proof of both by the model (the first is tests/test_kzg_cosets_host.py's Made)"""

    def __init__(self, cname, n, l):
        m = self.m = made(cname, n, l)
        cv, ov, r = m.cv, m.ov, m.cv.r
        self.cv, self.ov, self.n, self.l, self.np = cv, ov, n, l, n // l
        self.g2_0 = m.g2[:4 * cv.fp_bytes]
        self.g2_l = m.tau_pow_g2(l)
        self.digests = [km.commit(ov, m.f, m.tau), km.commit(ov, m.other, m.tau)]
        self.h_scalars = [kcm.direct(f, n, l, m.w, m.tau, r) for f in (m.f, m.other)]
        self.hs = [[ov.mul(ov.g1, k) if k else None for k in hk] for hk in self.h_scalars]
        self.values = [m.values, kcm.values_by_coset(m.other, n, l, m.w, r)]

    def row(self, p, i):
        """(digest_of, index, values, H)"""
        return p, i, self.values[p][i * self.l:(i + 1) * self.l], self.hs[p][i]

    def all_of(self, p):
        return [self.row(p, i) for i in range(self.np)]

    def interleaved(self):
        return [self.row(p, i if p == 0 else self.np - 1 - i) for i in range(self.np) for p in (0, 1)]

    def verify(self, rows, digests=None, g2_tau_l=None, srs=None, vk=None, n=None, l=None, device=-1, nb_digests=None, count=None):
        cv = self.cv
        digests = self.digests[:1 + max(r[0] for r in rows)] if digests is None else digests
        return lib.apk_kzg_batch_verify_cosets(C.byref(vk or self.m.vk), device, g2_tau_l or self.g2_l, srs or self.m.srs, self.n if n is None else n,
                                               self.l if l is None else l, len(digests) if nb_digests is None else nb_digests, cv.g1_vector(digests),
                                               len(rows) if count is None else count, u32s([r[0] for r in rows]), u64s([r[1] for r in rows]),
                                               cv.fr_vector([v for r in rows for v in r[2]]), cv.g1_vector([r[3] for r in rows]))

    def weights(self, rows, digests=None):
        cv = self.cv
        digests = self.digests[:1 + max(r[0] for r in rows)] if digests is None else digests
        out = C.create_string_buffer(32 * len(rows))
        rc = lib.apk_kzg_cosets_weights(C.byref(self.m.vk), self.g2_l, self.n, self.l, len(digests), cv.g1_vector(digests), len(rows),
                                        u32s([r[0] for r in rows]), u64s([r[1] for r in rows]), cv.fr_vector([v for r in rows for v in r[2]]),
                                        cv.g1_vector([r[3] for r in rows]), out)
        assert rc == OK, lib.apk_last_error()
        return cv.fr_vector_decode(out.raw)

    def short(self):
        """(digest, row) of a polynomial below degree l on coset 0: its own remainder, H = infinity"""
        m = self.m
        f = m.f[:self.l]
        return km.commit(self.ov, f, m.tau), kcm.values_by_coset(f, self.n, self.l, m.w, self.cv.r)[:self.l]


_PAIRS = {}


def pair(cname, n, l) -> Pair:
    if (cname, n, l) not in _PAIRS:
        _PAIRS[(cname, n, l)] = Pair(cname, n, l)
    return _PAIRS[(cname, n, l)]


@pytest.mark.parametrize("cname", NAMES)
def test_weights_are_the_rules(cname):
    p = pair(cname, 8, 2)
    cv, ov = p.cv, p.ov
    d_short, v_short = p.short()
    batches = [(p.all_of(0), p.digests[:1]), (p.interleaved(), p.digests), ([p.row(0, 1)], p.digests[:1]),
               (p.all_of(0) + [p.row(0, 2)] + [(1, 0, v_short, None)], [p.digests[0], d_short])]        # a repeated row, H = infinity
    for rows, digests in batches:
        got = p.weights(rows, digests)
        want = model_weights(cv, ov, p.g2_0, p.g2_l, p.n, p.l, digests, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
        assert got == want and got[0] == 1 and all(0 <= w < 1 << 128 for w in got[1:])
    # what the caller hands in moves the weights
    rows = p.all_of(0)
    base = p.weights(rows)
    moved = list(rows)
    moved[3] = (0, 3, [rows[3][2][0], (rows[3][2][1] + 1) % cv.r], rows[3][3])
    assert p.weights(moved)[1:] != base[1:]
    moved[3] = (0, 2, rows[3][2], rows[3][3])
    assert p.weights(moved)[1:] != base[1:]
    assert p.weights(rows, [p.digests[1]])[1:] != base[1:]


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RULE_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cname", NAMES)
def test_batches_accepted_and_what_is_wrong_rejected(cname, shape):
    p = pair(cname, *shape)
    cv, ov, r, np, l = p.cv, p.ov, p.cv.r, p.np, p.l
    assert p.verify(p.all_of(0)) == OK, lib.apk_last_error()
    both = p.interleaved()
    assert p.verify(both) == OK, lib.apk_last_error()
    assert p.verify(both + both[:3]) == OK, lib.apk_last_error()                        # repeated (commitment, coset) pairs

    def changed(rows, k, **kw):
        out = list(rows)
        d = dict(zip(("digest_of", "index", "values", "h"), out[k]), **kw)
        out[k] = (d["digest_of"], d["index"], d["values"], d["h"])
        return out

    k = len(both) // 2
    vals = list(both[k][2])
    vals[l - 1] = (vals[l - 1] + 1) % r
    assert p.verify(changed(both, k, values=vals)) == ERR_VERIFY                        # one changed value in one row
    assert b"do not verify" in lib.apk_last_error()
    rows = p.all_of(0)
    if np > 2:
        swapped = changed(changed(rows, 0, h=rows[np - 1][3]), np - 1, h=rows[0][3])
        assert p.verify(swapped) == ERR_VERIFY                                          # two rows' H swapped
    else:
        assert rows[0][3] == rows[1][3]                                                 # n' = 2: both cosets have the one proof
    assert p.verify(changed(both, 1, digest_of=0)) == ERR_VERIFY                        # a row pointing at the other polynomial
    assert p.verify(changed(rows, np - 1, index=np - 2)) == ERR_VERIFY                  # an index off by one
    assert p.verify(rows, g2_tau_l=p.m.tau_pow_g2(l // 2)) == ERR_VERIFY                # [tau^(l/2)]G2
    # the same row twice, H + P in one copy and H - P in the other: equal weights would accept it
    s, P = p.h_scalars[0][0], 5
    twice = [(0, 0, rows[0][2], ov.mul(ov.g1, (s + P) % r)), (0, 0, rows[0][2], ov.mul(ov.g1, (s - P) % r))]
    assert p.verify(twice) == ERR_VERIFY
    assert p.verify([rows[0], rows[0]]) == OK
    # a polynomial below degree l, H = infinity, beside ordinary rows
    d_short, v_short = p.short()
    assert p.verify(rows + [(1, 0, v_short, None)], digests=[p.digests[0], d_short]) == OK, lib.apk_last_error()
    assert p.verify(rows + [(1, 0, v_short, rows[0][3])], digests=[p.digests[0], d_short]) == ERR_VERIFY
    # points outside the group: the message says which kind
    off = (1, 3)
    assert p.verify(changed(rows, 0, h=off)) == ERR_VERIFY and b"proof is not a point" in lib.apk_last_error()
    assert p.verify(rows, digests=[off]) == ERR_VERIFY and b"digest is not a point" in lib.apk_last_error()


@pytest.mark.parametrize("cname", NAMES)
def test_a_batch_of_one_gives_verify_cosets_verdict(cname):
    p = pair(cname, 64, 8)
    m, r = p.m, p.cv.r
    for i in (0, p.np - 1):
        row = p.row(0, i)
        assert m.verify(i) == OK and p.verify([row]) == OK
        bad = list(row[2])
        bad[0] = (bad[0] + 1) % r
        assert m.verify(i, values=bad) == ERR_VERIFY and p.verify([(0, i, bad, row[3])]) == ERR_VERIFY
        assert m.verify(i, h=m.h[(i + 1) % p.np]) == ERR_VERIFY and p.verify([(0, i, row[2], p.hs[0][(i + 1) % p.np])]) == ERR_VERIFY


@pytest.mark.parametrize("cname", NAMES)
def test_verify_argument_errors_come_before_the_device(cname):
    p = pair(cname, 8, 2)
    cv, m = p.cv, p.m
    rows = p.interleaved()
    assert p.verify(rows) == OK
    devices = (-1, 0)
    for kw in (dict(n=0), dict(n=12), dict(n=2), dict(l=0), dict(l=1), dict(l=3), dict(l=8), dict(n=1 << 40), dict(count=0),
               dict(count=(1 << 20) + 1), dict(nb_digests=0), dict(nb_digests=len(rows) + 1), dict(device=-2)):
        for device in devices:
            assert p.verify(rows, **dict(dict(device=device), **kw)) == ERR_ARG, kw
            assert lib.apk_last_error(), kw
    for device in devices:
        assert p.verify(rows, digests=p.digests[:1], device=device) == ERR_ARG                  # digest_of = 1 with one digest
        assert p.verify([(0, 4, rows[0][2], rows[0][3])], device=device) == ERR_ARG             # index = n / l
        assert p.verify([(0, 1 << 63, rows[0][2], rows[0][3])], device=device) == ERR_ARG
        bad = km.kzg_vk(cv, m.g2)
        bad.g2[0][0] ^= 1
        assert p.verify(rows, vk=bad, device=device) == ERR_ARG
        off = bytearray(p.g2_l)
        off[0] ^= 1
        assert p.verify(rows, g2_tau_l=bytes(off), device=device) == ERR_ARG
        unknown = km.kzg_vk(cv, m.g2)
        unknown.curve = 7
        assert p.verify(rows, vk=unknown, device=device) == ERR_ARG
        srs = bytearray(m.srs)
        srs[0] ^= 1
        assert p.verify(rows, srs=bytes(srs), device=device) == ERR_ARG
    k = len(rows)
    good = [C.byref(m.vk), -1, p.g2_l, m.srs, 8, 2, 2, cv.g1_vector(p.digests), k, u32s([r[0] for r in rows]), u64s([r[1] for r in rows]),
            cv.fr_vector([v for r in rows for v in r[2]]), cv.g1_vector([r[3] for r in rows])]
    assert lib.apk_kzg_batch_verify_cosets(*good) == OK
    for device in devices:
        for at in (0, 2, 3, 7, 9, 10, 11, 12):
            args = list(good)
            args[1], args[at] = device, None
            assert lib.apk_kzg_batch_verify_cosets(*args) == ERR_ARG, at
            assert lib.apk_last_error()
        raw = bytearray(good[11])
        raw[32 * (2 * k - 1):] = b"\xff" * 32                                                   # the last scalar is not below r
        args = list(good)
        args[1], args[11] = device, bytes(raw)
        assert lib.apk_kzg_batch_verify_cosets(*args) == ERR_ARG
    # the weights: the same checks, no SRS
    out = C.create_string_buffer(32 * k)
    wgood = [good[0], good[2]] + good[4:] + [out]
    assert lib.apk_kzg_cosets_weights(*wgood) == OK
    for at in (0, 1, 5, 7, 8, 9, 10, 11):
        args = list(wgood)
        args[at] = None
        assert lib.apk_kzg_cosets_weights(*args) == ERR_ARG, at
    if _lib.device_count() == 0:
        args = list(good)
        args[1] = 0
        assert lib.apk_kzg_batch_verify_cosets(*args) == ERR_HIP
        assert b"no CPU fallback" in lib.apk_last_error()


# ---- the host rule, stand-alone under ASAN + UBSAN ---------------------------------------------------------------------------------
def test_cosets_batch_check_under_address_and_undefined_sanitizers():
    r = subprocess.run(["make", "-C", CSRC, "san-kzg-cosets-batch"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "san", "kzg_cosets_batch_check")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "KZG COSETS BATCH CHECK OK" in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    # the folds it printed, held to the model:  Q <curve> <n> <l> <count> : <indices> : <weights> : <count x l values> : <l coefficients>
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("Q ")]
    assert len(lines) == 6
    for t in lines:
        abi, n, l, count = (int(x) for x in t[1:5])
        cv = [CURVES[c][0] for c in NAMES if CURVES[c][0].abi == abi][0]
        at = 6
        indices = [int(x) for x in t[at:at + count]]
        at += count + 1
        weights = [int(x, 16) for x in t[at:at + count]]
        at += count + 1
        vals = [int(x, 16) for x in t[at:at + count * l]]
        at += count * l + 1
        q = [int(x, 16) for x in t[at:at + l]]
        assert len(q) == l and weights[0] == 1 and len(set(weights)) == count
        assert model_fold(cv, n, l, indices, weights, [vals[k * l:(k + 1) * l] for k in range(count)]) == q, t[:5]


# ---- the exports and the Python wrapper ------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and ("int %s(" % name) in hdr
        assert getattr(lib, name).argtypes is not None, name
    assert _lib.ABI_VERSION == 5 and lib.apk_abi_version() == 5 and "#define APK_ABI_VERSION 5" in hdr          # additive
    assert "a batched verifier that folds" not in hdr


def test_python_wrapper():
    p = pair("bn254", 8, 2)
    cv, m = p.cv, p.m
    vk = ap_kzg.VerifyingKey(cv, cv.g1, m.g2)
    rows = p.interleaved()
    proofs = [ap_kzg.CosetOpeningProof(r[3], list(r[2])) for r in rows]
    digest_of, indices = [r[0] for r in rows], [r[1] for r in rows]
    ap_kzg.BatchVerifyCosets(p.digests, digest_of, indices, proofs, 2, vk, p.g2_l, m.srs, n=8)
    assert ap_kzg.CosetsWeights(p.digests, digest_of, indices, proofs, 2, vk, p.g2_l, 8) == p.weights(rows)
    bad = [ap_kzg.CosetOpeningProof(q.H, list(q.ClaimedValues)) for q in proofs]
    bad[2].ClaimedValues[1] = (bad[2].ClaimedValues[1] + 1) % cv.r
    with pytest.raises(ap_kzg.VerificationError, match="do not verify"):
        ap_kzg.BatchVerifyCosets(p.digests, digest_of, indices, bad, 2, vk, p.g2_l, m.srs, n=8)
    for kw in (dict(proofs=[]), dict(digests=[]), dict(digest_of=digest_of[:-1]), dict(indices=indices + [0]), dict(digest_of=[2] + digest_of[1:]),
               dict(proofs=[ap_kzg.CosetOpeningProof(proofs[0].H, [1])] + proofs[1:]), dict(srs=m.srs[:2 * cv.fp_bytes])):
        a = dict(dict(digests=p.digests, digest_of=digest_of, indices=indices, proofs=proofs, srs=m.srs), **kw)
        with pytest.raises(ap_kzg.VerificationError):
            ap_kzg.BatchVerifyCosets(a["digests"], a["digest_of"], a["indices"], a["proofs"], 2, vk, p.g2_l, a["srs"], n=8)
    with pytest.raises(ValueError):
        ap_kzg.BatchVerifyCosets(p.digests, digest_of, indices, proofs, 2, vk, b"\0" * 5, m.srs, n=8)
    with pytest.raises(_lib.ApkError):
        ap_kzg.BatchVerifyCosets(p.digests, digest_of, indices, proofs, 2, vk, p.g2_l, m.srs, n=12)        # the library's argument error

"""CPU tier: kzg.BatchVerifyMultiPoints on the host (include/apk.h apk_kzg_batch_verify_multi with device = -1,
apk_kzg_multi_weights; csrc/kzg_protocol.h) against openings made in big integers with a known tau (tests/kzg_model.py): the
unaltered batch, every single alteration, errors that cancel under equal weights, the weights against a restatement of their
rule, bad points / scalars / keys against what apk_kzg_verify answers for the same fault, the first-HIP-call record of the new
exports, and the rule once more stand-alone under ASAN + UBSAN."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import pytest

import kzg_model as km
from algoplonk_amd import _lib, kzg as ap_kzg, setup as ap_setup
from algoplonk_amd._lib import lib
from helpers import CURVES
from oracle import curves as ocurves
from oracle.prng import SplitMix64, tau_from_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
NAMES = ["bn254", "bls12-381"]
COUNTS = [1, 2, 3, 17]
OK, ERR_ARG, ERR_HIP, ERR_VERIFY = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_HIP, _lib.APK_ERR_VERIFY


class Material:
    """17 openings per curve, made by the model: polynomials of 1 .. 9 coefficients (a constant among them: H = infinity), each
    at its own point; the first N of them are the batch of N."""

    def __init__(self, cname: str):
        self.cv, self.ov = CURVES[cname]
        cv, ov = self.cv, self.ov
        r = cv.r
        g = SplitMix64(0x4D554C + cv.abi)
        self.tau = tau_from_seed(0x4D55, r)
        self.g2 = ap_setup.g2_from_tau(cv, self.tau)
        self.vk = km.kzg_vk(cv, self.g2)
        self.digests, self.points, self.values, self.hs = [], [], [], []
        for i in range(max(COUNTS)):
            f = km.polynomial("random", 1 if i == 3 else 2 + (5 * i) % 8, r, g)
            z = g.fr(r)
            H, v = km.open_at(ov, f, z, self.tau)
            self.digests.append(km.commit(ov, f, self.tau)); self.points.append(z); self.values.append(v); self.hs.append(H)
        assert self.hs[3] is None
        self.other = ov.mul(ov.g1, g.fr(r))

    def batch(self, n):
        return self.digests[:n], self.points[:n], self.values[:n], self.hs[:n]


_MAT = {}


def material(cname: str) -> Material:
    if cname not in _MAT:
        _MAT[cname] = Material(cname)
    return _MAT[cname]


def multi_verify(cv, vk, digests, points, values, hs, device=-1) -> int:
    return lib.apk_kzg_batch_verify_multi(C.byref(vk), device, len(digests), cv.g1_vector(digests), cv.fr_vector(points),
                                          cv.fr_vector(values), cv.g1_vector(hs))


def model_weights(cv, ov, g2: bytes, digests, points, values, hs):
    """The weights' rule, restated: lambda_0 = 1, lambda_j = the low 128 bits of sha256("apk-kzg-multi" || D || be32(j)) with
    D = sha256(be32(curve) || g1 || g2[0] || g2[1] || be32(count) || per opening: digest, point, value, H) - G1 points in the
    transcript's raw encoding, scalars canonical big-endian, the G2 points in their in-memory bytes."""
    h = hashlib.sha256()
    h.update(cv.abi.to_bytes(4, "big"))
    h.update(ov.raw_bytes(ov.g1))
    w = 4 * cv.fp_bytes
    h.update(g2[:w]); h.update(g2[w:2 * w])
    h.update(len(digests).to_bytes(4, "big"))
    for d, z, v, H in zip(digests, points, values, hs):
        h.update(ov.raw_bytes(d)); h.update(z.to_bytes(32, "big")); h.update(v.to_bytes(32, "big")); h.update(ov.raw_bytes(H))
    D = h.digest()
    out = [1]
    for j in range(1, len(digests)):
        out.append(int.from_bytes(hashlib.sha256(b"apk-kzg-multi" + D + j.to_bytes(4, "big")).digest()[16:], "big"))
    return out


def lib_weights(cv, vk, digests, points, values, hs):
    out = C.create_string_buffer(32 * len(digests))
    rc = lib.apk_kzg_multi_weights(C.byref(vk), len(digests), cv.g1_vector(digests), cv.fr_vector(points), cv.fr_vector(values),
                                   cv.g1_vector(hs), out)
    assert rc == OK, lib.apk_last_error()
    return cv.fr_vector_decode(out.raw)


def _alterations(m, n):
    """(what, digests, points, values, hs) with ONE field of ONE opening changed, at the first, a middle and the last position"""
    r = m.cv.r
    for pos in sorted({0, n // 2, n - 1}):
        for what in ("value", "H", "point", "digest"):
            d, z, v, h = [list(x) for x in m.batch(n)]
            if what == "value":
                v[pos] = (v[pos] + 1) % r
            elif what == "H":
                h[pos] = m.other
            elif what == "point":
                z[pos] = (z[pos] + 1) % r
            else:
                d[pos] = m.other
            yield "%s at %d" % (what, pos), d, z, v, h


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("cname", NAMES)
def test_batch_accepted_and_every_single_alteration_rejected(cname, n):
    m = material(cname)
    cv = m.cv
    assert multi_verify(cv, m.vk, *m.batch(n)) == OK, lib.apk_last_error()
    for what, d, z, v, h in _alterations(m, n):
        assert multi_verify(cv, m.vk, d, z, v, h) == ERR_VERIFY, (n, what)
    # two openings swapped as a whole are still n valid openings
    if n >= 2:
        d, z, v, h = [list(x) for x in m.batch(n)]
        for x in (d, z, v, h):
            x[0], x[n - 1] = x[n - 1], x[0]
        assert multi_verify(cv, m.vk, d, z, v, h) == OK, lib.apk_last_error()


@pytest.mark.parametrize("cname", NAMES)
def test_weights_are_the_rules(cname):
    m = material(cname)
    cv, ov = m.cv, m.ov
    for n in COUNTS:
        got = lib_weights(cv, m.vk, *m.batch(n))
        assert got == model_weights(cv, ov, m.g2, *m.batch(n)), n
        assert got[0] == 1 and all(0 <= w < 1 << 128 for w in got[1:])
    # every byte the caller hands in moves the weights: each byte of each field of each opening in turn
    n = 3
    d, z, v, h = m.batch(n)
    base = lib_weights(cv, m.vk, d, z, v, h)
    bufs = [cv.g1_vector(d), cv.fr_vector(z), cv.fr_vector(v), cv.g1_vector(h)]
    out = C.create_string_buffer(32 * n)
    seen = {tuple(base)}
    for which, buf in enumerate(bufs):
        per = len(buf) // n
        for pos in range(n):
            for off in range(per):
                alt = bytearray(buf)
                alt[pos * per + off] ^= 1
                args = [bytes(alt) if i == which else b for i, b in enumerate(bufs)]
                rc = lib.apk_kzg_multi_weights(C.byref(m.vk), n, args[0], args[1], args[2], args[3], out)
                if rc == ERR_ARG:      # (a scalar's top byte: the altered scalar is not below r)
                    assert which in (1, 2) and int.from_bytes(alt[pos * per:(pos + 1) * per], "little") >= cv.r, (which, pos, off)
                    continue
                assert rc == OK, lib.apk_last_error()
                got = tuple(cv.fr_vector_decode(out.raw))
                assert got[0] == 1 and got[1:] != tuple(base[1:]) and got not in seen, (which, pos, off)
                seen.add(got)
    # another key (tau + 1): other weights; one opening more: other weights for the first three
    vk2 = km.kzg_vk(cv, ap_setup.g2_from_tau(cv, m.tau + 1))
    assert lib_weights(cv, vk2, d, z, v, h)[1:] != base[1:]
    assert lib_weights(cv, m.vk, *m.batch(4))[1:3] != base[1:]
    # the order of the openings matters
    assert lib_weights(cv, m.vk, d[::-1], z[::-1], v[::-1], h[::-1])[1:] != base[1:]


@pytest.mark.parametrize("cname", NAMES)
def test_errors_that_cancel_under_equal_weights_are_rejected(cname):
    """v_0 + delta and v_1 - delta: sum v_i is unchanged, so a fold with lambda_0 = lambda_1 would accept; the hashed weights
    differ, and the call rejects."""
    m = material(cname)
    cv, ov, r = m.cv, m.ov, m.cv.r
    d, z, v, h = [list(x) for x in m.batch(2)]
    # (the equal-weight fold of the unaltered pair, in the model: it holds, and it still holds with the compensated values)
    delta = 0x1234567
    bad = [(v[0] + delta) % r, (v[1] - delta) % r]
    for vals in (v, bad):
        A = ov.add(ov.add(d[0], d[1]), ov.add(ov.mul(h[0], z[0]), ov.mul(h[1], z[1])))
        A = ov.add(A, ov.mul(ov.g1, (-(vals[0] + vals[1])) % r))
        B = ov.add(h[0], h[1])
        assert A == ov.mul(B, m.tau)      # e(A, G2) = e(B, tau G2)
    assert multi_verify(cv, m.vk, d, z, v, h) == OK
    assert multi_verify(cv, m.vk, d, z, bad, h) == ERR_VERIFY
    w = lib_weights(cv, m.vk, d, z, bad, h)
    assert w[0] != w[1]


def _single(m, d, z, v, h) -> int:
    cv = m.cv
    return lib.apk_kzg_verify(C.byref(m.vk), d, z, v, h)


def _outside_subgroup(cv, ov):
    x = 1
    while True:      # the first x with a point on the curve: with a cofactor of ~2^126 such a point is outside the subgroup
        x += 1
        y = ocurves.sqrt_mod((x ** 3 + 4) % cv.p, cv.p)
        if y is not None and ov.add(ov.mul((x, y), cv.r - 1), (x, y)) is not None:
            return (x, y)


@pytest.mark.parametrize("cname", NAMES)
def test_bad_points_scalars_and_keys_answer_as_the_single_call(cname):
    m = material(cname)
    cv, ov = m.cv, m.ov
    n = 5
    w = 2 * cv.fp_bytes
    H1 = m.hs[1]
    off = (H1[0], (H1[1] + 1) % cv.p)
    assert not ov.is_on_curve(off)
    big = (cv.p).to_bytes(cv.fp_bytes, "little") + cv.g1_to_bytes(H1)[cv.fp_bytes:]      # a coordinate that is not below p
    faults = [("digest", cv.g1_to_bytes(off)), ("H", cv.g1_to_bytes(off)), ("digest", big), ("H", big),
              ("value", cv.r.to_bytes(32, "little")), ("point", cv.r.to_bytes(32, "little"))]
    if cname == "bls12-381":
        P = _outside_subgroup(cv, ov)
        faults += [("digest", cv.g1_to_bytes(P)), ("H", cv.g1_to_bytes(P))]
    for pos in (0, n - 1):
        for field, raw in faults:
            d, z, v, h = m.batch(n)
            bufs = {"digest": bytearray(cv.g1_vector(d)), "point": bytearray(cv.fr_vector(z)), "value": bytearray(cv.fr_vector(v)),
                    "H": bytearray(cv.g1_vector(h))}
            per = w if field in ("digest", "H") else 32
            bufs[field][pos * per:(pos + 1) * per] = raw
            one = {k: bytes(b[pos * (w if k in ("digest", "H") else 32):(pos + 1) * (w if k in ("digest", "H") else 32)]) for k, b in bufs.items()}
            want = _single(m, one["digest"], one["point"], one["value"], one["H"])
            assert want in (ERR_VERIFY, ERR_ARG), (field, pos)
            got = lib.apk_kzg_batch_verify_multi(C.byref(m.vk), -1, n, bytes(bufs["digest"]), bytes(bufs["point"]), bytes(bufs["value"]), bytes(bufs["H"]))
            assert got == want, (field, pos, got, want, lib.apk_last_error())
    # bad keys: garbage for a G2 point, G1 at infinity, an unknown curve - and null arguments, counts and devices out of range
    d, z, v, h = m.batch(n)
    for spoil in ("g2", "g1", "curve"):
        bad = km.kzg_vk(cv, m.g2)
        if spoil == "g2":
            bad.g2[1][0] ^= 1
        elif spoil == "g1":
            C.memset(bad.g1, 0, _lib.G1_MAX)
        else:
            bad.curve = 7
        want = km.verify(cv, bad, d[0], z[0], v[0], h[0])
        assert want == ERR_ARG and multi_verify(cv, bad, d, z, v, h) == want, spoil
    args = [cv.g1_vector(d), cv.fr_vector(z), cv.fr_vector(v), cv.g1_vector(h)]
    assert lib.apk_kzg_batch_verify_multi(None, -1, n, *args) == ERR_ARG
    for hole in range(4):
        holed = [None if i == hole else a for i, a in enumerate(args)]
        assert lib.apk_kzg_batch_verify_multi(C.byref(m.vk), -1, n, *holed) == ERR_ARG
        assert lib.apk_kzg_multi_weights(C.byref(m.vk), n, *holed, C.create_string_buffer(32 * n)) == ERR_ARG
    assert lib.apk_kzg_multi_weights(C.byref(m.vk), n, *args, None) == ERR_ARG
    assert lib.apk_kzg_batch_verify_multi(C.byref(m.vk), -2, n, *args) == ERR_ARG
    big_args = [cv.g1_vector([d[0]] * 33), cv.fr_vector([z[0]] * 33), cv.fr_vector([v[0]] * 33), cv.g1_vector([h[0]] * 33)]
    for count in (0, 33):
        assert lib.apk_kzg_batch_verify_multi(C.byref(m.vk), -1, count, *big_args) == ERR_ARG
    assert lib.apk_kzg_batch_verify_multi(C.byref(m.vk), -1, 32, *[a[:len(a) // 33 * 32] for a in big_args]) == OK      # the same opening 32 times


@pytest.mark.parametrize("cname", NAMES)
def test_a_batch_of_one_is_the_single_call(cname):
    m = material(cname)
    cv, r = m.cv, m.cv.r
    for i in (0, 3, 5):      # (3: the constant, H = infinity)
        d, z, v, h = m.digests[i], m.points[i], m.values[i], m.hs[i]
        for dd, zz, vv, hh in ((d, z, v, h), (d, z, (v + 1) % r, h), (m.other, z, v, h), (d, (z + 1) % r, v, h), (d, z, v, m.other)):
            want = km.verify(cv, m.vk, dd, zz, vv, hh)
            assert multi_verify(cv, m.vk, [dd], [zz], [vv], [hh]) == want
        assert km.verify(cv, m.vk, d, z, v, h) == OK


def test_python_mirror_of_the_verifier():
    m = material("bn254")
    cv, r = m.cv, m.cv.r
    vk = ap_kzg.VerifyingKey(cv, cv.g1, m.g2)
    d, z, v, h = m.batch(5)
    proofs = [ap_kzg.OpeningProof(H, val) for H, val in zip(h, v)]
    ap_kzg.BatchVerifyMultiPoints(d, proofs, z, vk)
    proofs[3] = ap_kzg.OpeningProof(h[3], (v[3] + 1) % r)
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.BatchVerifyMultiPoints(d, proofs, z, vk)
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.BatchVerifyMultiPoints(d, proofs[:4], z, vk)


# ---- the opening call without a context: the order of the checks ---------------------------------------------------------------
def _multi_args(cv, count=2, n=4):
    bufs = [C.create_string_buffer(cv.fr_vector([1] * n), 32 * n) for _ in range(max(count, 1))]
    ptrs = (C.c_void_p * len(bufs))(*[C.addressof(b) for b in bufs])
    lens = (C.c_uint64 * len(bufs))(*[n] * len(bufs))
    return bufs, ptrs, lens, cv.fr_vector([2] * len(bufs)), C.create_string_buffer(96 * len(bufs)), C.create_string_buffer(32 * len(bufs))


@pytest.mark.parametrize("cname", NAMES)
def test_open_multi_checks_arguments_then_the_device_then_the_context(cname):
    cv, _ = CURVES[cname]
    bufs, ptrs, lens, zs, h, vals = _multi_args(cv, 33)
    for fn in (lib.apk_kzg_open_multi, lib.apk_kzg_open_multi_device):
        assert fn(None, 0, ptrs, lens, zs, h, vals) == ERR_ARG
        assert fn(None, 33, ptrs, lens, zs, h, vals) == ERR_ARG
        assert fn(None, 2, None, lens, zs, h, vals) == ERR_ARG
        assert fn(None, 2, ptrs, None, zs, h, vals) == ERR_ARG
        assert fn(None, 2, ptrs, lens, None, h, vals) == ERR_ARG
        assert fn(None, 2, ptrs, lens, zs, None, vals) == ERR_ARG
        assert fn(None, 2, ptrs, lens, zs, h, None) == ERR_ARG
        assert fn(None, 2, ptrs, (C.c_uint64 * 2)(4, 0), zs, h, vals) == ERR_ARG          # a polynomial without coefficients
        assert fn(None, 2, ptrs, (C.c_uint64 * 2)(4, 1 << 40), zs, h, vals) == ERR_ARG    # no SRS is that long
        assert fn(None, 2, (C.c_void_p * 2)(ptrs[0], None), lens, zs, h, vals) == ERR_ARG
        # everything but the context in order: the device is missed first where there is none
        want = ERR_HIP if _lib.device_count() == 0 else ERR_ARG
        assert fn(None, 2, ptrs, lens, zs, h, vals) == want
        if want == ERR_HIP:
            assert b"no CPU fallback" in lib.apk_last_error()


# ---- the new exports record the library's first HIP call (runtime_env.h) -------------------------------------------------------
NEED = 16
_WALK = {
    "apk_kzg_open_multi": "lib.apk_kzg_open_multi(None, 1, (C.c_void_p * 1)(C.addressof(z)), (C.c_uint64 * 1)(1), z, o, o)",
    "apk_kzg_open_multi_device": "lib.apk_kzg_open_multi_device(None, 1, (C.c_void_p * 1)(C.addressof(z)), (C.c_uint64 * 1)(1), z, o, o)",
    "apk_kzg_batch_verify_multi": "lib.apk_kzg_batch_verify_multi(C.byref(_lib.KzgVk()), 0, 1, z, z, z, z)",
}
_WALK_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from algoplonk_amd import _lib
from algoplonk_amd._lib import lib
z, o = C.create_string_buffer(4096), C.create_string_buffer(4096)
before = _lib.runtime()["first_hip_call"]
%s
print("RESULT " + json.dumps({"before": before, "after": _lib.runtime()}))
"""


@pytest.mark.parametrize("export", sorted(_WALK))
def test_the_new_exports_record_the_first_hip_call(export):
    e = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    e.pop("APK_HW_QUEUES", None)
    r = subprocess.run([sys.executable, "-c", _WALK_CHILD % (ROOT, _WALK[export])], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert got["before"] == -1, got
    assert got["after"]["first_hip_call"] == 1 and got["after"]["hw_queues_at_first_hip"] == NEED, (export, got)


def test_the_host_fold_makes_no_hip_call():
    code = _WALK_CHILD % (ROOT, "lib.apk_kzg_batch_verify_multi(C.byref(_lib.KzgVk()), -1, 1, z, z, z, z); lib.apk_kzg_multi_weights(C.byref(_lib.KzgVk()), 1, z, z, z, z, o)")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert got["before"] == -1 and got["after"]["first_hip_call"] == -1, got


# ---- the rule stand-alone under ASAN + UBSAN ------------------------------------------------------------------------------------
def _line(m, expect, digests, points, values, hs, g2=None, raw_values=None):
    cv = m.cv
    return " ".join([str(cv.abi), str(expect), cv.g1_to_bytes(cv.g1).hex(), (g2 or m.g2).hex(), str(len(digests)),
                     cv.g1_vector(digests).hex(), cv.fr_vector(points).hex(), (raw_values or cv.fr_vector(values)).hex(), cv.g1_vector(hs).hex()])


def test_multi_point_rule_under_address_and_undefined_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "san-kzg-multi"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines, weights = [], []
    for cname in NAMES:
        m = material(cname)
        cv, ov, rr = m.cv, m.ov, m.cv.r
        for n in (1, 3, 17):
            d, z, v, h = m.batch(n)
            lines.append(_line(m, 1, d, z, v, h)); weights.append(model_weights(cv, ov, m.g2, d, z, v, h))
            bumped = list(v); bumped[n - 1] = (bumped[n - 1] + 1) % rr
            lines.append(_line(m, 0, d, z, bumped, h)); weights.append(model_weights(cv, ov, m.g2, d, z, bumped, h))
        d, z, v, h = m.batch(2)
        bad = [(v[0] + 99) % rr, (v[1] - 99) % rr]
        lines.append(_line(m, 0, d, z, bad, h)); weights.append(model_weights(cv, ov, m.g2, d, z, bad, h))      # errors that cancel
        off = (h[1][0], (h[1][1] + 1) % cv.p)
        lines.append(_line(m, 0, d, z, v, [h[0], off])); weights.append(None)                                    # H off the curve
        lines.append(_line(m, 3, d, z, v, h, raw_values=cv.fr_vector([v[0]]) + rr.to_bytes(32, "little"))); weights.append(None)
        g2 = bytearray(m.g2); g2[0] ^= 1
        lines.append(_line(m, 2, d, z, v, h, g2=bytes(g2))); weights.append(None)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "san", "kzg_multi_check"), str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "KZG MULTI CHECK OK: %d cases" % len(lines) in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = [l for l in r.stdout.splitlines() if l.startswith("case ")]
    assert len(out) == len(lines)
    for i, (l, want) in enumerate(zip(out, weights)):
        if want is None:
            continue
        cv = CURVES[NAMES[int(lines[i].split()[0])]][0]
        assert cv.fr_vector_decode(bytes.fromhex(l.split(" weights ")[1])) == want, i

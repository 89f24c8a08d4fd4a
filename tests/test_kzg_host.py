"""CPU tier: the host half of the KZG primitives (include/apk.h apk_kzg_verify, apk_kzg_batch_verify, apk_kzg_fold_challenge;
csrc/kzg_protocol.h) against the big-integer model of tests/kzg_model.py, the argument and no-device errors of the four opening
calls, the fold challenge against the executed reference template, and kzg_protocol.h once more stand-alone under ASAN + UBSAN."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess

import pytest

import kzg_model as km
from algoplonk_amd import _lib, setup as ap_setup
from algoplonk_amd._lib import lib
from helpers import CURVES
from oracle import curves as ocurves
from oracle.prng import SplitMix64, tau_from_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
NAMES = ["bn254", "bls12-381"]
OK, ERR_ARG, ERR_HIP, ERR_VERIFY = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_HIP, _lib.APK_ERR_VERIFY


class Material:
    """One single opening and one batch opening per curve, made by the model."""

    def __init__(self, cname: str):
        self.cv, self.ov = CURVES[cname]
        cv, ov = self.cv, self.ov
        r = cv.r
        g = SplitMix64(0x4B5A47 + cv.abi)
        self.tau = tau_from_seed(0x4B5A, r)
        self.g2 = ap_setup.g2_from_tau(cv, self.tau)
        self.vk = km.kzg_vk(cv, self.g2)
        self.z = g.fr(r)
        self.f = km.polynomial("random", 7, r, g)
        self.digest = km.commit(ov, self.f, self.tau)
        self.H, self.v = km.open_at(ov, self.f, self.z, self.tau)
        self.other = ov.mul(ov.g1, g.fr(r))
        self.polys = [km.polynomial("random", 5, r, g), km.polynomial("random", 1, r, g), km.polynomial("top", 9, r, g)]
        self.extra = bytes(g.below(256) for _ in range(100))
        self.digests, self.values, self.gamma, self.bH = km.batch_open_at(ov, self.polys, self.z, self.tau, self.extra)


_MAT = {}


def material(cname: str) -> Material:
    if cname not in _MAT:
        _MAT[cname] = Material(cname)
    return _MAT[cname]


@pytest.mark.parametrize("cname", NAMES)
def test_single_opening_accepted_and_every_mutation_rejected(cname):
    m = material(cname)
    cv, r = m.cv, m.cv.r
    assert km.verify(cv, m.vk, m.digest, m.z, m.v, m.H) == OK, lib.apk_last_error()
    assert km.verify(cv, m.vk, m.digest, m.z, (m.v + 1) % r, m.H) == ERR_VERIFY
    assert km.verify(cv, m.vk, m.digest, m.z, m.v, m.other) == ERR_VERIFY
    assert km.verify(cv, m.vk, m.other, m.z, m.v, m.H) == ERR_VERIFY
    assert km.verify(cv, m.vk, m.digest, (m.z + 1) % r, m.v, m.H) == ERR_VERIFY


@pytest.mark.parametrize("cname", NAMES)
def test_batch_opening_accepted_and_every_mutation_rejected(cname):
    m = material(cname)
    cv, r = m.cv, m.cv.r
    assert km.batch_verify(cv, m.vk, m.digests, m.values, m.z, m.extra, m.bH) == OK, lib.apk_last_error()
    bumped = [m.values[0], (m.values[1] + 1) % r, m.values[2]]
    assert km.batch_verify(cv, m.vk, m.digests, bumped, m.z, m.extra, m.bH) == ERR_VERIFY
    assert km.batch_verify(cv, m.vk, m.digests, m.values, m.z, m.extra, m.other) == ERR_VERIFY
    swapped = [m.digests[1], m.digests[0], m.digests[2]]
    assert km.batch_verify(cv, m.vk, swapped, m.values, m.z, m.extra, m.bH) == ERR_VERIFY
    assert km.batch_verify(cv, m.vk, m.digests, m.values, (m.z + 1) % r, m.extra, m.bH) == ERR_VERIFY
    flipped = bytes([m.extra[0] ^ 1]) + m.extra[1:]
    assert km.batch_verify(cv, m.vk, m.digests, m.values, m.z, flipped, m.bH) == ERR_VERIFY
    # no data transcript: another challenge, another H
    d2, v2, g2, h2 = km.batch_open_at(m.ov, m.polys, m.z, m.tau, b"")
    assert g2 != m.gamma and km.batch_verify(cv, m.vk, d2, v2, m.z, b"", h2) == OK
    # a batch of one is the single opening under gamma^0
    assert km.batch_verify(cv, m.vk, [m.digest], [m.v], m.z, b"", m.H) == OK


@pytest.mark.parametrize("cname", NAMES)
def test_fold_challenge_is_the_models_hash(cname):
    m = material(cname)
    cv = m.cv
    out = C.create_string_buffer(32)
    for extra in (m.extra, b""):
        assert lib.apk_kzg_fold_challenge(cv.abi, 3, cv.g1_vector(m.digests), cv.fr_vector(m.values), cv.fr_vector([m.z]),
                                          extra or None, len(extra), out) == OK
        assert cv.fr_from_mont_bytes(out.raw) == km.fold_challenge(m.ov, m.z, m.digests, m.values, extra)
    # infinity among the digests: both infinity encodings of the transcript (0x40 00.. on BLS12-381, zeros on BN254)
    digs = [None, m.digests[1], m.digests[2]]
    assert lib.apk_kzg_fold_challenge(cv.abi, 3, cv.g1_vector(digs), cv.fr_vector(m.values), cv.fr_vector([m.z]), None, 0, out) == OK
    assert cv.fr_from_mont_bytes(out.raw) == km.fold_challenge(m.ov, m.z, digs, m.values)


@pytest.mark.parametrize("cname", NAMES)
def test_zero_polynomial_is_accepted(cname):
    m = material(cname)
    assert km.verify(m.cv, m.vk, None, m.z, 0, None) == OK, lib.apk_last_error()
    assert km.verify(m.cv, m.vk, None, m.z, 1, None) == ERR_VERIFY
    assert km.batch_verify(m.cv, m.vk, [None, None], [0, 0], m.z, b"", None) == OK


def _raw_verify(m, digest_bytes, h_bytes):
    cv = m.cv
    return lib.apk_kzg_verify(C.byref(m.vk), digest_bytes, cv.fr_vector([m.z]), cv.fr_vector([m.v]), h_bytes)


@pytest.mark.parametrize("cname", NAMES)
def test_points_off_the_curve_are_rejected(cname):
    m = material(cname)
    cv = m.cv
    off = (m.H[0], (m.H[1] + 1) % cv.p)
    assert not m.ov.is_on_curve(off)
    assert _raw_verify(m, cv.g1_to_bytes(m.digest), cv.g1_to_bytes(off)) == ERR_VERIFY
    assert _raw_verify(m, cv.g1_to_bytes(off), cv.g1_to_bytes(m.H)) == ERR_VERIFY
    # coordinates that are not below p
    big = (cv.p).to_bytes(cv.fp_bytes, "little") + cv.g1_to_bytes(m.H)[cv.fp_bytes:]
    assert _raw_verify(m, cv.g1_to_bytes(m.digest), big) == ERR_VERIFY


def test_bls12_381_point_outside_the_subgroup_is_rejected():
    m = material("bls12-381")
    cv, ov = m.cv, m.ov
    x = 1
    while True:      # the first x with a point on the curve: with a cofactor of ~2^126 such a point is outside the subgroup
        x += 1
        y = ocurves.sqrt_mod((x ** 3 + 4) % cv.p, cv.p)
        if y is not None and ov.add(ov.mul((x, y), cv.r - 1), (x, y)) is not None:      # [r]P != infinity
            break
    P = (x, y)
    assert ov.is_on_curve(P)
    assert _raw_verify(m, cv.g1_to_bytes(m.digest), cv.g1_to_bytes(P)) == ERR_VERIFY
    assert b"opening does not verify" in lib.apk_last_error()
    assert _raw_verify(m, cv.g1_to_bytes(P), cv.g1_to_bytes(m.H)) == ERR_VERIFY


@pytest.mark.parametrize("cname", NAMES)
def test_bad_keys_scalars_and_counts_are_argument_errors(cname):
    m = material(cname)
    cv = m.cv
    assert lib.apk_kzg_verify(None, cv.g1_to_bytes(m.digest), cv.fr_vector([m.z]), cv.fr_vector([m.v]), cv.g1_to_bytes(m.H)) == ERR_ARG
    assert lib.apk_kzg_verify(C.byref(m.vk), None, cv.fr_vector([m.z]), cv.fr_vector([m.v]), cv.g1_to_bytes(m.H)) == ERR_ARG
    # a value that is not below r
    assert lib.apk_kzg_verify(C.byref(m.vk), cv.g1_to_bytes(m.digest), cv.fr_vector([m.z]), cv.r.to_bytes(32, "little"), cv.g1_to_bytes(m.H)) == ERR_ARG
    # G2 points swapped for garbage / G1 at infinity
    bad = km.kzg_vk(cv, m.g2)
    bad.g2[1][0] ^= 1
    assert km.verify(cv, bad, m.digest, m.z, m.v, m.H) == ERR_ARG
    bad = km.kzg_vk(cv, m.g2)
    C.memset(bad.g1, 0, _lib.G1_MAX)
    assert km.verify(cv, bad, m.digest, m.z, m.v, m.H) == ERR_ARG
    bad = km.kzg_vk(cv, m.g2)
    bad.curve = 7
    assert km.verify(cv, bad, m.digest, m.z, m.v, m.H) == ERR_ARG
    for count in (0, 33):
        assert lib.apk_kzg_batch_verify(C.byref(m.vk), count, cv.g1_vector([m.digest] * 33), cv.fr_vector([m.v] * 33), cv.fr_vector([m.z]),
                                        None, 0, cv.g1_to_bytes(m.H)) == ERR_ARG


# ---- the fold challenge against the executed reference template ------------------------------------------------------------------
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "template_verdicts.json")))
VALID = [(c, r) for c in FIX["cases"] for r in c["results"] if r["mutation"] == "valid"]


def _pt(j):
    return None if j is None else (int(j[0], 16), int(j[1], 16))


@pytest.mark.parametrize("case,res", VALID, ids=["%s-%s" % (c["curve"], c["circuit"]) for c, _ in VALID])
def test_fold_challenge_in_the_plonk_arrangement_is_the_templates(case, res):
    """digests [lin] [L] [R] [O] [S1] [S2] [Qcp_i], their claimed values, extra = Z(omega zeta): the challenge must be the folding
    challenge the reference's verifier template derived when it was executed (the proof's layout: helper.go:27-88)."""
    cv, ov = CURVES[case["curve"]]
    vk, want = case["vk"], res["intermediates"]
    k = len(vk["qcp"])
    blob = bytes.fromhex(res["proof"])
    w = 2 * cv.fp_bytes

    def pt(off):
        return ov.from_raw_bytes(blob[off:off + w])

    def fr(off):
        return int.from_bytes(blob[off:off + 32], "big")

    s0 = 6 * w
    tail = s0 + 192 + 3 * w
    lin = ov.from_raw_bytes(bytes.fromhex(want["lin_poly_com"]))
    digests = [lin, pt(0), pt(w), pt(2 * w), _pt(vk["s"][0]), _pt(vk["s"][1])] + [_pt(q) for q in vk["qcp"]]
    values = [int(want["linearized_poly_at_z"], 16)] + [fr(s0 + 32 * i) for i in range(5)] + [fr(tail + 32 * i) for i in range(k)]
    extra = blob[s0 + 160 + w: s0 + 192 + w]
    out = C.create_string_buffer(32)
    assert lib.apk_kzg_fold_challenge(cv.abi, len(digests), cv.g1_vector(digests), cv.fr_vector(values), cv.fr_vector([int(want["zeta"], 16)]),
                                      extra, 32, out) == OK, lib.apk_last_error()
    assert hex(cv.fr_from_mont_bytes(out.raw)) == want["gamma_kzg"]


# ---- the opening calls without a context ------------------------------------------------------------------------------------------
def _open_args(cv, n=4):
    return (cv.fr_vector([1] * n), n, cv.fr_vector([2]), C.create_string_buffer(96), C.create_string_buffer(32))


def _batch_args(cv, count=2, n=4):
    bufs = [C.create_string_buffer(cv.fr_vector([1] * n), 32 * n) for _ in range(max(count, 1))]
    ptrs = (C.c_void_p * len(bufs))(*[C.addressof(b) for b in bufs])
    lens = (C.c_uint64 * len(bufs))(*[n] * len(bufs))
    return bufs, ptrs, lens, C.create_string_buffer(96), C.create_string_buffer(32 * len(bufs)), C.create_string_buffer(32)


@pytest.mark.parametrize("cname", NAMES)
def test_open_calls_need_a_device_and_a_context(cname):
    """Arguments other than the context are checked first; then the device (no CPU fallback: APK_ERR_HIP without one); then the
    context.  With a GPU in the box a null context is therefore an argument error, without one the device is missed first."""
    cv, _ = CURVES[cname]
    want = ERR_HIP if _lib.device_count() == 0 else ERR_ARG
    poly, n, z, h, v = _open_args(cv)
    assert lib.apk_kzg_open(None, poly, n, z, h, v) == want
    assert lib.apk_kzg_open_device(None, poly, n, z, h, v) == want
    bufs, ptrs, lens, bh, vals, gamma = _batch_args(cv)
    assert lib.apk_kzg_batch_open(None, 2, ptrs, lens, None, z, None, 0, bh, vals, gamma) == want
    assert lib.apk_kzg_batch_open_device(None, 2, ptrs, lens, None, z, None, 0, bh, vals, None) == want
    if want == ERR_HIP:
        assert b"no CPU fallback" in lib.apk_last_error()


@pytest.mark.parametrize("cname", NAMES)
def test_open_calls_argument_errors(cname):
    cv, _ = CURVES[cname]
    poly, n, z, h, v = _open_args(cv)
    for fn in (lib.apk_kzg_open, lib.apk_kzg_open_device):
        assert fn(None, poly, 0, z, h, v) == ERR_ARG                 # len == 0
        assert fn(None, poly, 1 << 40, z, h, v) == ERR_ARG           # no SRS is that long
        assert fn(None, None, n, z, h, v) == ERR_ARG
        assert fn(None, poly, n, None, h, v) == ERR_ARG
        assert fn(None, poly, n, z, None, v) == ERR_ARG
        assert fn(None, poly, n, z, h, None) == ERR_ARG
    bufs, ptrs, lens, bh, vals, gamma = _batch_args(cv, 33)
    for fn in (lib.apk_kzg_batch_open, lib.apk_kzg_batch_open_device):
        assert fn(None, 0, ptrs, lens, None, z, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 33, ptrs, lens, None, z, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 2, None, lens, None, z, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 2, ptrs, None, None, z, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 2, ptrs, lens, None, None, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 2, ptrs, lens, None, z, None, 5, bh, vals, gamma) == ERR_ARG     # extra_len without extra
        assert fn(None, 2, ptrs, lens, None, z, None, 0, None, vals, gamma) == ERR_ARG
        assert fn(None, 2, ptrs, lens, None, z, None, 0, bh, None, gamma) == ERR_ARG
        zero = (C.c_uint64 * 2)(4, 0)
        assert fn(None, 2, ptrs, zero, None, z, None, 0, bh, vals, gamma) == ERR_ARG     # a polynomial without coefficients
        holes = (C.c_void_p * 2)(ptrs[0], None)
        assert fn(None, 2, holes, lens, None, z, None, 0, bh, vals, gamma) == ERR_ARG


def test_kzg_shape_is_exported():
    a, b = C.c_int(0), C.c_int(0)
    assert lib.apk_kzg_shape(C.byref(a), C.byref(b)) == OK
    assert a.value >= 1 and b.value % a.value == 0 and b.value // a.value in (64, 128, 256, 512, 1024)
    assert lib.apk_kzg_shape(None, C.byref(b)) == ERR_ARG


# ---- kzg_protocol.h stand-alone under ASAN + UBSAN --------------------------------------------------------------------------------
def _line(m, batch, expect, digests, values, z, extra, H, g2=None):
    cv = m.cv
    return " ".join([str(cv.abi), str(int(batch)), str(expect), cv.g1_to_bytes(cv.g1).hex(), (g2 or m.g2).hex(), str(len(digests)),
                     cv.g1_vector(digests).hex(), cv.fr_vector(values).hex(), cv.fr_vector([z]).hex(), extra.hex() or "-", cv.g1_to_bytes(H).hex()])


def test_kzg_protocol_under_address_and_undefined_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "san-kzg"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = []
    for cname in NAMES:
        m = material(cname)
        rr = m.cv.r
        lines += [
            _line(m, 0, 1, [m.digest], [m.v], m.z, b"", m.H),
            _line(m, 0, 0, [m.digest], [(m.v + 1) % rr], m.z, b"", m.H),
            _line(m, 0, 0, [m.digest], [m.v], m.z, b"", (m.H[0], (m.H[1] + 1) % m.cv.p)),
            _line(m, 0, 1, [None], [0], m.z, b"", None),
            _line(m, 1, 1, m.digests, m.values, m.z, m.extra, m.bH),
            _line(m, 1, 0, m.digests, m.values, m.z, m.extra[:-1], m.bH),
            _line(m, 1, 0, m.digests, m.values, m.z, m.extra, m.other),
            _line(m, 0, 2, [m.digest], [m.v], m.z, b"", m.H, g2=m.g2[:-1] + bytes([m.g2[-1] ^ 1])),
        ]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "san", "kzg_check"), str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "KZG CHECK OK: %d cases" % len(lines) in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]

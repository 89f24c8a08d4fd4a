"""CPU tier of the openings on every coset of the domain (include/apk.h apk_kzg_cosets_prepare, apk_kzg_open_cosets*,
apk_kzg_verify_coset): the identities the kernels run, restated in the exponent with a known tau (tests/kzg_cosets_model.py) and held
to each other; apk_kzg_verify_coset on proofs the model makes; the host interpolation and check stand-alone under ASAN + UBSAN;
the exports; the argument errors that come before the device check; the Python wrapper's argument errors."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import pytest

import kzg_all_model as kam
import kzg_cosets_model as kcm
import kzg_model as km
from algoplonk_amd import _lib, kzg as ap_kzg, setup as ap_setup
from algoplonk_amd._lib import lib
from helpers import CURVES
from oracle.prng import SplitMix64, tau_from_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
NAMES = ["bn254", "bls12-381"]
OK, ERR_ARG, ERR_HIP, ERR_VERIFY = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_HIP, _lib.APK_ERR_VERIFY
NEW = ["apk_kzg_cosets_prepare", "apk_kzg_open_cosets", "apk_kzg_open_cosets_device", "apk_kzg_verify_coset"]
GPU_SHAPES = [(8, 2), (8, 4), (128, 2), (128, 8), (128, 64), (512, 16), (512, 64), (2048, 64)]      # tests/test_gpu_kzg_cosets.py


def lengths(n, l):
    return sorted({1, l, l + 1, 2 * l, n // 2 + 1, n - 1, n})


def _sizes(n):
    l = 2
    while l <= n // 2:
        yield l
        l *= 2


# ---- the identities ---------------------------------------------------------------------------------------------------------------------
def _hold(cname, n, l, L, seed, compose=True):
    cv, _ = CURVES[cname]
    r = cv.r
    g = SplitMix64(seed + cv.abi)
    tau = tau_from_seed(0xC05 + n + l, r)
    w, w_2n = cv.omega(n), cv.omega(2 * n)
    f = [g.fr(r) for _ in range(L)]
    want = kcm.direct(f, n, l, w, tau, r)                                                 # (1)
    what = (cname, n, l, L)
    assert kcm.by_transform(f, n, l, w, tau, r) == want, what                             # (2)
    assert kcm.arrangement(f, n, l, w_2n, tau, r) == want, what                           # (3)
    if L <= l:
        assert want == [0] * (n // l), what
    for c in sorted({0, 1, l - 1}):                                                       # (4)
        a, _ = kcm.sequences(f, n, l, c, tau, r)
        a_hat = kam.dft(a, pow(w_2n, l, r), r)
        even, odd = kcm.a_hat_split(f, n, l, c, w_2n, r)
        assert a_hat[0::2] == even and a_hat[1::2] == odd, what
    if compose:
        assert kcm.composition(f, n, l, w, tau, r) == want, what                          # (5)
    # (6) on one coset: the interpolant is the remainder, and the check accepts exactly the right proof
    i = (n // l) - 1
    vals = kcm.values_by_coset(f, n, l, w, r)[i * l:(i + 1) * l]
    assert vals == [kam.horner(f, x, r) for x in kcm.coset_points(n, l, i, w, r)]
    assert kcm.interpolate(vals, n, l, i, w, r) == kcm.remainder(f, n, l, pow(w, i * l, r), r), what
    ft = kam.horner(f, tau, r)
    assert kcm.accepts(ft, vals, want[i], n, l, i, w, tau, r)
    assert not kcm.accepts(ft, vals, (want[i] + 1) % r, n, l, i, w, tau, r)


@pytest.mark.parametrize("n", [8, 16, 64])
@pytest.mark.parametrize("cname", NAMES)
def test_the_identities_at_every_coset_size(cname, n):
    for l in _sizes(n):
        for L in lengths(n, l):
            _hold(cname, n, l, L, 0xC010 + n + l)


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cname", NAMES)
def test_the_identities_at_the_shapes_of_the_gpu_tier(cname, shape):
    n, l = shape
    for L in lengths(n, l):
        # (the composition over n single-point openings costs n^2 products: once per shape at the larger ones)
        _hold(cname, n, l, L, 0xC020 + n + l, compose=n <= 128 or L == n)


@pytest.mark.parametrize("cname", NAMES)
def test_structured_polynomials_of_the_gpu_tier(cname):
    """What tests/test_gpu_kzg_cosets.py says of its structured inputs, at n = 16, l = 4 (and l = 2 for the meeting terms)"""
    cv, _ = CURVES[cname]
    r, n, l = cv.r, 16, 4
    tau = tau_from_seed(0xC03, r)
    w, w_2n = cv.omega(n), cv.omega(2 * n)
    g = SplitMix64(0xC030 + cv.abi)
    np = n // l
    assert kcm.direct([0] * n, n, l, w, tau, r) == [0] * np
    assert kcm.direct([g.fr(r) for _ in range(l)] + [0] * (n // 2), n, l, w, tau, r) == [0] * np
    assert kcm.direct([0] * l + [1], n, l, w, tau, r) == [1] * np                            # X^l: every H = s_0
    top = [0] * (n - 1) + [1]
    assert kcm.h_terms(top, n, l, tau, r) == [pow(tau, n - 1 - l * (m + 1), r) for m in range(np - 1)] + [0]
    for i in (0, 2):
        vanishing = [(-pow(w, i * l, r)) % r] + [0] * (l - 1) + [1]
        assert kcm.values_by_coset(vanishing, n, l, w, r)[i * l:(i + 1) * l] == [0] * l
        assert kcm.direct(vanishing, n, l, w, tau, r) == [1] * np
    f = [0 if k % l == 1 else g.fr(r) for k in range(n)]
    a, _ = kcm.sequences(f, n, l, 1, tau, r)
    assert a == [0] * (2 * np) and kcm.arrangement(f, n, l, w_2n, tau, r) == kcm.direct(f, n, l, w, tau, r)
    for opposite in (False, True):
        f, i_star = meeting_terms(cv, 16, tau, g, opposite)
        t0, t1 = kcm.t_hat(16, 2, 0, w_2n, tau, r), kcm.t_hat(16, 2, 1, w_2n, tau, r)
        a0 = kam.dft(kcm.sequences(f, 16, 2, 0, tau, r)[0], pow(w_2n, 2, r), r)
        a1 = kam.dft(kcm.sequences(f, 16, 2, 1, tau, r)[0], pow(w_2n, 2, r), r)
        x, y = a0[i_star] * t0[i_star] % r, a1[i_star] * t1[i_star] % r
        assert x != 0 and y == ((-x) % r if opposite else x)
        assert kcm.arrangement(f, 16, 2, w_2n, tau, r) == kcm.direct(f, 16, 2, w, tau, r)


def meeting_terms(cv, n, tau, g, opposite, i_star=3):
    """l = 2: f = (.., f_2 = alpha, f_3 = +-alpha T^_0[i*] / T^_1[i*]) and nothing above, so that a_0 = (alpha, 0 ..) and
    a_1 = (f_3, 0 ..) have constant transforms and the two terms of output i* are equal (opposite).  (f, i*)"""
    r = cv.r
    w_2n = cv.omega(2 * n)
    t0, t1 = kcm.t_hat(n, 2, 0, w_2n, tau, r)[i_star], kcm.t_hat(n, 2, 1, w_2n, tau, r)[i_star]
    assert t0 and t1
    alpha = g.fr(r) or 1
    f3 = alpha * t0 % r * pow(t1, -1, r) % r
    return [g.fr(r), g.fr(r), alpha, (-f3) % r if opposite else f3], i_star


# ---- apk_kzg_verify_coset on the model's proofs ----------------------------------------------------------------------------------------
class Made:
    """A polynomial, its commitment and every coset proof, by the model; the key and [tau^l]G2 by apk_g2_mul_generator"""

    def __init__(self, cname, n, l, seed=0xC040):
        self.cv, self.ov = CURVES[cname]
        cv, ov, r = self.cv, self.ov, self.cv.r
        self.n, self.l, self.np = n, l, n // l
        g = SplitMix64(seed + cv.abi + n + l)
        self.tau = tau_from_seed(seed + n + l, r)
        self.w = cv.omega(n)
        self.f = [g.fr(r) for _ in range(n)]
        self.other = [g.fr(r) for _ in range(n)]
        self.g2 = ap_setup.g2_from_tau(cv, self.tau)
        self.vk = km.kzg_vk(cv, self.g2)
        self.srs = b"".join(cv.g1_to_bytes(ov.mul(ov.g1, pow(self.tau, c, r))) for c in range(l))
        self.digest = cv.g1_to_bytes(km.commit(ov, self.f, self.tau))
        hs = kcm.direct(self.f, n, l, self.w, self.tau, r)
        self.h = [cv.g1_to_bytes(ov.mul(ov.g1, k) if k else None) for k in hs]
        self.values = kcm.values_by_coset(self.f, n, l, self.w, r)

    def tau_pow_g2(self, e):
        w = 4 * self.cv.fp_bytes
        return ap_setup.g2_from_tau(self.cv, pow(self.tau, e, self.cv.r))[w:2 * w]

    def vals(self, i):
        return self.values[i * self.l:(i + 1) * self.l]

    def verify(self, i, values=None, h=None, digest=None, g2=None, index=None, vk=None, n=None, l=None, srs=None):
        cv = self.cv
        return lib.apk_kzg_verify_coset(C.byref(vk or self.vk), g2 or self.tau_pow_g2(self.l), srs or self.srs, self.n if n is None else n,
                                        self.l if l is None else l, i if index is None else index, digest or self.digest,
                                        cv.fr_vector(values or self.vals(i)), h or self.h[i])


_MADE = {}


def made(cname, n, l) -> Made:
    if (cname, n, l) not in _MADE:
        _MADE[(cname, n, l)] = Made(cname, n, l)
    return _MADE[(cname, n, l)]


@pytest.mark.parametrize("shape", [(8, 2), (8, 4), (64, 8)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cname", NAMES)
def test_verify_coset_accepts_every_index_and_rejects_what_is_wrong(cname, shape):
    m = made(cname, *shape)
    cv, ov, r, np = m.cv, m.ov, m.cv.r, m.np
    for i in range(np):
        assert m.verify(i) == OK, (i, lib.apk_last_error())
    i = np - 1
    bad = list(m.vals(i))
    bad[m.l - 1] = (bad[m.l - 1] + 1) % r
    assert m.verify(i, values=bad) == ERR_VERIFY                                    # one value changed
    assert lib.apk_last_error()
    assert m.verify(i, index=i - 1) == ERR_VERIFY                                   # the index off by one
    if np > 2:
        assert m.verify(i, h=m.h[i - 1]) == ERR_VERIFY                              # H of the neighbouring coset
    else:
        # n' = 2: H_i = sum_{m <= n'-2} (w^l)^(i m) h_m = h_0 for both cosets - the neighbour's H is this coset's own proof
        assert m.h[0] == m.h[1] and m.verify(i, h=m.h[i - 1]) == OK
    assert m.verify(i, digest=cv.g1_to_bytes(km.commit(ov, m.other, m.tau))) == ERR_VERIFY
    assert m.verify(i, g2=m.tau_pow_g2(m.l // 2)) == ERR_VERIFY                     # [tau^(l/2)]G2
    # a polynomial below degree l: its own remainder, H = infinity
    short = m.f[:m.l]
    vals = kcm.values_by_coset(short, m.n, m.l, m.w, r)[:m.l]
    d = cv.g1_to_bytes(km.commit(ov, short, m.tau))
    assert m.verify(0, values=vals, h=cv.g1_to_bytes(None), digest=d) == OK, lib.apk_last_error()
    assert m.verify(0, values=vals, h=m.h[0], digest=d) == ERR_VERIFY


@pytest.mark.parametrize("cname", NAMES)
def test_verify_coset_argument_errors(cname):
    m = made(cname, 8, 2)
    cv, r = m.cv, m.cv.r
    assert m.verify(0) == OK
    for kw in (dict(n=0), dict(n=12), dict(n=2), dict(l=0), dict(l=1), dict(l=3), dict(l=8), dict(n=1 << 40), dict(index=4), dict(index=1 << 63)):
        assert m.verify(0, **kw) == ERR_ARG, kw
        assert lib.apk_last_error(), kw
    good = (C.byref(m.vk), m.tau_pow_g2(2), m.srs, 8, 2, 0, m.digest, cv.fr_vector(m.vals(0)), m.h[0])
    assert lib.apk_kzg_verify_coset(*good) == OK
    for k in (0, 1, 2, 6, 7, 8):
        args = list(good)
        args[k] = None
        assert lib.apk_kzg_verify_coset(*args) == ERR_ARG, k
    # a scalar that is not below r; a bad key; a G2 point off the twist
    raw = bytearray(cv.fr_vector(m.vals(0)))
    raw[0:32] = b"\xff" * 32
    assert lib.apk_kzg_verify_coset(*good[:7], bytes(raw), good[8]) == ERR_ARG
    bad = km.kzg_vk(cv, m.g2)
    bad.g2[1][0] ^= 1
    assert m.verify(0, vk=bad) == ERR_ARG
    off = bytearray(m.tau_pow_g2(2))
    off[0] ^= 1
    assert m.verify(0, g2=bytes(off)) == ERR_ARG
    unknown = km.kzg_vk(cv, m.g2)
    unknown.curve = 7
    assert m.verify(0, vk=unknown) == ERR_ARG
    assert m.verify(0) == OK


# ---- the host interpolation and check, stand-alone under ASAN + UBSAN --------------------------------------------------------------
def test_coset_check_under_address_and_undefined_sanitizers():
    r = subprocess.run(["make", "-C", CSRC, "san-kzg-cosets"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "san", "kzg_cosets_check")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "KZG COSETS CHECK OK" in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    # the interpolants it printed, held to the model:  I <curve> <n> <l> <index> : <l values> : <l coefficients>
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("I ")]
    assert len(lines) >= 8
    for t in lines:
        abi, n, l, i = (int(x) for x in t[1:5])
        cv = [CURVES[c][0] for c in NAMES if CURVES[c][0].abi == abi][0]
        vals, co = [int(x, 16) for x in t[6:6 + l]], [int(x, 16) for x in t[7 + l:7 + 2 * l]]
        assert kcm.interpolate(vals, n, l, i, cv.omega(n), cv.r) == co, t[:5]


# ---- the exports ----------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and ("int %s(" % name) in hdr
        assert getattr(lib, name).argtypes is not None, name
    assert _lib.ABI_VERSION == 5 and lib.apk_abi_version() == 5 and "#define APK_ABI_VERSION 5" in hdr          # additive


@pytest.mark.parametrize("cname", NAMES)
def test_argument_errors_come_before_the_device_and_write_nothing(cname):
    cv, _ = CURVES[cname]
    n, w = 8, 2 * cv.fp_bytes
    poly = C.create_string_buffer(cv.fr_vector([1] * n), 32 * n)
    mark = b"\xa5" * (w * n)
    h, vals = C.create_string_buffer(mark, w * n), C.create_string_buffer(mark[:32 * n], 32 * n)
    srs = C.create_string_buffer(w * n)
    for fn in (lib.apk_kzg_open_cosets, lib.apk_kzg_open_cosets_device):
        for bad in ((None, n, h, vals), (poly, 0, h, vals), (poly, n, None, vals), (poly, 1 << 40, h, vals)):
            assert fn(None, *bad) == ERR_ARG, bad[1]
            assert lib.apk_last_error(), "an argument error carries a message"
    assert lib.apk_kzg_cosets_prepare(None, None, n, 2) == ERR_ARG
    assert lib.apk_kzg_cosets_prepare(None, srs, 0, 2) == ERR_ARG
    for l in (0, 1, 3, 6):
        assert lib.apk_kzg_cosets_prepare(None, srs, n, l) == ERR_ARG, l
    assert h.raw == mark and vals.raw == mark[:32 * n]
    # everything but the context in order: the device is missed first where there is none (out_values may be null)
    want = ERR_HIP if _lib.device_count() == 0 else ERR_ARG
    for fn in (lib.apk_kzg_open_cosets, lib.apk_kzg_open_cosets_device):
        assert fn(None, poly, n, h, vals) == want
        assert fn(None, poly, n, h, None) == want
    assert lib.apk_kzg_cosets_prepare(None, srs, n, 2) == want
    if want == ERR_HIP:
        assert b"no CPU fallback" in lib.apk_last_error()
    assert h.raw == mark and vals.raw == mark[:32 * n]


# ---- the Python wrapper -----------------------------------------------------------------------------------------------------------
class _Key:
    def __init__(self, cv, n):
        self.curve, self.n = cv, n

    @property
    def ctx(self):
        raise AssertionError("the wrapper reached the library with bad arguments")


class _NoDomain:
    def __init__(self, cv):
        self.curve = cv

    ctx = _Key.ctx


def test_python_wrapper_argument_errors():
    cv, _ = CURVES["bn254"]
    key = _Key(cv, 8)
    w = 2 * cv.fp_bytes
    with pytest.raises(ValueError, match="domain"):
        ap_kzg.PrepareCosets(_NoDomain(cv), b"\0" * (w * 8), 2)
    for l in (0, 1, 3, 8):
        with pytest.raises(ValueError, match="coset size"):
            ap_kzg.PrepareCosets(key, b"\0" * (w * 8), l)
    with pytest.raises(ValueError, match="SRS"):
        ap_kzg.PrepareCosets(key, b"\0" * (w * 5), 2)          # n - l - 1 points
    with pytest.raises(AssertionError, match="reached the library"):
        ap_kzg.PrepareCosets(key, b"\0" * (w * 6), 2)
    for bad in ([], [1] * 9):
        with pytest.raises(ValueError):
            ap_kzg.OpenCosets(bad, key)
    with pytest.raises(ValueError, match="PrepareCosets"):
        ap_kzg.OpenCosets([1] * 8, key)
    key.kzg_coset_size = 2
    with pytest.raises(AssertionError, match="reached the library"):
        ap_kzg.OpenCosets([1] * 8, key)
    m = made("bn254", 8, 2)
    vk = ap_kzg.VerifyingKey(cv, cv.g1, m.g2)
    proof = ap_kzg.CosetOpeningProof(cv.g1_from_bytes(m.h[1]), m.vals(1))
    ap_kzg.VerifyCoset(cv.g1_from_bytes(m.digest), proof, 1, 2, vk, m.tau_pow_g2(2), m.srs, n=8)
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.VerifyCoset(cv.g1_from_bytes(m.digest), proof, 0, 2, vk, m.tau_pow_g2(2), m.srs, n=8)
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.VerifyCoset(cv.g1_from_bytes(m.digest), ap_kzg.CosetOpeningProof(proof.H, m.vals(1)[:1]), 1, 2, vk, m.tau_pow_g2(2), m.srs, n=8)
    with pytest.raises(ValueError):
        ap_kzg.VerifyCoset(cv.g1_from_bytes(m.digest), proof, 1, 2, vk, b"\0" * 5, m.srs, n=8)

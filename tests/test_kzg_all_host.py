"""CPU tier of the openings at every point of the domain (include/apk.h apk_kzg_all_prepare, apk_kzg_open_all*): the arrangement
the kernels run, restated in the exponent with a known tau (tests/kzg_all_model.py) and held to (f(tau) - f(w^i)) / (tau - w^i);
the twiddle split of csrc/kzg_all_twiddles.h, stand-alone under ASAN + UBSAN and once more in big integers; the exports; the
argument errors that come before the device check; the Python wrapper's argument errors."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import pytest

import kzg_all_model as kam
from algoplonk_amd import _lib, kzg as ap_kzg
from algoplonk_amd._lib import lib
from helpers import CURVES
from oracle.prng import SplitMix64, tau_from_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
NAMES = ["bn254", "bls12-381"]
OK, ERR_ARG, ERR_HIP = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_HIP
NEW = ["apk_kzg_all_prepare", "apk_kzg_open_all", "apk_kzg_open_all_device"]
HALF_BITS = 130      # csrc/glv_params.h


def _lengths(n):
    return sorted({1, 2, 3, n // 2 + 1, n - 1, n})


# ---- the arrangement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 16, 64])
@pytest.mark.parametrize("cname", NAMES)
def test_arrangement_gives_every_opening(cname, n):
    cv, _ = CURVES[cname]
    r = cv.r
    g = SplitMix64(0xA110 + n + cv.abi)
    tau = tau_from_seed(0xA11 + n, r)
    w_2n = cv.omega(2 * n)
    assert w_2n * w_2n % r == cv.omega(n)
    for L in _lengths(n):
        f = [g.fr(r) for _ in range(L)]
        want = kam.direct(f, n, cv.omega(n), tau, r)
        assert kam.arrangement(f, n, w_2n, tau, r) == want, (cname, n, L)
        if L == 1:
            assert want == [0] * n
        # the even / odd split of A^
        a, _ = kam.sequences(f, n, tau, r)
        a_hat = kam.dft(a, w_2n, r)
        even, odd = kam.a_hat_split(f, n, w_2n, r)
        assert a_hat[0::2] == even and a_hat[1::2] == odd, (cname, n, L)


@pytest.mark.parametrize("cname", NAMES)
def test_structured_polynomials_of_the_gpu_tier(cname):
    """What tests/test_gpu_kzg_all.py says of its structured inputs, at a small n: X opens to s_0 everywhere, X^(n-1) has
    h_k = s_(n-2-k), X + X^(n/2+1) has a quarter of A^ zero, and the two polynomials built from tau make h_0 = +-h_(n/2)."""
    cv, _ = CURVES[cname]
    r, n = cv.r, 16
    tau = tau_from_seed(0xA12, r)
    w, w_2n = cv.omega(n), cv.omega(2 * n)
    assert kam.direct([0, 1], n, w, tau, r) == [1] * n
    top = [0] * (n - 1) + [1]
    assert kam.h_terms(top, n, tau, r) == [pow(tau, n - 2 - k, r) for k in range(n - 1)] + [0]
    sparse = [0] * n
    sparse[1] = sparse[n // 2 + 1] = 1
    a, _ = kam.sequences(sparse, n, tau, r)
    assert kam.dft(a, w_2n, r).count(0) == n // 2
    g = SplitMix64(0xA13 + cv.abi)
    tail = [g.fr(r) for _ in range(n - 1 - n // 2)]
    for opposite in (False, True):
        f = kam.meeting_points(n, tau, r, tail, opposite)
        h = kam.h_terms(f, n, tau, r)
        assert h[n // 2] != 0 and h[0] == (-h[n // 2] % r if opposite else h[n // 2])
        assert kam.arrangement(f, n, w_2n, tau, r) == kam.direct(f, n, w, tau, r)


# ---- the twiddle split, stand-alone under ASAN + UBSAN and in big integers -----------------------------------------------------------
def test_twiddle_split_under_address_and_undefined_sanitizers():
    r = subprocess.run(["make", "-C", CSRC, "san-kzg-all"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "san", "kzg_all_check"), "12"], capture_output=True, text=True, timeout=600, env=env)
    n = 1 << 11
    assert r.returncode == 0 and "KZG ALL CHECK OK: %d twiddles per curve" % n in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    for cname in NAMES:
        cv, _ = CURVES[cname]
        rr = cv.r
        lam, w = [int(x, 16) for x in [l for l in lines if l.startswith("lambda %d " % cv.abi)][0].split()[2:]]
        assert lam not in (0, 1) and (lam * lam + lam + 1) % rr == 0          # a cube root of unity: the endomorphism's eigenvalue
        assert w == cv.omega(2 * n)
        tw = [l.split() for l in lines if l.startswith("tw %d " % cv.abi)]
        assert [int(t[2]) for t in tw] == list(range(n))
        cur = 1
        for t in tw:
            neg, k1, k2 = int(t[3]), int(t[4], 16), int(t[5], 16)
            assert k1 < 1 << HALF_BITS and k2 < 1 << HALF_BITS, t[2]
            k = ((-k1 if neg & 1 else k1) + (-k2 if neg & 2 else k2) * lam) % rr
            assert k == cur, (cname, t[2])
            cur = cur * w % rr


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
    for fn in (lib.apk_kzg_open_all, lib.apk_kzg_open_all_device):
        for bad in ((None, n, h, vals), (poly, 0, h, vals), (poly, n, None, vals), (poly, 1 << 40, h, vals)):
            assert fn(None, *bad) == ERR_ARG, bad[1]
            assert lib.apk_last_error(), "an argument error carries a message"
    assert lib.apk_kzg_all_prepare(None, None, n) == ERR_ARG
    assert lib.apk_kzg_all_prepare(None, srs, 0) == ERR_ARG
    assert h.raw == mark and vals.raw == mark[:32 * n]
    # everything but the context in order: the device is missed first where there is none (out_values may be null)
    want = ERR_HIP if _lib.device_count() == 0 else ERR_ARG
    for fn in (lib.apk_kzg_open_all, lib.apk_kzg_open_all_device):
        assert fn(None, poly, n, h, vals) == want
        assert fn(None, poly, n, h, None) == want
    assert lib.apk_kzg_all_prepare(None, srs, n) == want
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
    for bad in ([], [1] * 9):
        with pytest.raises(ValueError):
            ap_kzg.OpenAllDomain(bad, key)
    with pytest.raises(ValueError, match="domain"):
        ap_kzg.OpenAllDomain([1], _NoDomain(cv))
    with pytest.raises(ValueError):
        ap_kzg.PrepareAllDomain(key, b"\0" * (w * 6))          # n - 2 points
    with pytest.raises(AssertionError, match="reached the library"):
        ap_kzg.PrepareAllDomain(key, b"\0" * (w * 7))
    with pytest.raises(AssertionError, match="reached the library"):
        ap_kzg.OpenAllDomain([1] * 8, key)

"""CPU tier of the KZG openings in evaluation form (include/apk.h apk_kzg_open_lagrange*, apk_kzg_batch_open_lagrange*): the
big-integer model of tests/kzg_lagrange_model.py held to the canonical model of tests/kzg_model.py on the interpolated
coefficients, the new exports and their argument and no-device errors, and the Python wrappers' argument errors."""
from __future__ import annotations

import ctypes as C
import os

import pytest

import kzg_lagrange_model as klm
import kzg_model as km
from algoplonk_amd import _lib, kzg as ap_kzg
from algoplonk_amd._lib import lib
from helpers import CURVES
from oracle.prng import SplitMix64, tau_from_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254", "bls12-381"]
OK, ERR_ARG, ERR_HIP = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_HIP
NEW = ["apk_kzg_open_lagrange", "apk_kzg_open_lagrange_device", "apk_kzg_batch_open_lagrange", "apk_kzg_batch_open_lagrange_device",
       "apk_kzg_lagrange_shape"]


# ---- the model against the canonical model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("cname", NAMES)
def test_model_is_the_canonical_model_of_the_interpolant(cname, n):
    cv, ov = CURVES[cname]
    r = cv.r
    g = SplitMix64(0x1A6 + 7 * n + cv.abi)
    tau = tau_from_seed(0x1A60 + n, r)
    dom = klm.Domain(cv.omega(n), n, r)
    srs = klm.Srs(dom, tau)
    points = [g.fr(r), g.fr(r), 0, 1, r - 1, dom.pts[n - 1], dom.pts[3]]
    assert dom.find(points[0]) is None and dom.find(1) == 0 and dom.find(r - 1) == n // 2 and dom.find(dom.pts[n - 1]) == n - 1
    vectors = [klm.vector(kind, dom, g, m) for kind, m in (("random", 0), ("random", 0), ("zero", 0), ("constant", 0), ("one-hot", 0),
                                                            ("one-hot", n // 2), ("one-hot", n - 1), ("max", 0), ("top", 0))]
    for f in vectors:
        coeffs = dom.interpolate(f)
        assert [km.horner(coeffs, p, r) for p in dom.pts] == [x % r for x in f]
        assert klm.commit(ov, srs, f) == km.commit(ov, coeffs, tau)
        for z in points:
            assert klm.open_at(ov, srs, f, z) == km.open_at(ov, coeffs, z, tau), (cname, n, z)
    assert dom.interpolate(klm.vector("top", dom, g)) == [0] * (n - 1) + [1]
    # the batch: the same digests, values, challenge and H as the canonical batch over the coefficients
    some = vectors[:5]
    coeffs = [dom.interpolate(f) for f in some]
    for z in (points[0], dom.pts[n - 1]):
        for extra in (b"", b"data"):
            assert klm.batch_open_at(ov, srs, some, z, extra) == km.batch_open_at(ov, coeffs, z, tau, extra)


def test_batch_inverse():
    r = CURVES["bn254"][0].r
    xs = [1, 2, r - 1, 12345, 3]
    assert [x * y % r for x, y in zip(xs, klm.batch_inverse(xs, r))] == [1] * len(xs)


# ---- the exports --------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and ("int %s(" % name) in hdr
        assert getattr(lib, name).argtypes is not None, name
    assert _lib.ABI_VERSION == 5 and lib.apk_abi_version() == 5          # additive


def test_lagrange_shape_is_exported():
    a, b = C.c_int(0), C.c_int(0)
    assert lib.apk_kzg_lagrange_shape(C.byref(a), C.byref(b)) == OK
    assert a.value >= 1 and b.value % a.value == 0 and b.value // a.value in (64, 128, 256, 512, 1024)
    assert b.value >= 32          # span / 4 is a domain size
    assert lib.apk_kzg_lagrange_shape(None, C.byref(b)) == ERR_ARG
    assert lib.apk_kzg_lagrange_shape(C.byref(a), None) == ERR_ARG


def _open_args(cv, n=8):
    return (cv.fr_vector([1] * n), n, cv.fr_vector([2]), C.create_string_buffer(96), C.create_string_buffer(32))


def _batch_args(cv, count=2, n=8):
    bufs = [C.create_string_buffer(cv.fr_vector([1] * n), 32 * n) for _ in range(max(count, 1))]
    ptrs = (C.c_void_p * len(bufs))(*[C.addressof(b) for b in bufs])
    return bufs, ptrs, C.create_string_buffer(96), C.create_string_buffer(32 * len(bufs)), C.create_string_buffer(32)


@pytest.mark.parametrize("cname", NAMES)
def test_calls_need_a_device_and_a_context(cname):
    """Arguments other than the context first; then the device (no CPU fallback: APK_ERR_HIP without one); then the context."""
    cv, _ = CURVES[cname]
    want = ERR_HIP if _lib.device_count() == 0 else ERR_ARG
    ev, n, z, h, v = _open_args(cv)
    assert lib.apk_kzg_open_lagrange(None, ev, n, z, h, v) == want
    assert lib.apk_kzg_open_lagrange_device(None, ev, n, z, h, v) == want
    bufs, ptrs, bh, vals, gamma = _batch_args(cv)
    for count in (1, 2):
        assert lib.apk_kzg_batch_open_lagrange(None, count, ptrs, None, z, None, 0, bh, vals, gamma) == want
        assert lib.apk_kzg_batch_open_lagrange_device(None, count, ptrs, None, z, b"data", 4, bh, vals, None) == want
    bufs, ptrs, bh, vals, gamma = _batch_args(cv, 32)
    assert lib.apk_kzg_batch_open_lagrange(None, 32, ptrs, None, z, None, 0, bh, vals, gamma) == want
    if want == ERR_HIP:
        assert b"no CPU fallback" in lib.apk_last_error()


@pytest.mark.parametrize("cname", NAMES)
def test_argument_errors(cname):
    cv, _ = CURVES[cname]
    ev, n, z, h, v = _open_args(cv)
    for fn in (lib.apk_kzg_open_lagrange, lib.apk_kzg_open_lagrange_device):
        assert fn(None, ev, 0, z, h, v) == ERR_ARG                   # no values
        assert fn(None, ev, 1 << 40, z, h, v) == ERR_ARG             # no domain is that long
        assert fn(None, None, n, z, h, v) == ERR_ARG
        assert fn(None, ev, n, None, h, v) == ERR_ARG
        assert fn(None, ev, n, z, None, v) == ERR_ARG
        assert fn(None, ev, n, z, h, None) == ERR_ARG
    bufs, ptrs, bh, vals, gamma = _batch_args(cv, 33)
    for fn in (lib.apk_kzg_batch_open_lagrange, lib.apk_kzg_batch_open_lagrange_device):
        assert fn(None, 0, ptrs, None, z, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 33, ptrs, None, z, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 2, None, None, z, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 2, ptrs, None, None, None, 0, bh, vals, gamma) == ERR_ARG
        assert fn(None, 2, ptrs, None, z, None, 5, bh, vals, gamma) == ERR_ARG        # extra_len without extra
        assert fn(None, 2, ptrs, None, z, None, 0, None, vals, gamma) == ERR_ARG
        assert fn(None, 2, ptrs, None, z, None, 0, bh, None, gamma) == ERR_ARG
        holes = (C.c_void_p * 2)(ptrs[0], None)
        assert fn(None, 2, holes, None, z, None, 0, bh, vals, gamma) == ERR_ARG


# ---- the Python wrappers ------------------------------------------------------------------------------------------------------------
class _Key:
    """What the wrappers read of a plonk.ProvingKey before they reach the library."""

    def __init__(self, cv, n):
        self.curve, self.n = cv, n

    @property
    def ctx(self):
        raise AssertionError("the wrapper reached the library with bad arguments")


class _NoDomain:
    def __init__(self, cv):
        self.curve = cv

    ctx = _Key.ctx


def test_python_wrappers_argument_errors():
    cv, _ = CURVES["bn254"]
    key = _Key(cv, 8)
    for bad in ([], [1] * 7, [1] * 9, [1] * 11):
        with pytest.raises(ValueError):
            ap_kzg.CommitLagrange(bad, key)
        with pytest.raises(ValueError):
            ap_kzg.OpenLagrange(bad, 5, key)
        with pytest.raises(ValueError):
            ap_kzg.BatchOpenSinglePointLagrange([[1] * 8, bad], None, 5, key)
    with pytest.raises(ValueError):
        ap_kzg.BatchOpenSinglePointLagrange([], None, 5, key)
    with pytest.raises(ValueError):
        ap_kzg.BatchOpenSinglePointLagrange([[1] * 8, [2] * 8], [cv.g1], 5, key)       # one digest for two vectors
    for fn, args in ((ap_kzg.CommitLagrange, ([1] * 8,)), (ap_kzg.OpenLagrange, ([1] * 8, 5)),
                     (ap_kzg.BatchOpenSinglePointLagrange, ([[1] * 8], None, 5))):
        with pytest.raises(ValueError, match="domain"):
            fn(*args, _NoDomain(cv))

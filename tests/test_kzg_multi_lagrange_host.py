"""CPU tier of the evaluation-form openings at several points (include/apk.h apk_kzg_open_multi_lagrange*): the two exports, their
argument and no-device errors, the Python wrapper's argument errors, and the identity the GPU tier rests on - for mixed (vector,
point) pairs the big-integer model of tests/kzg_lagrange_model.py on the values is the canonical model of tests/kzg_model.py on
the interpolated coefficients."""
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
NEW = ["apk_kzg_open_multi_lagrange", "apk_kzg_open_multi_lagrange_device"]


def _fns():
    return [getattr(lib, name) for name in NEW]


# ---- the exports --------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and ("int %s(" % name) in hdr
        assert getattr(lib, name).argtypes is not None, name
    assert _lib.ABI_VERSION == 5 and lib.apk_abi_version() == 5          # additive


def _args(cv, count=2, n=8):
    bufs = [C.create_string_buffer(cv.fr_vector([1] * n), 32 * n) for _ in range(max(count, 1))]
    ptrs = (C.c_void_p * len(bufs))(*[C.addressof(b) for b in bufs])
    w = 2 * cv.fp_bytes
    return bufs, ptrs, cv.fr_vector([2] * len(bufs)), C.create_string_buffer(w * len(bufs)), C.create_string_buffer(32 * len(bufs))


@pytest.mark.parametrize("cname", NAMES)
def test_argument_errors_come_before_the_device(cname):
    cv, _ = CURVES[cname]
    bufs, ptrs, zs, h, vals = _args(cv, 33)
    for fn in _fns():
        for bad in ((0, ptrs, zs, h, vals), (33, ptrs, zs, h, vals), (2, None, zs, h, vals), (2, ptrs, None, h, vals),
                    (2, ptrs, zs, None, vals), (2, ptrs, zs, h, None)):
            assert fn(None, *bad) == ERR_ARG, bad[0]
            assert lib.apk_last_error(), "an argument error carries a message"


@pytest.mark.parametrize("cname", NAMES)
def test_calls_need_a_device_and_a_context(cname):
    """Arguments other than the context first; then the device (no CPU fallback: APK_ERR_HIP without one); then the context."""
    cv, _ = CURVES[cname]
    want = ERR_HIP if _lib.device_count() == 0 else ERR_ARG
    for count in (1, 2, 4, 5, 32):
        bufs, ptrs, zs, h, vals = _args(cv, count)
        for fn in _fns():
            assert fn(None, count, ptrs, zs, h, vals) == want
    one = (C.c_void_p * 3)(ptrs[0], ptrs[0], ptrs[0])      # a pointer may repeat
    for fn in _fns():
        assert fn(None, 3, one, zs, h, vals) == want
    if want == ERR_HIP:
        assert b"no CPU fallback" in lib.apk_last_error()


# ---- the Python wrapper -------------------------------------------------------------------------------------------------------------
class _Key:
    """What the wrapper reads of a plonk.ProvingKey before it reaches the library."""

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
    good = [1] * 8
    for bad in ([], [1] * 7, [1] * 9):
        with pytest.raises(ValueError):
            ap_kzg.OpenMultiPointsLagrange([good, bad], [5, 6], key)          # a wrong length
    with pytest.raises(ValueError):
        ap_kzg.OpenMultiPointsLagrange([], [], key)                           # no vectors
    with pytest.raises(ValueError):
        ap_kzg.OpenMultiPointsLagrange([good] * 33, list(range(33)), key)     # more than 32
    with pytest.raises(ValueError):
        ap_kzg.OpenMultiPointsLagrange([good, good], [5], key)                # one point for two vectors
    with pytest.raises(ValueError, match="domain"):
        ap_kzg.OpenMultiPointsLagrange([good], [5], _NoDomain(cv))
    with pytest.raises(AssertionError, match="reached the library"):          # well-formed arguments do reach it
        ap_kzg.OpenMultiPointsLagrange([good] * 32, list(range(32)), key)


# ---- the model identity the GPU tier rests on ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("cname", NAMES)
def test_model_of_mixed_pairs_is_the_canonical_model_of_the_interpolants(cname, n):
    cv, ov = CURVES[cname]
    r = cv.r
    g = SplitMix64(0x1AB + 7 * n + cv.abi)
    tau = tau_from_seed(0x1AB0 + n, r)
    dom = klm.Domain(cv.omega(n), n, r)
    srs = klm.Srs(dom, tau)
    f, f2 = klm.vector("random", dom, g), klm.vector("random", dom, g)
    hot = klm.vector("one-hot", dom, g, 3)
    m = n // 2 + 1
    # off the domain, 0, omega^m, and the same vector twice (at two points, and the same pair again)
    pairs = [(f, g.fr(r)), (f2, 0), (f, dom.pts[m]), (f, g.fr(r)), (hot, dom.pts[3]), (f2, dom.pts[n - 1]), (f, dom.pts[m]),
             (klm.vector("constant", dom, g), g.fr(r)), (klm.vector("top", dom, g), dom.pts[1])]
    assert dom.find(pairs[0][1]) is None and dom.find(pairs[2][1]) == m
    coeffs = {}
    for vec, z in pairs:
        if id(vec) not in coeffs:
            coeffs[id(vec)] = dom.interpolate(vec)
        got = klm.open_at(ov, srs, vec, z)
        assert got == km.open_at(ov, coeffs[id(vec)], z, tau), (cname, n, z)
        if dom.find(z) is not None:
            assert got[1] == vec[dom.find(z)]
    assert klm.open_at(ov, srs, *pairs[2]) == klm.open_at(ov, srs, *pairs[6])

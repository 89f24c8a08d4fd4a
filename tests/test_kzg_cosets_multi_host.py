"""CPU tier of apk_kzg_open_cosets_multi* beside the planner (tests/test_kzg_cosets_multi_plan.py): the two exports exist, are declared
in include/apk.h with their limit, listed and bound in _lib.py, and the ABI version stays; without a GPU the calls miss the device
first and write nothing; the Python wrapper raises its argument errors before it reaches the library.  No GPU."""
from __future__ import annotations

import ctypes as C
import os

import pytest

from algoplonk_amd import _lib, kzg as ap_kzg
from algoplonk_amd._lib import lib
from helpers import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["apk_kzg_open_cosets_multi", "apk_kzg_open_cosets_multi_device"]
ERR_ARG, ERR_HIP = _lib.APK_ERR_ARG, _lib.APK_ERR_HIP


def test_new_exports_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and ("int %s(" % name) in hdr
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == 6, name
        assert fn.argtypes[1] is C.c_uint32 and fn.argtypes[2] is C.POINTER(C.c_void_p) and fn.argtypes[3] is C.POINTER(C.c_uint64), name
    assert "#define APK_KZG_COSETS_MULTI_MAX 64" in hdr and ap_kzg.COSETS_MULTI_MAX == 64
    assert _lib.ABI_VERSION == 5 and lib.apk_abi_version() == 5 and "#define APK_ABI_VERSION 5" in hdr          # additive


@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_no_context_or_no_device_writes_nothing(cname):
    cv, _ = CURVES[cname]
    n, w = 8, 2 * cv.fp_bytes
    poly = C.create_string_buffer(cv.fr_vector([1] * n), 32 * n)
    mark = b"\xa5" * (w * n)
    h, vals = C.create_string_buffer(mark, w * n), C.create_string_buffer(mark[:64 * n], 64 * n)
    ptrs = (C.c_void_p * 2)(C.addressof(poly), C.addressof(poly))
    lens = (C.c_uint64 * 2)(n, n)
    # a usable device, then the context: every other rule needs the context's state and comes after both
    want = ERR_HIP if _lib.device_count() == 0 else ERR_ARG
    for fn in (lib.apk_kzg_open_cosets_multi, lib.apk_kzg_open_cosets_multi_device):
        for args in ((2, ptrs, lens, h, vals), (0, ptrs, lens, h, vals), (65, ptrs, lens, h, None), (2, None, None, None, None)):
            assert fn(None, *args) == want, args[0]
            assert lib.apk_last_error(), "an error carries a message"
    if want == ERR_HIP:
        assert b"no CPU fallback" in lib.apk_last_error()
    else:
        assert lib.apk_last_error() == b"null context"
    assert h.raw == mark and vals.raw == mark[:64 * n]


class _Key:
    def __init__(self, cv, n):
        self.curve, self.n = cv, n

    @property
    def ctx(self):
        raise AssertionError("the wrapper reached the library with bad arguments")


def test_python_wrapper_argument_errors():
    cv, _ = CURVES["bn254"]
    key = _Key(cv, 8)
    good = [1] * 8
    with pytest.raises(ValueError, match="number of polynomials"):
        ap_kzg.OpenCosetsMulti([], key)
    with pytest.raises(ValueError, match="number of polynomials"):
        ap_kzg.OpenCosetsMulti([good] * 65, key)
    with pytest.raises(ValueError, match="polynomial 1"):
        ap_kzg.OpenCosetsMulti([good, []], key)
    with pytest.raises(ValueError, match="polynomial 2"):
        ap_kzg.OpenCosetsMulti([good, good, [1] * 9], key)
    with pytest.raises(ValueError, match="PrepareCosets"):
        ap_kzg.OpenCosetsMulti([good] * 64, key)
    key.kzg_coset_size = 2
    with pytest.raises(AssertionError, match="reached the library"):
        ap_kzg.OpenCosetsMulti([good] * 64, key)

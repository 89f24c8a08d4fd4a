"""CPU tier: the load-time claim on GPU_MAX_HW_QUEUES (algoplonk_amd/csrc/runtime_env.h, apk_api.cpp) and apk_runtime_read.

ROCm maps a process's HIP streams onto GPU_MAX_HW_QUEUES hardware queues and reads the variable once, when the runtime
initialises.  The library needs a queue per proving stream: 16 (more costs a lone proof latency).  Its constructor
therefore RAISES the variable to the need when the library is loaded - a value at or above the need stays as the host set it, a
lower, missing or unreadable one becomes the need - and APK_HW_QUEUES sets the need (4 .. 32) or, with 0, leaves the environment
exactly as found.  The constructor runs once per process, so every case is a fresh child; the child reads the C environment
through libc's getenv and the library's record through apk_runtime_read (Python's os.environ does not see a C setenv).  Nothing
here has a GPU in it.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSET, UNREADABLE = -1, -2
NEED, LO, HI = 16, 4, 32

_CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, %r)
libc = C.CDLL(None)
libc.getenv.restype = C.c_char_p
libc.getenv.argtypes = [C.c_char_p]
cenv = lambda: (lambda v: None if v is None else v.decode())(libc.getenv(b"GPU_MAX_HW_QUEUES"))
out = {"c_before": cenv()}
from algoplonk_amd import _lib
from algoplonk_amd._lib import lib
out["c_after"] = cenv()
out["py_after"] = os.environ.get("GPU_MAX_HW_QUEUES")
out["size"] = C.sizeof(_lib.Runtime)
out["loaded"] = _lib.runtime()
out["rc_null"] = lib.apk_runtime_read(None)
if os.environ.get("TEST_HOST_CHANGES"):
    libc.setenv(b"GPU_MAX_HW_QUEUES", os.environ["TEST_HOST_CHANGES"].encode(), 1)
n = C.c_int(-1)
out["rc_count"] = lib.apk_device_count(C.byref(n))          # the library's first call into the HIP runtime
out["called"] = _lib.runtime()
libc.setenv(b"GPU_MAX_HW_QUEUES", b"5", 1)                     # later changes do not rewrite the record of the first call
lib.apk_device_count(C.byref(n))
out["later"] = _lib.runtime()
print("RESULT " + json.dumps(out))
"""


def _child(found, knob, **extra):
    e = dict(os.environ)
    for k in ("GPU_MAX_HW_QUEUES", "APK_HW_QUEUES", "TEST_HOST_CHANGES"):
        e.pop(k, None)
    if found is not None:
        e["GPU_MAX_HW_QUEUES"] = found
    if knob is not None:
        e["APK_HW_QUEUES"] = knob
    e.update(extra)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _value(s):
    """The rule's reading of a variable, restated: decimal digits and nothing else, UNSET, or UNREADABLE."""
    if s is None:
        return UNSET
    return int(s) if s and all(c in "0123456789" for c in s) else UNREADABLE


def _expect(found, knob):
    """(need, left, written) by the raise-only rule."""
    f, k = _value(found), _value(knob)
    if k == 0:
        return 0, f, 0
    need = min(max(k, LO), HI) if k > 0 else NEED
    return (need, f, 0) if f >= need else (need, need, 1)


@pytest.mark.parametrize("knob", [None, "0", "8", "32"])
@pytest.mark.parametrize("found", [None, "4", "8", "16", "24", "32", "", "many"])
def test_the_claim_is_raise_only(found, knob):
    got = _child(found, knob)
    need, left, written = _expect(found, knob)
    rt = got["loaded"]
    assert got["size"] == 32 and got["rc_null"] == 1, got                       # APK_ERR_ARG for a null out
    assert got["c_before"] == found and got["py_after"] == found, got             # the child started from the case's environment
    assert rt["hw_queues_found"] == _value(found), got
    assert (rt["hw_queues_need"], rt["hw_queues_left"], rt["hw_queues_written"]) == (need, left, written), (got, need, left, written)
    if written:
        # raised: the C environment holds the need, which is never outside 4 .. 32 and never below what was found
        assert got["c_after"] == str(need) and LO <= need <= HI and need > _value(found), got
    else:
        # left alone - with APK_HW_QUEUES=0 whatever it held, unreadable or missing included; otherwise because it was enough
        assert got["c_after"] == found, got
        assert knob == "0" or _value(found) >= need, got
    assert rt["hw_queues_now"] == _value(got["c_after"]) and rt["first_hip_call"] == -1, got
    # the library's first HIP call found what the constructor left ...
    assert got["rc_count"] == 0, got
    called = got["called"]
    assert called["first_hip_call"] == 1 and called["hw_queues_at_first_hip"] == left, got
    # ... and that record stays when the variable changes later (the runtime has read it by then)
    later = got["later"]
    assert later["hw_queues_now"] == 5 and later["first_hip_call"] == 1 and later["hw_queues_at_first_hip"] == left, got
    assert {k: later[k] for k in ("hw_queues_found", "hw_queues_left", "hw_queues_need", "hw_queues_written")} == \
           {k: rt[k] for k in ("hw_queues_found", "hw_queues_left", "hw_queues_need", "hw_queues_written")}, got


@pytest.mark.parametrize("knob,need", [("1", 4), ("3", 4), ("", NEED), ("x", NEED), ("-7", NEED)])
def test_a_small_or_unreadable_knob(knob, need):
    """A need below 4 is held to 4; an unreadable knob is no knob.  (No case asks for more than 32: the rule clamps there too.)"""
    got = _child("4", knob)
    rt = got["loaded"]
    assert rt["hw_queues_need"] == need and rt["hw_queues_written"] == (1 if need > 4 else 0), got
    assert got["c_after"] == str(need), got


@pytest.mark.parametrize("found,value", [(" 8", UNREADABLE), ("+8", UNREADABLE), ("8 ", UNREADABLE), ("4x", UNREADABLE), ("0x20", UNREADABLE),
                                         ("-4", UNREADABLE), ("2.5e1", UNREADABLE), ("028", 28), ("0", 0)])
def test_the_accepted_grammar_is_decimal_digits_only(found, value):
    """No sign, no blanks, no suffix: what the HIP runtime's own parser would make of such a string does not matter, because an
    unreadable value is raised to the need.  The same grammar reads APK_HW_QUEUES (an unreadable knob is no knob)."""
    got = _child(found, None)
    rt = got["loaded"]
    assert rt["hw_queues_found"] == value == _value(found), got
    assert got["c_after"] == (found if value >= NEED else str(NEED)) and rt["hw_queues_written"] == (0 if value >= NEED else 1), got
    got = _child("4", found)
    want = NEED if value == UNREADABLE else 0 if value == 0 else min(max(value, LO), HI)
    assert got["loaded"]["hw_queues_need"] == want, got


# every export that can be the FIRST of the library to reach the HIP runtime records that moment (runtime_env.h, the invariant
# beside runtime_checkpoint): each one alone in a fresh process, with arguments that are harmless with and without a GPU
_WALK = {
    "apk_device_count": "lib.apk_device_count(C.byref(C.c_int(0)))",
    "apk_ctx_create": "lib.apk_ctx_create(C.byref(_lib.CircuitDesc()), C.byref(C.c_void_p()))",
    "apk_msm_ctx_create": "lib.apk_msm_ctx_create(0, 0, z, 0, 0, C.byref(C.c_void_p()))",
    "apk_host_alloc": "lib.apk_host_alloc(0, 64, C.byref(hp)); lib.apk_host_free(hp)",
    "apk_host_register": "lib.apk_host_register(z, 4096) == 0 and lib.apk_host_unregister(z)",
    "apk_kzg_open": "lib.apk_kzg_open(None, z, 1, z, o, o)",
    "apk_kzg_batch_open": "lib.apk_kzg_batch_open(None, 1, (C.c_void_p * 1)(C.addressof(z)), (C.c_uint64 * 1)(1), z, z, None, 0, o, o, o)",
    "apk_g1_mul_batch": "lib.apk_g1_mul_batch(0, 0, z, z, 1, o)",
    "apk_g1_decompress": "lib.apk_g1_decompress(0, 0, z, 1, o)",
    "apk_g1_to_lagrange": "lib.apk_g1_to_lagrange(0, 0, z, 2, o)",
    "apk_device_fe_op": "lib.apk_device_fe_op(0, 0, 0, 0, 1, z, z, o)",
    "apk_device_feu_op": "lib.apk_device_feu_op(0, 0, 0, 0, 1, z, o)",
    "apk_device_g1_op": "lib.apk_device_g1_op(0, 0, 0, 1, z, z, o)",
    "apk_verify_batch": "lib.apk_verify_batch(0, C.byref(_lib.VerifyingKey()), None, None, None, 0, None, None)",
    "apk_verify_batch_keys": "lib.apk_verify_batch_keys(0, None, 0, None, None, None, None, 0, None, None)",
    "apk_verify_blobs": "lib.apk_verify_blobs(0, None, 0, None, None, None, None, None, 0, None, None)",
    "apk_g1_lincomb_segments": "lib.apk_g1_lincomb_segments(0, 0, z, z, (C.c_uint64 * 2)(0, 1), 1, o)",
}

_WALK_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
from algoplonk_amd import _lib
from algoplonk_amd._lib import lib
z, o, hp = C.create_string_buffer(4096), C.create_string_buffer(4096), C.c_void_p()
before = _lib.runtime()["first_hip_call"]
%s
print("RESULT " + json.dumps({"before": before, "after": _lib.runtime()}))
"""


@pytest.mark.parametrize("export", sorted(_WALK))
def test_every_device_taking_export_records_the_first_hip_call(export):
    e = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    e.pop("APK_HW_QUEUES", None)
    r = subprocess.run([sys.executable, "-c", _WALK_CHILD % (ROOT, _WALK[export])], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert got["before"] == -1, got
    assert got["after"]["first_hip_call"] == 1 and got["after"]["hw_queues_at_first_hip"] == NEED, (export, got)


def test_a_host_that_changes_the_variable_before_the_first_hip_call_shows():
    got = _child("4", None, TEST_HOST_CHANGES="8")
    assert got["loaded"]["hw_queues_left"] == NEED and got["loaded"]["first_hip_call"] == -1, got
    assert got["called"]["first_hip_call"] == 0 and got["called"]["hw_queues_at_first_hip"] == 8, got
    got = _child("4", None, TEST_HOST_CHANGES=str(NEED))                                # rewritten to the same value: nothing changed
    assert got["called"]["first_hip_call"] == 1, got


def test_binding_and_header_agree():
    import re
    from algoplonk_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    assert "apk_runtime_read" in _lib.SYMBOLS and "int apk_runtime_read(apk_runtime* out);" in hdr
    body = hdr[hdr.index("typedef struct {\n    int32_t hw_queues_found;"):hdr.index("} apk_runtime;")]
    fields = re.findall(r"\b([a-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == _lib.Runtime._names, fields
    assert "#define APK_HWQ_UNSET (-1)" in hdr and "#define APK_HWQ_UNREADABLE (-2)" in hdr
    assert _lib.ABI_VERSION == 5 and "#define APK_ABI_VERSION 5" in hdr            # additive

"""CPU tier: the device-wide scheduler (algoplonk_amd/csrc/device_sched.h).  A process that serves several circuits holds several
contexts on one GPU; they share the device's proving streams, its load figure and one first-come-first-served order.  None of
that has a GPU in it:

  * tools/san/sched_hammer.cpp : three gates on one scheduler plus a gate on a second device ordinal, 96 threads, under
    ThreadSanitizer and AddressSanitizer - the hammer asserts the invariants itself (its header lists them) and exits non-zero on
    a breach; a report from either sanitizer fails the test;
  * tools/san/host_hammer.cpp  : a gate that was never attached still builds and behaves as before;
  * apk_device_sched_read      : host state only - it answers without a GPU and before any context exists.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
SAN_ENV = dict(TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1:exitcode=67")


def _make(san, target):
    r = subprocess.run(["make", "-C", CSRC, "SAN=%s" % san, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("san", ["thread", "address"])
def test_scheduler_hammer_under_the_sanitizers(san):
    _make(san, "san-sched")
    r = subprocess.run([os.path.join(ROOT, "tools", "san", "sched_hammer_%s" % san)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **SAN_ENV))
    print(r.stdout)
    assert r.returncode == 0 and "SCHED HAMMER OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
    # the scenes the hammer is there for did happen: leads queued for streams across contexts, gangs formed with 16 + 16 callers
    assert "0 served out of turn" in r.stdout and "gangs expected in both" in r.stdout and "none expected" in r.stdout


@pytest.mark.parametrize("san", ["thread", "address"])
def test_an_unattached_gate_is_what_it_was(san):
    """host_hammer.cpp as committed: SlotGate without a scheduler keeps a private budget of its own max_streams."""
    _make(san, "san-hammer")
    r = subprocess.run([os.path.join(ROOT, "tools", "san", "host_hammer_%s" % san)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0 and "SAN HAMMER OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]


_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, %r)
import algoplonk_amd
from algoplonk_amd import _lib
from algoplonk_amd._lib import lib
out = {"abi": lib.apk_abi_version(), "size": C.sizeof(_lib.DeviceSched), "paths_size": C.sizeof(_lib.PathCounts)}
ds = _lib.DeviceSched()
out["rc"] = lib.apk_device_sched_read(0, C.byref(ds), 0)
out["dev0"] = ds.as_dict()
out["rc7"] = lib.apk_device_sched_read(7, C.byref(ds), 1)
out["dev7"] = ds.as_dict()
out["rc_neg"] = lib.apk_device_sched_read(-1, C.byref(ds), 0)
out["err_neg"] = (lib.apk_last_error() or b"").decode()
out["rc_null"] = lib.apk_device_sched_read(0, None, 0)
out["py"] = algoplonk_amd.device_sched(device=0, reset=True)
print("RESULT " + json.dumps(out))
"""


def _child(**env):
    e = dict(os.environ)
    for k in ("APK_MAX_SLOTS", "APK_DEVICE_SCHED"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_device_sched_read_is_host_state_only():
    """In a fresh process, before any context exists (and without a GPU where there is none): APK_OK, zero counts, the budget."""
    got = _child()
    assert got["abi"] == 5
    assert got["size"] == 32 and got["paths_size"] == 24 * 8          # additive: no existing struct changed size
    zero = dict(contexts=0, max_streams=16, streams_in_use=0, streams_peak=0, proofs_in_flight=0, proofs_peak=0, waiting=0, device_wide=1)
    assert got["rc"] == 0 and got["dev0"] == zero, got
    assert got["rc7"] == 0 and got["dev7"] == zero, got                # the registry is keyed by ordinal, whatever devices exist
    assert got["py"] == zero, got
    assert got["rc_neg"] == 1 and "device" in got["err_neg"], got      # APK_ERR_ARG
    assert got["rc_null"] == 1, got


def test_the_budget_follows_apk_max_slots_and_the_switch():
    got = _child(APK_MAX_SLOTS="6")
    assert got["rc"] == 0 and got["dev0"]["max_streams"] == 6 and got["dev0"]["device_wide"] == 1, got
    got = _child(APK_DEVICE_SCHED="0", APK_MAX_SLOTS="12")
    assert got["rc"] == 0 and got["dev0"]["device_wide"] == 0 and got["dev0"]["max_streams"] == 12 and got["dev0"]["contexts"] == 0, got


def test_binding_and_header_agree():
    from algoplonk_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    assert "apk_device_sched_read" in _lib.SYMBOLS and "int apk_device_sched_read(int device, apk_device_sched* out, int reset);" in hdr
    assert "forms_by_device_load" in hdr and _lib.PathCounts._names[-1] == "forms_by_device_load"
    body = hdr[hdr.index("typedef struct {\n    uint32_t contexts;"):hdr.index("} apk_device_sched;")]
    import re
    fields = re.findall(r"\b([a-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body))
    assert fields == _lib.DeviceSched._names, fields

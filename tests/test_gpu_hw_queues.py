"""-m gpu: the hardware-queue claim on a real runtime.  A machine that exports GPU_MAX_HW_QUEUES=4 in front of every command has
"set" the variable: the library's load-time constructor raises it to its need all the same (csrc/runtime_env.h), and with
APK_HW_QUEUES=0 it leaves the environment exactly as found and schedules as it always did.  Either way the proofs are the C
oracle's, byte for byte: how many queues the streams land on changes when kernels run, never what they compute.

The constructor runs once per process and the runtime reads the variable once, so each case is a fresh child with a time limit of
its own.  The circuit is BN254 2^10 with 8 callers, 2 proofs each, over 4 distinct assignments - callers outnumber the 4 queues
of the second case.  The oracle's blobs are computed once, here, and handed to both children.
"""
import json
import os
import subprocess
import sys

import pytest

from algoplonk_amd import batch, setup as ap_setup, workloads
from bench_cpu import oracle_blobs

from helpers import CURVES, oracle_threads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N, SEED, CALLERS, ROUNDS, K = 10, 0x4851, 8, 2, 4

_CHILD = r"""
import ctypes as C, json, sys, threading
sys.path.insert(0, %(root)r)
from algoplonk_amd import _lib, batch, ecc, plonk, setup, workloads
from algoplonk_amd._lib import lib, check
log_n, seed, callers, rounds, K = %(log_n)d, %(seed)d, %(callers)d, %(rounds)d, %(k)d
out = {"loaded": _lib.runtime()}
libc = C.CDLL(None)
libc.getenv.restype = C.c_char_p
libc.getenv.argtypes = [C.c_char_p]
v = libc.getenv(b"GPU_MAX_HW_QUEUES")
out["c_env"] = None if v is None else v.decode()
cv = ecc.BN254
wl = workloads.random_circuit(cv, log_n, seed)
srs = setup.unsafe_srs(cv, wl.ccs.domain_size(), wl.tau, device=0)
pk, vk = plonk.Setup(wl.ccs, srs, device=0, slots=callers)
ws = batch.WitnessSet(pk, wl.ccs, workloads.variants(wl, K, seed)).to_device()
pk.paths(reset=True)
got, errors, lock = [], [], threading.Lock()
def worker(i):
    pr = _lib.Proof()
    for r in range(rounds):
        a = (i + r) %% K
        rc = ws.prove(a, pr, "device")
        if rc != 0:
            errors.append((rc, (lib.apk_last_error() or b"").decode()))
            return
        buf = C.create_string_buffer(2048)
        ln = C.c_size_t(0)
        check(lib.apk_marshal_proof(C.byref(pr), buf, 2048, C.byref(ln)))
        with lock:
            got.append((a, buf.raw[:ln.value].hex()))
th = [threading.Thread(target=worker, args=(i,)) for i in range(callers)]
[t.start() for t in th]
[t.join() for t in th]
out["errors"], out["blobs"] = errors, got
out["paths"] = pk.paths()
out["sched"] = _lib.device_sched(0)
out["after"] = _lib.runtime()
ws.close()
pk.close()
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def want(gpu):
    """The C oracle's blob for each of the K assignments (the children rebuild the same seeded circuit, SRS and assignments)."""
    cv, _ = CURVES["bn254"]
    wl = workloads.random_circuit(cv, LOG_N, SEED)
    srs = ap_setup.unsafe_srs(cv, wl.ccs.domain_size(), wl.tau, device=gpu)
    items = batch.WitnessSet(None, wl.ccs, workloads.variants(wl, K, SEED), curve=cv).items
    blobs = oracle_blobs(cv, wl.ccs, srs, items, threads=oracle_threads(), check_first_against_plain=True)
    assert len(set(blobs)) == K and None not in blobs, "the assignments are meant to be distinct and satisfying"
    return [b.hex() for b in blobs]


def _child(**env):
    e = dict(os.environ)
    for k in ("GPU_MAX_HW_QUEUES", "APK_HW_QUEUES", "APK_MAX_SLOTS", "APK_GANG", "APK_DEVICE_SCHED"):
        e.pop(k, None)
    e.update(env)
    src = _CHILD % dict(root=ROOT, log_n=LOG_N, seed=SEED, callers=CALLERS, rounds=ROUNDS, k=K)
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=240, env=e, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _assert_proofs(got, want):
    assert not got["errors"], got["errors"][0]
    assert len(got["blobs"]) == CALLERS * ROUNDS and {a for a, _ in got["blobs"]} == set(range(K))
    wrong = [(a, b[:24]) for a, b in got["blobs"] if b != want[a]]
    assert not wrong, "%d blob(s) differ from the C oracle's proof of the SAME inputs: %s" % (len(wrong), wrong[:4])
    assert got["paths"]["proofs"] == CALLERS * ROUNDS, got["paths"]


def test_four_queues_in_the_environment_are_raised_to_the_need(want):
    got = _child(GPU_MAX_HW_QUEUES="4")
    rt = got["loaded"]
    assert rt["hw_queues_found"] == 4 and rt["hw_queues_need"] == 16 and rt["hw_queues_left"] == rt["hw_queues_need"], rt
    assert rt["hw_queues_written"] == 1 and got["c_env"] == "16", got["c_env"]
    # the C environment still held what the constructor left at the library's first HIP call.  (Whether the RUNTIME took the value
    # is not visible from inside the process: only a kernel trace's queue count shows it - profiles/hw_queues_ab.txt.)
    assert got["after"]["first_hip_call"] == 1 and got["after"]["hw_queues_at_first_hip"] == 16, got["after"]
    _assert_proofs(got, want)
    assert got["sched"]["max_streams"] == 16 and got["paths"]["gang_proofs"] == 0, (got["sched"], got["paths"])


def test_apk_hw_queues_0_leaves_four_queues_and_the_defaults(want):
    """No rule follows the queue count (the sweep of profiles/hw_queues_ab.txt found no stream budget or gang size that beats 16
    lone streams on 4 queues): the stream budget and the gangs are the unchanged defaults - 16 streams, and no gang with 8 callers."""
    got = _child(GPU_MAX_HW_QUEUES="4", APK_HW_QUEUES="0")
    rt = got["loaded"]
    assert (rt["hw_queues_found"], rt["hw_queues_left"], rt["hw_queues_need"], rt["hw_queues_written"]) == (4, 4, 0, 0), rt
    assert got["c_env"] == "4"
    assert got["after"]["first_hip_call"] == 1 and got["after"]["hw_queues_at_first_hip"] == 4, got["after"]
    _assert_proofs(got, want)
    assert got["sched"]["max_streams"] == 16 and got["sched"]["device_wide"] == 1, got["sched"]
    assert got["sched"]["streams_peak"] <= 8 and got["paths"]["gang_proofs"] == 0, (got["sched"], got["paths"])

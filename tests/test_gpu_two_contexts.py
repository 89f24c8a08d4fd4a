"""-m gpu: several contexts proving on ONE GPU at the same time (the device-wide scheduler, csrc/device_sched.h).

A process that serves several circuits holds one context per compiled circuit - the reference's integration tests compile one per
curve in one process.  Until the scheduler every context scheduled as if it owned the GPU: 16 streams of its own, kernel forms
chosen from its own busy count.  Here two contexts prove together - distinct assignments per caller, every blob held to the C
oracle's proof of ITS OWN inputs under ITS OWN circuit, as in test_gpu_load.py - while a sampler reads apk_device_sched_read: the
device never runs more proving streams than its budget, the load figure a context chooses its kernel forms from is the device's,
a context can be destroyed while another proves, and APK_DEVICE_SCHED=0 still gives the same bytes.
"""
import ctypes as C
import dataclasses
import gc
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from algoplonk_amd import _lib, batch, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd._lib import lib, check

from helpers import CURVES, oracle_threads

pytestmark = pytest.mark.gpu

K = 6                                                  # distinct assignments per circuit
SPECS = {"bn254-17": ("bn254", 17, 0xD5C0), "bls12-381-14": ("bls12-381", 14, 0xD5C1), "bn254-15": ("bn254", 15, 0xD5C2)}
_HOST = {}


def _marshal(pr) -> bytes:
    out = C.create_string_buffer(2048)
    ln = C.c_size_t(0)
    check(lib.apk_marshal_proof(C.byref(pr), out, 2048, C.byref(ln)))
    return out.raw[: ln.value]


def _host(name, gpu, oracle=True):
    """The host half of a circuit, made once per process: workload, SRS, packed assignments and (oracle=True) the C oracle's blobs."""
    if name not in _HOST:
        cname, log_n, seed = SPECS[name]
        cv, ov = CURVES[cname]
        wl = workloads.random_circuit(cv, log_n, seed)
        srs = ap_setup.unsafe_srs(cv, wl.ccs.domain_size(), wl.tau, device=gpu)
        items = batch.WitnessSet(None, wl.ccs, workloads.variants(wl, K, seed), curve=cv).items
        _HOST[name] = dict(cv=cv, wl=wl, srs=srs, items=items, want=None)
    h = _HOST[name]
    if oracle and h["want"] is None:
        from bench_cpu import oracle_blobs
        h["want"] = oracle_blobs(h["cv"], h["wl"].ccs, h["srs"], h["items"], threads=oracle_threads(), check_first_against_plain=True)
        assert len(set(h["want"])) == K, "the assignments are meant to be distinct"
    return h


class Rig:
    """A context of its own over a cached circuit, its assignments resident on the device."""

    def __init__(self, name, gpu, slots, oracle=True):
        h = _host(name, gpu, oracle)
        self.name, self.want = name, h["want"]
        self.pk, self.vk = ap_plonk.Setup(h["wl"].ccs, h["srs"], device=gpu, slots=slots)
        self.ws = batch.WitnessSet(self.pk, h["wl"].ccs, [])
        self.ws.items = [dataclasses.replace(it, dev=None, pinned=None) for it in h["items"]]
        self.ws.to_device()

    def close(self):
        self.ws.close()
        self.pk.close()


class Callers:
    """`callers` threads on one rig; caller i proves assignment (i + 3 r) % K in round r - `rounds` of them, or until `stop` is set."""

    def __init__(self, rig, callers, rounds=None, stop=None):
        self.rig, self.rounds, self.stop = rig, rounds, stop
        self.got, self.errors, self.lock = {}, [], threading.Lock()
        self.threads = [threading.Thread(target=self._work, args=(i,)) for i in range(callers)]

    def _work(self, i):
        pr = _lib.Proof()
        r = 0
        while (r < self.rounds) if self.rounds is not None else not self.stop.is_set():
            a = (i + 3 * r) % K
            rc = self.rig.ws.prove(a, pr, "device")
            if rc != 0:
                self.errors.append((self.rig.name, rc, lib.apk_last_error()))
                return
            blob = _marshal(pr)
            with self.lock:
                self.got[(a, blob)] = self.got.get((a, blob), 0) + 1
            r += 1

    def start(self):
        [t.start() for t in self.threads]
        return self

    def join(self):
        [t.join() for t in self.threads]
        return self

    def check(self, want, what, total=None):
        assert not self.errors, self.errors[0]
        wrong = [(a, hashlib.sha256(b).hexdigest()[:12], c) for (a, b), c in self.got.items() if b != want[a]]
        assert not wrong, "%s: %d blob(s) differ from the C oracle's proof of the SAME inputs: %s" % (what, len(wrong), wrong[:6])
        if total is not None:
            assert sum(self.got.values()) == total, (what, sum(self.got.values()), total)


class Sampler:
    """Reads apk_device_sched_read for as long as it runs: the budget must hold at every moment, not only at the end."""

    def __init__(self, gpu):
        self.gpu, self.stop, self.samples, self.over, self.contexts = gpu, threading.Event(), 0, [], set()
        self.t = threading.Thread(target=self._work)

    def _work(self):
        while not self.stop.is_set():
            d = _lib.device_sched(self.gpu)
            self.samples += 1
            self.contexts.add(d["contexts"])
            if d["streams_in_use"] > d["max_streams"] or d["streams_peak"] > d["max_streams"]:
                self.over.append(d)
            time.sleep(0.002)

    def __enter__(self):
        self.t.start()
        return self

    def __exit__(self, *a):
        self.stop.set()
        self.t.join()


def _wait_for(cond, what, seconds=120):
    t0 = time.time()
    while not cond():
        assert time.time() - t0 < seconds, "timed out waiting for %s: %s" % (what, _lib.device_sched(0))
        time.sleep(0.001)


def _two_at_once(gpu, name_a, slots_a, name_b, slots_b, rounds, expect_gangs_on_b):
    gc.collect()
    base = _lib.device_sched(gpu)["contexts"]
    A, B = Rig(name_a, gpu, slots_a), Rig(name_b, gpu, slots_b)
    try:
        _lib.device_sched(gpu, reset=True)
        A.pk.paths(reset=True), B.pk.paths(reset=True)
        with Sampler(gpu) as sm:
            ca, cb = Callers(A, 32, rounds).start(), Callers(B, 32, rounds).start()
            ca.join(), cb.join()
        d = _lib.device_sched(gpu)
        pa, pb = A.pk.paths(), B.pk.paths()
        print("device:", d, "samples:", sm.samples, "\n%s:" % name_a, pa, "\n%s:" % name_b, pb)
        ca.check(A.want, name_a + " beside " + name_b, 32 * rounds)
        cb.check(B.want, name_b + " beside " + name_a, 32 * rounds)
        assert not sm.over, sm.over[:3]
        assert d["device_wide"] == 1 and d["max_streams"] == 16
        assert d["streams_peak"] <= d["max_streams"], d
        assert d["proofs_peak"] > d["max_streams"], d
        assert d["contexts"] - base == 2 and sm.contexts == {base + 2}, (d, base, sm.contexts)
        assert d["streams_in_use"] == 0 and d["proofs_in_flight"] == 0 and d["waiting"] == 0, d
        assert pa["proofs"] == 32 * rounds and pb["proofs"] == 32 * rounds
        if expect_gangs_on_b:
            assert pb["gang_proofs"] > 0, pb
        return ca.got, cb.got
    finally:
        A.close()
        B.close()


def test_two_curves_at_once(gpu):
    """BN254 2^17 (16 slots) and BLS12-381 2^14 (32 slots, gangs), 32 callers each, together."""
    _two_at_once(gpu, "bn254-17", 32, "bls12-381-14", 32, rounds=3, expect_gangs_on_b=True)


def test_two_bn254_circuits_of_different_size(gpu):
    """Several compiled circuits on one curve: 2^17 and 2^15 (the small one gangs)."""
    _two_at_once(gpu, "bn254-17", 32, "bn254-15", 32, rounds=3, expect_gangs_on_b=True)


def test_the_load_is_the_devices(gpu):
    """ONE proof on context A while context B saturates the GPU takes the loaded kernel forms - A's own busy count is 1, and before the
    device-wide scheduler it chose the latency forms (four lanes per point operation, a side stream for tail fill) against a full
    device.  With B idle the same context takes the lone forms again.  The bytes never change."""
    A, B = Rig("bn254-17", gpu, 16), Rig("bls12-381-14", gpu, 32)
    try:
        pr = _lib.Proof()
        check(A.ws.prove(2, pr, "device"))
        lone = _marshal(pr)
        assert lone == A.want[2]
        done = threading.Event()
        cb = Callers(B, 32, stop=done).start()
        try:
            _wait_for(lambda: _lib.device_sched(gpu)["proofs_in_flight"] >= 16 or cb.errors, "B to saturate the device")
            A.pk.paths(reset=True)
            check(A.ws.prove(2, pr, "device"))
            during = _lib.device_sched(gpu)
            p = A.pk.paths(reset=True)
        finally:
            done.set()              # B stops when A is done: an event, not timing luck
            cb.join()
        print("A beside a saturated B:", p, during)
        cb.check(B.want, "B while A proves")
        assert _marshal(pr) == lone
        assert p["proofs"] == 1
        assert p["ntt_radix4_by_load"] > 0 and p["msm_units_by_load"] > 0 and p["forms_by_device_load"] > 0, p
        assert p["tail_fill_proofs"] == 0, p
        # B idle: the lone forms, the same bytes
        _wait_for(lambda: _lib.device_sched(gpu)["proofs_in_flight"] == 0, "the device to go idle")
        check(A.ws.prove(2, pr, "device"))
        q = A.pk.paths(reset=True)
        print("A alone:", q)
        assert _marshal(pr) == lone
        assert q["tail_fill_proofs"] == 1 and q["forms_by_device_load"] == 0 and q["ntt_radix4_by_load"] == 0 and q["msm_units_by_load"] == 0, q
    finally:
        A.close()
        B.close()


def test_destroying_a_context_while_another_proves(gpu):
    gc.collect()
    base = _lib.device_sched(gpu)["contexts"]
    A, B = Rig("bn254-17", gpu, 16), Rig("bn254-15", gpu, 8)
    closed_a = False
    try:
        pr = _lib.Proof()
        check(B.ws.prove(1, pr, "device"))
        assert _marshal(pr) == B.want[1]
        assert _lib.device_sched(gpu)["contexts"] - base == 2
        ca = Callers(A, 16, 4).start()
        _wait_for(lambda: _lib.device_sched(gpu)["proofs_in_flight"] >= 8 or ca.errors, "A's callers to be in flight")
        in_flight = _lib.device_sched(gpu)["proofs_in_flight"]
        B.close()                                            # ... while A's 16 callers prove
        after = _lib.device_sched(gpu)
        ca.join()
        print("in flight at the destruction:", in_flight, "after:", after)
        assert after["contexts"] - base == 1, after
        ca.check(A.want, "A while B is destroyed", 16 * 4)
        # a further context afterwards: the device's streams are as they were
        D = Rig("bls12-381-14", gpu, 4)
        try:
            assert _lib.device_sched(gpu)["contexts"] - base == 2
            for a in range(K):
                check(D.ws.prove(a, pr, "device"))
                assert _marshal(pr) == D.want[a], a
            check(A.ws.prove(0, pr, "device"))
            assert _marshal(pr) == A.want[0]
        finally:
            D.close()
        A.close()
        closed_a = True
        assert _lib.device_sched(gpu)["contexts"] == base
    finally:
        if not closed_a:
            A.close()


def _child_main(out_path):
    """APK_DEVICE_SCHED=0 in a process of its own: the two curves at once on per-context pools; writes the blobs' digests."""
    gpu = 0
    d0 = _lib.device_sched(gpu)
    A, B = Rig("bn254-17", gpu, 32, oracle=False), Rig("bls12-381-14", gpu, 32, oracle=False)
    ca, cb = Callers(A, 32, 2).start(), Callers(B, 32, 2).start()
    ca.join(), cb.join()
    res = {"before": d0, "after": _lib.device_sched(gpu), "errors": [repr(e) for e in ca.errors + cb.errors],
           "a": sorted({(a, hashlib.sha256(b).hexdigest()) for a, b in ca.got}), "b": sorted({(a, hashlib.sha256(b).hexdigest()) for a, b in cb.got}),
           "proofs": [sum(ca.got.values()), sum(cb.got.values())], "gang_proofs_b": B.pk.paths()["gang_proofs"]}
    A.close()
    B.close()
    with open(out_path, "w") as f:
        json.dump(res, f)


def test_per_context_pools_give_the_same_bytes(gpu, tmp_path):
    """APK_DEVICE_SCHED=0 (read once per process, hence a child): the scheduler is off, the bytes are those of test_two_curves_at_once."""
    wa, wb = _host("bn254-17", gpu)["want"], _host("bls12-381-14", gpu)["want"]
    out = str(tmp_path / "child.json")
    env = dict(os.environ, APK_DEVICE_SCHED="0")
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = json.load(open(out))
    print({k: res[k] for k in ("before", "after", "proofs", "gang_proofs_b")})
    assert not res["errors"], res["errors"][:2]
    assert res["before"]["device_wide"] == 0 and res["after"]["device_wide"] == 0, res["after"]
    assert res["proofs"] == [64, 64]
    assert [tuple(x) for x in res["a"]] == sorted((a, hashlib.sha256(wa[a]).hexdigest()) for a in range(K))
    assert [tuple(x) for x in res["b"]] == sorted((a, hashlib.sha256(wb[a]).hexdigest()) for a in range(K))


if __name__ == "__main__":
    _child_main(sys.argv[1])

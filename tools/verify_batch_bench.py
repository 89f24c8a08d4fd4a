#!/usr/bin/env python3
"""Batch verification against what a service can do today: N sequential apk_verify calls on one thread (a), the same calls
spread over 16 host threads (b), one apk_verify_batch on the host (device = -1) and one on GPU 0.  Medians of `--runs` runs
after a warm-up call; one JSON line per point, written to profiles/verify_batch.json (the file is replaced).

    python tools/verify_batch_bench.py [--sizes 16,64,256,1024] [--runs 5] [--curves bn254,bls12-381] [--k 0,1] [--no-device]
                                       [--seq-max-n N]     (a) is linear in N and slow: not run above N proofs (null in the line)
    python tools/verify_batch_bench.py --split             one apk_verify cut into its parts, by proxy calls (see split())
    python tools/verify_batch_bench.py --load              prover throughput with and without a verifier batch beside it
    python tools/verify_batch_bench.py --one bls12-381,256 one device batch and nothing else (the program of a kernel-trace run)
    python tools/verify_batch_bench.py --keys [--keys-n 256] [--curves bls12-381] [--parent-lib path/to/libapk.so]
                                       N proofs over 4 keys of one SRS: four apk_verify_batch calls of N / 4 (through the library
                                       --parent-lib names, when given: an A/B against another build) against ONE
                                       apk_verify_batch_keys call of N, on GPU 0 and on the host, alternating; medians and spreads
    python tools/verify_batch_bench.py --one-keys bls12-381,256  one cross-circuit device batch and nothing else (kernel-trace run)

The proof material is the test-suite's (tests/verify_batch_material.py: oracle proofs of the reference's test circuits).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from algoplonk_amd import _lib                      # noqa: E402
from algoplonk_amd._lib import lib                  # noqa: E402
import verify_batch_material as vbm                 # noqa: E402


def median_ms(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def split(a):
    """One apk_verify (Pythagorean circuit, key checks cached) against proxies of its parts through the C-ABI, one thread
    (APK_VERIFY_THREADS=1 must be set by the caller): the 24 scalar multiplications of a k = 0 verification as one host
    apk_g1_lincomb_segments call of 24 full-width terms; the 9 subgroup checks (BLS12-381 only) as 9 terms with the scalar
    r - 1, which costs what [r]P costs; the rest (transcript, field work, the two-pair pairing) is the difference."""
    from oracle.prng import SplitMix64
    for cname in a.curves.split(","):
        m = vbm.material(cname, "pyth")
        cv, ov = m.cv, m.ov
        rv = m.vk.raw()
        raws, pubs, _ = m.take(1)
        buf = cv.fr_vector(pubs[0])
        g = SplitMix64(1)
        pts = [ov.mul(cv.g1, g.fr(cv.r)) for _ in range(24)]
        full = [g.fr(cv.r) | (1 << 250) for _ in range(24)]
        verify = median_ms(lambda: lib.apk_verify(C.byref(rv), C.byref(raws[0]), buf), 20)
        smul = median_ms(lambda: vbm.lincomb(cv, -1, pts, full, [0, 24]), 20)
        sub = median_ms(lambda: vbm.lincomb(cv, -1, pts[:9], [cv.r - 1] * 9, [0, 9]), 20) if cname != "bn254" else 0.0
        yield {"mode": "split", "curve": cname, "threads": os.environ.get("APK_VERIFY_THREADS"), "apk_verify_ms": verify,
               "scalar_mults_24_ms": smul, "subgroup_checks_9_ms": sub, "pairing_and_rest_ms": verify - smul - sub}


def load(a):
    """8 callers proving a BN254 2^13 circuit for a fixed time, alone and beside a thread that keeps verifying device batches
    of 32 of their proofs (the set-up of the GPU test, timed)."""
    import threading
    from algoplonk_amd import batch, ecc, plonk as ap_plonk, setup as ap_setup, workloads
    cv = ecc.BN254
    wl = workloads.random_circuit(cv, 13, 0xA190)
    srs = ap_setup.unsafe_srs(cv, wl.ccs.domain_size(), wl.tau, device=0)
    T, K, secs = 8, 32, 4.0
    pk, vk = ap_plonk.Setup(wl.ccs, srs, device=0, slots=T)
    ws = batch.WitnessSet(pk, wl.ccs, workloads.variants(wl, K, 0xA190)).to_device()
    proofs = []
    for i in range(K):
        pr = _lib.Proof()
        assert ws.prove(i, pr, "device") == 0
        proofs.append(pr)
    assert ws.verify_all(proofs, vk, 0) == [True] * K

    def run(with_verifier):
        stop, counts, batches = threading.Event(), [0] * T, [0]

        def prover(i):
            pr = _lib.Proof()
            r = 0
            while not stop.is_set():
                assert ws.prove((i + r) % K, pr, "device") == 0
                counts[i] += 1
                r += 1

        def verifier():
            while not stop.is_set():
                assert ws.verify_all(proofs, vk, 0) == [True] * K
                batches[0] += 1

        th = [threading.Thread(target=prover, args=(i,)) for i in range(T)] + ([threading.Thread(target=verifier)] if with_verifier else [])
        t0 = time.perf_counter()
        [t.start() for t in th]
        time.sleep(secs)
        stop.set()
        [t.join() for t in th]
        dt = time.perf_counter() - t0
        return sum(counts) / dt, batches[0] / dt

    run(False)
    for rep in range(3):
        alone, _ = run(False)
        beside, bps = run(True)
        yield {"mode": "load", "curve": "bn254", "log_n": 13, "provers": T, "proofs_per_s_alone": alone, "proofs_per_s_beside_verifier": beside,
               "verifier_batches_of_32_per_s": bps}
    ws.close()
    pk.close()


def keys_material(cname, n):
    """n proofs over 4 circuits of one SRS (k = 0, 0, 1, 2), interleaved: -> (materials, key_of, raws, pubs)"""
    import verify_keys_material as vkm
    mats = [vbm.material(cname, c) for c in ("pyth", "id", "bsb1", "bsb2")]
    key_of, raws, pubs, _ = vkm.interleave(mats, n // 4)
    return mats, key_of, raws, pubs


def keys(a):
    """Cross-circuit against per-circuit: the same N proofs as four apk_verify_batch calls (one per key, N / 4 proofs each) and as one
    apk_verify_batch_keys call - three pairings and three launch sequences fewer.  The forms alternate run by run."""
    import verify_keys_material as vkm
    parent = C.CDLL(a.parent_lib) if a.parent_lib else lib
    if a.parent_lib:
        parent.apk_verify_batch.argtypes = lib.apk_verify_batch.argtypes
    for cname in a.curves.split(","):
        mats, key_of, raws, pubs = keys_material(cname, a.keys_n)
        vks = [m.vk for m in mats]
        per_key = [[j for j in range(len(raws)) if key_of[j] == i] for i in range(4)]

        def four_calls(dev):
            for i, sel in enumerate(per_key):
                n = len(sel)
                arr = (_lib.Proof * n)(*[raws[j] for j in sel])
                bufs = [mats[i].cv.fr_vector(pubs[j]) for j in sel]
                ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bufs])
                nbs = (C.c_uint32 * n)(*[len(pubs[j]) for j in sel])
                status = (C.c_int * n)()
                rv = vks[i].raw()
                assert parent.apk_verify_batch(dev, C.byref(rv), arr, ptrs, nbs, n, status, None) == 0

        def one_call(dev):
            rc, st, tr = vkm.run_keys(vks, key_of, raws, pubs, device=dev)
            assert rc == 0 and tr.groups == 1 and tr.folds == 1

        devices = ([0] if not a.no_device and _lib.device_count() > 0 else []) + [-1]
        for dev in devices:
            four_calls(dev); one_call(dev)                      # warm-up: key checks cached, device buffers pooled
            ts = {"four_calls": [], "one_call": []}
            for _ in range(a.runs):
                for name, fn in (("four_calls", four_calls), ("one_call", one_call)):
                    t0 = time.perf_counter()
                    fn(dev)
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            line = {"mode": "keys", "curve": cname, "n_proofs": a.keys_n, "keys": 4, "device": dev, "runs": a.runs,
                    "four_calls_through": a.parent_lib or "this library"}
            for name, v in ts.items():
                line[name + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            yield line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,64,256,1024")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--curves", default="bn254,bls12-381")
    ap.add_argument("--k", default="0,1")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch.json"))
    ap.add_argument("--seq-max-n", type=int, default=1 << 30)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--load", action="store_true")
    ap.add_argument("--one", default="")
    ap.add_argument("--keys", action="store_true")
    ap.add_argument("--keys-n", type=int, default=256)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--one-keys", default="")
    a = ap.parse_args()
    device = not a.no_device and _lib.device_count() > 0
    if a.one:
        cname, n = a.one.split(",")
        m = vbm.material(cname, "pyth")
        raws, pubs, _ = m.take(int(n))
        for _ in range(2):
            rc, st, tr = vbm.run_batch(m.vk, raws, pubs, device=0)
            assert rc == 0 and tr.folds == 1
        return
    if a.one_keys:
        import verify_keys_material as vkm
        cname, n = a.one_keys.split(",")
        mats, key_of, raws, pubs = keys_material(cname, int(n))
        for _ in range(2):
            rc, st, tr = vkm.run_keys([m.vk for m in mats], key_of, raws, pubs, device=0)
            assert rc == 0 and tr.folds == 1
        return
    if a.split or a.load or a.keys:
        with open(a.out, "w") as out:
            for line in (split(a) if a.split else load(a) if a.load else keys(a)):
                print(json.dumps(line), flush=True)
                out.write(json.dumps(line) + "\n")
        return
    with open(a.out, "w") as out:
        for cname in a.curves.split(","):
            for k in (int(x) for x in a.k.split(",")):
                m = vbm.material(cname, "pyth" if k == 0 else "bsb%d" % k)
                rv = m.vk.raw()
                for n in (int(x) for x in a.sizes.split(",")):
                    raws, pubs, _ = m.take(n)
                    bufs = [m.cv.fr_vector(p) for p in pubs]

                    def one(j):
                        assert lib.apk_verify(C.byref(rv), C.byref(raws[j]), bufs[j]) == 0

                    def threaded():
                        with ThreadPoolExecutor(16) as ex:
                            list(ex.map(one, range(n)))

                    def batched(dev):
                        rc, st, tr = vbm.run_batch(m.vk, raws, pubs, device=dev)
                        assert rc == 0 and tr.folds == 1

                    line = {"curve": cname, "k": k, "n_proofs": n, "runs": a.runs,
                            "sequential_ms": median_ms(lambda: [one(j) for j in range(n)], a.runs) if n <= a.seq_max_n else None,
                            "threads16_ms": median_ms(threaded, a.runs),
                            "batch_host_ms": median_ms(lambda: batched(-1), a.runs),
                            "batch_device_ms": median_ms(lambda: batched(0), a.runs) if device else None}
                    print(json.dumps(line), flush=True)
                    out.write(json.dumps(line) + "\n")
                    out.flush()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Two contexts on one GPU, measured: does the device-wide scheduler (csrc/device_sched.h) pay, and does one context pay for it?

    python tools/two_contexts_bench.py --other-lib ab/parent/libapk.so --repeats 3 --out profiles/two_contexts_ab.txt

Two legs, alternating, every run in a process of its own (APK_LIB is read when the package is imported): "this" = the in-tree
libapk.so, "other" = --other-lib (a build of the parent commit) or, without it, the in-tree library with APK_DEVICE_SCHED=0.
Every run times, with a warm-up each, for --seconds each:
  (a) BN254 2^17 alone, 32 callers            (b) BLS12-381 2^14 alone, 32 callers
  (c) both at once, 32 callers each: proofs/s per context and the aggregate share  p_A / solo_A + p_B / solo_B
  (l) the latency of a lone BN254 2^17 proof (median of 15)
Only the library runs inside the timed regions (distinct assignments per caller, resident on the device); afterwards every blob
made is held to the C oracle's proof of its own inputs (the first run computes the digests, the others compare with them).
With several repeats per leg the spread of a leg against itself is known, and the verdict uses it:
  pass = (c)'s share on "this" is not below "other" by more than the spread, and (a), (b), (l) are within the spread of "other".
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")

K = 6
SPECS = {"A": ("bn254", 17, 0x2C0A), "B": ("bls12-381", 14, 0x2C0B)}


def run_once(args):
    from algoplonk_amd import _lib, batch, plonk as ap_plonk, setup as ap_setup, workloads
    from algoplonk_amd._lib import lib, check
    from helpers import CURVES, oracle_threads

    def marshal(pr):
        out = C.create_string_buffer(2048)
        ln = C.c_size_t(0)
        check(lib.apk_marshal_proof(C.byref(pr), out, 2048, C.byref(ln)))
        return out.raw[: ln.value]

    rigs = {}
    for name, (cname, log_n, seed) in SPECS.items():
        cv, _ = CURVES[cname]
        wl = workloads.random_circuit(cv, log_n, seed)
        srs = ap_setup.unsafe_srs(cv, wl.ccs.domain_size(), wl.tau, device=0)
        pk, _vk = ap_plonk.Setup(wl.ccs, srs, device=0, slots=32)
        ws = batch.WitnessSet(pk, wl.ccs, workloads.variants(wl, K, seed)).to_device()
        rigs[name] = dict(cv=cv, wl=wl, srs=srs, pk=pk, ws=ws, seen=set())

    def timed(names, seconds):
        """32 callers per named context for `seconds`; proofs/s per context, counted between the first and the last barrier."""
        stop, counts, errors, lock = threading.Event(), {n: 0 for n in names}, [], threading.Lock()
        t_open = [None]

        def work(name, i):
            rig, pr, r = rigs[name], _lib.Proof(), 0
            while not stop.is_set():
                a = (i + 3 * r) % K
                rc = rig["ws"].prove(a, pr, "device")
                if rc != 0:
                    errors.append((name, rc, lib.apk_last_error()))
                    return
                blob = marshal(pr)
                with lock:
                    rig["seen"].add((a, blob))
                    if t_open[0] is not None:
                        counts[name] += 1
                r += 1

        th = [threading.Thread(target=work, args=(n, i)) for n in names for i in range(32)]
        [t.start() for t in th]
        time.sleep(args.warmup)
        with lock:
            t_open[0] = t0 = time.perf_counter()
        time.sleep(seconds)
        with lock:
            t1 = time.perf_counter()
            got = dict(counts)
            t_open[0] = None
        stop.set()
        [t.join() for t in th]
        if errors:
            raise RuntimeError(errors[0])
        return {n: got[n] / (t1 - t0) for n in names}

    res = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "env": {k: v for k, v in sorted(os.environ.items()) if k.startswith("APK_") and k != "APK_LIB"}}
    pr = _lib.Proof()
    lat = []
    for i in range(20):
        t0 = time.perf_counter()
        check(rigs["A"]["ws"].prove(i % K, pr, "device"))
        lat.append((time.perf_counter() - t0) * 1e3)
        rigs["A"]["seen"].add((i % K, marshal(pr)))
    res["proof_latency_ms"] = statistics.median(lat[5:])
    res["solo_A"] = timed(["A"], args.seconds)["A"]
    res["solo_B"] = timed(["B"], args.seconds)["B"]
    both = timed(["A", "B"], args.seconds)
    res["both_A"], res["both_B"] = both["A"], both["B"]
    res["share"] = both["A"] / res["solo_A"] + both["B"] / res["solo_B"]
    res["paths_A"], res["paths_B"] = rigs["A"]["pk"].paths(), rigs["B"]["pk"].paths()
    try:
        res["device_sched"] = _lib.device_sched(0)
    except Exception as e:        # (a library from before the scheduler)
        res["device_sched"] = str(e)
    # ---- after the timed regions: every blob against the C oracle's proof of the same inputs
    digests = {n: sorted({(a, hashlib.sha256(b).hexdigest()) for a, b in rigs[n]["seen"]}) for n in rigs}
    if args.oracle_file and os.path.exists(args.oracle_file):
        want = json.load(open(args.oracle_file))
    else:
        from bench_cpu import oracle_blobs
        want = {}
        for n, rig in rigs.items():
            blobs = oracle_blobs(rig["cv"], rig["wl"].ccs, rig["srs"], rig["ws"].items, threads=oracle_threads())
            want[n] = [[a, hashlib.sha256(blobs[a]).hexdigest()] for a in range(K)]
        if args.oracle_file:
            json.dump(want, open(args.oracle_file, "w"))
    for n in rigs:
        if [list(x) for x in digests[n]] != want[n]:
            raise RuntimeError("context %s: blobs differ from the C oracle's: %s" % (n, digests[n][:3]))
    res["oracle_checked_blobs"] = sum(len(d) for d in digests.values())
    for rig in rigs.values():
        rig["ws"].close()
        rig["pk"].close()
    print("RESULT " + json.dumps(res), flush=True)


METRICS = ["solo_A", "solo_B", "both_A", "both_B", "share", "proof_latency_ms"]


def drive(args):
    legs = [("this", {})]
    legs.append(("other", {"APK_LIB": os.path.abspath(args.other_lib)}) if args.other_lib else ("other", {"APK_DEVICE_SCHED": "0"}))
    oracle_file = os.path.join(args.scratch, "two_contexts_oracle.json")
    os.makedirs(args.scratch, exist_ok=True)
    if os.path.exists(oracle_file):
        os.remove(oracle_file)
    runs = {"this": [], "other": []}
    lines = []
    for rep in range(args.repeats):
        for leg, env in (legs if rep % 2 == 0 else legs[::-1]):
            cmd = ["timeout", "-k", "10", str(args.run_timeout), sys.executable, os.path.abspath(__file__), "--run", "--seconds", str(args.seconds),
                   "--warmup", str(args.warmup), "--oracle-file", oracle_file]
            r = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, cwd=ROOT)
            if r.returncode != 0:         # nothing more is started on the GPU after a failed run
                sys.stderr.write(r.stdout[-3000:] + r.stderr[-5000:])
                raise SystemExit("run %d of leg %s ended with status %d" % (rep, leg, r.returncode))
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs[leg].append(res)
            line = "%-5s rep %d  " % (leg, rep) + "  ".join("%s %.2f" % (m, res[m]) for m in METRICS)
            print(line, flush=True)
            lines.append(line)
    out = ["two contexts on one GPU: BN254 2^17 (A) and BLS12-381 2^14 (B), 32 callers each; %d repeats per leg, %.0f s per timed region" % (args.repeats, args.seconds),
           "this  = %s %s" % (runs["this"][0]["lib"], runs["this"][0]["env"]),
           "other = %s %s" % (runs["other"][0]["lib"], runs["other"][0]["env"]), ""] + lines + [""]
    med = {leg: {m: statistics.median(r[m] for r in runs[leg]) for m in METRICS} for leg in runs}
    spread = {}
    for m in METRICS:      # the widest distance of a leg's run from its own median, relative: what one leg measures against itself
        spread[m] = max(abs(r[m] - med[leg][m]) / med[leg][m] for leg in runs for r in runs[leg])
        out.append("%-17s this %9.2f   other %9.2f   delta %+6.2f %%   spread of a leg against itself %5.2f %%" %
                   (m, med["this"][m], med["other"][m], 100 * (med["this"][m] / med["other"][m] - 1), 100 * spread[m]))
    ok_share = med["this"]["share"] >= med["other"]["share"] * (1 - spread["share"])
    ok_solo = all(abs(med["this"][m] / med["other"][m] - 1) <= spread[m] for m in ("solo_A", "solo_B", "proof_latency_ms"))
    out += ["", "aggregate share with both at once: %s" % ("not below the other leg beyond the spread" if ok_share else "BELOW the other leg"),
            "one context alone (a), (b), lone latency: %s" % ("within the spread of the other leg" if ok_solo else "OUTSIDE the spread of the other leg"),
            "verdict: %s" % ("pass" if ok_share and ok_solo else "FAIL"), "",
            "this leg, last run: device_sched %s" % runs["this"][-1]["device_sched"],
            "  paths A %s" % runs["this"][-1]["paths_A"], "  paths B %s" % runs["this"][-1]["paths_B"],
            "other leg, last run:", "  paths A %s" % runs["other"][-1]["paths_A"], "  paths B %s" % runs["other"][-1]["paths_B"]]
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return 0 if ok_share and ok_solo else 3


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="one measuring run in this process (what the driver starts)")
    ap.add_argument("--other-lib", default="", help="libapk.so of the other leg (default: this library with APK_DEVICE_SCHED=0)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--warmup", type=float, default=1.0)
    ap.add_argument("--run-timeout", type=int, default=420)
    ap.add_argument("--oracle-file", default="")
    ap.add_argument("--scratch", default=os.path.join(ROOT, "out"))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.run:
        run_once(a)
    else:
        sys.exit(drive(a))

#!/usr/bin/env python3
"""What an opening costs on top of the MSM of its quotient: the median wall time of apk_kzg_open_device(len = n + 2) against the
median of apk_msm_g1_device over the same length, on the same MSM-only context (n + 3 bases of a known-tau SRS), alone on the
device.  The difference is evaluate + divide (three launches of kernels_kzg.h and the value's copy).

    python tools/kzg_probe.py [--calls 50] [--device 0] [--leg both|canonical|lagrange|multi|multi-lagrange|all|cosets|cosets-verify|recover|cosets-multi]

A second leg does the same for the opening in evaluation form, on a circuit context of n rows: the median of
apk_kzg_open_lagrange_device (kernels_kzg_lagrange.h) against the median of apk_msm_g1_device(basis 1, n) on the same context and
run, and against the route a caller had before: apk_ntt(inverse) through host memory, then apk_kzg_open of the coefficients.

A third leg (--leg multi; not part of `both`) sets apk_kzg_open_multi_device against the per-pair route: the median of the call
with count = 4 and with count = 32, one polynomial of n + 2 coefficients at distinct points, against count x the median of
apk_kzg_open_device taken in the same run - on the MSM-only context of n + 3 bases (its workspace takes one MSM per launch
sequence: groups of one) and on a circuit context of n rows (groups of four).

A fourth leg (--leg multi-lagrange; not part of `both`) does the same in evaluation form on the circuit contexts:
apk_kzg_open_multi_lagrange_device with count = 4 and count = 32, ONE vector of n values at distinct points, against count x the
median of apk_kzg_open_lagrange_device taken in the same run.

A fifth leg (--leg all; not part of `both`) times apk_kzg_open_all_device - one polynomial of n coefficients opened at every point
of its domain - on circuit contexts: the median of a few calls (at most 5: a call is long) for each stage form, the two forms
on two contexts side by side with their calls alternating (APK_KZG_ALL_GLV is read at apk_kzg_all_prepare), apk_kzg_all_prepare
once each, against the route a caller had before: (n / 32) x the median of apk_kzg_open_multi_device(count = 32) in the same run.

A sixth leg (--leg cosets; not part of `both`) times apk_kzg_open_cosets_device - one polynomial of n coefficients opened on every
coset of l = 64 points - on circuit contexts: the median of 5 calls after one warm-up and apk_kzg_cosets_prepare once, against the
route a caller had before, in the same run: the median of apk_kzg_open_all_device plus the median of
apk_g1_lincomb_segments(device) over the n single-point proofs with the weights x_(i,j) / (l a_i) - which must give the call's own
bytes.  The line also carries the table's bytes in device memory.

A seventh leg (--leg cosets-verify; not part of `both`) is the consuming side: the n / l rows of one apk_kzg_open_cosets_device call
(l = 64) through apk_kzg_batch_verify_cosets, the median of 5 calls with the device and with device -1, each with the split
apk_kzg_cosets_phase_ms reports (key, SRS and scalar checks; point checks; hashing; fold; segmented sum; pairing), against the route a
caller had before: the median single call of apk_kzg_verify_coset over 16 rows times the number of rows - EXTRAPOLATED, and said so
in the line.

An eighth leg (--leg recover; not part of `both`) is the middle: apk_kzg_recover_cosets_device on half of the n / l cells (l = 64,
dropped at random from a fixed seed) of a polynomial of n / 2 coefficients that apk_kzg_open_cosets_device opened - the result must
be that polynomial - the median of 5 calls after one warm-up.  Beside it, in the same run: three size-n transforms through apk_ntt
(forward, inverse, inverse: code the recovery did not touch; each call carries the vector through host memory both ways, and the
line says so), the event-timed milliseconds of the three transforms INSIDE one more recovery call with the context's statistics on,
and the same recovery with no cell dropped (m = 0: no roots, a vanish kernel with no product) - the difference of the two medians
is what the roots and the vanish kernel cost, an estimate by difference, not a profile.

A ninth leg (--leg cosets-multi; not part of `both`) is the producing side for many polynomials: apk_kzg_open_cosets_multi_device on
`count` random polynomials of n coefficients in device memory (l = 64, --counts, default 1,2,4,8,16,32), the median of 5 calls after
one warm-up, against count x the median of apk_kzg_open_cosets_device taken in the same run on the same context - and the two must
give the same bytes, polynomial by polynomial.  One line per context and count; the ratio multi / (count x single) is what the call
is for.  (--counts 16 --calls 1 is the run a kernel trace is taken of.)

One JSON line per leg and configuration: BN254 2^17 and BLS12-381 2^14 (the sizes of DESIGN.md's tables)."""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from algoplonk_amd import ecc, kzg, plonk, setup, workloads  # noqa: E402
from algoplonk_amd._lib import check, lib  # noqa: E402
from oracle.prng import SplitMix64, tau_from_seed  # noqa: E402


def timed(fn, calls: int) -> float:
    for _ in range(5):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def probe_lagrange(cv, log_n: int, calls: int, device: int) -> dict:
    n, r = 1 << log_n, cv.r
    wl = workloads.random_circuit(cv, log_n, 0x9B0D)
    srs = setup.unsafe_srs(cv, n, wl.tau, device=device)
    pk, _ = plonk.Setup(wl.ccs, srs, device=device)
    ctx = pk.ctx
    g = SplitMix64(0x9B0E)
    f = [g.fr(r) for _ in range(n)]
    z = g.fr(r)
    buf = cv.fr_vector(f)
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    h, v, out = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32), C.create_string_buffer(2 * cv.fp_bytes)
    h2, v2 = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    zb = cv.fr_vector([z])
    # checked once: the route through the coefficients gives the same bytes
    work = C.create_string_buffer(buf, len(buf))
    check(lib.apk_ntt(ctx, 0, 1, 0, work))
    check(lib.apk_kzg_open(ctx, work, n, zb, h2, v2))
    check(lib.apk_kzg_open_lagrange_device(ctx, d, n, zb, h, v))
    assert (h.raw, v.raw) == (h2.raw, v2.raw), "the opening in evaluation form differs from the opening of the coefficients"

    def route_today():      # (the transform is in place: the buffer's contents change from call to call, the work does not)
        check(lib.apk_ntt(ctx, 0, 1, 0, work))
        check(lib.apk_kzg_open(ctx, work, n, zb, h2, v2))

    msm_ms = timed(lambda: check(lib.apk_msm_g1_device(ctx, 1, d, n, out)), calls)
    open_ms = timed(lambda: check(lib.apk_kzg_open_lagrange_device(ctx, d, n, zb, h, v)), calls)
    today_ms = timed(route_today, calls)
    check(lib.apk_device_free(ctx, d))
    pk.close()
    return {"leg": "lagrange", "curve": cv.name, "log_n": log_n, "len": n, "calls": calls, "msm_basis1_ms": round(msm_ms, 4),
            "open_lagrange_ms": round(open_ms, 4), "ntt_then_open_ms": round(today_ms, 4), "ratio_to_msm": round(open_ms / msm_ms, 4),
            "ratio_to_ntt_then_open": round(open_ms / today_ms, 4)}


def probe(cv, log_n: int, calls: int, device: int) -> dict:
    n, r = 1 << log_n, cv.r
    tau = tau_from_seed(0x9B0B, r)
    srs = setup.unsafe_srs(cv, n, tau, device=device)
    ctx = kzg.MsmContext(cv, srs.g1, device=device)
    g = SplitMix64(0x9B0C)
    L = n + 2
    f = [g.fr(r) for _ in range(L)]
    z = g.fr(r)
    buf = cv.fr_vector(f)
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx.ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx.ctx, d, buf, len(buf)))
    h, v, out = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32), C.create_string_buffer(2 * cv.fp_bytes)
    zb = cv.fr_vector([z])

    msm_ms = timed(lambda: check(lib.apk_msm_g1_device(ctx.ctx, 0, d, L, out)), calls)
    open_ms = timed(lambda: check(lib.apk_kzg_open_device(ctx.ctx, d, L, zb, h, v)), calls)
    # the opening is checked once: value by Horner, H by the known-tau rule
    acc = 0
    for c in reversed(f):
        acc = (acc * z + c) % r
    assert cv.fr_from_mont_bytes(v.raw) == acc, "f(z) differs from Horner"
    check(lib.apk_device_free(ctx.ctx, d))
    ctx.close()
    return {"leg": "canonical", "curve": cv.name, "log_n": log_n, "len": L, "calls": calls, "msm_ms": round(msm_ms, 4), "open_ms": round(open_ms, 4),
            "evaluate_divide_ms": round(open_ms - msm_ms, 4), "ratio": round(open_ms / msm_ms, 4)}


def probe_multi(cv, log_n: int, calls: int, device: int, context: str) -> dict:
    n, r = 1 << log_n, cv.r
    if context == "msm-only":
        srs = setup.unsafe_srs(cv, n, tau_from_seed(0x9B0B, r), device=device)
        key = kzg.MsmContext(cv, srs.g1, device=device)
    else:
        wl = workloads.random_circuit(cv, log_n, 0x9B0D)
        srs = setup.unsafe_srs(cv, n, wl.tau, device=device)
        key, _ = plonk.Setup(wl.ccs, srs, device=device)
    ctx = key.ctx
    g = SplitMix64(0x9B0F)
    L = n + 2
    f = [g.fr(r) for _ in range(L)]
    zs = [g.fr(r) for _ in range(32)]
    buf = cv.fr_vector(f)
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    w = 2 * cv.fp_bytes
    h1, v1 = C.create_string_buffer(w), C.create_string_buffer(32)
    h, v = C.create_string_buffer(32 * w), C.create_string_buffer(32 * 32)
    zb = cv.fr_vector(zs)
    ptrs, lens = (C.c_void_p * 32)(*[d.value] * 32), (C.c_uint64 * 32)(*[L] * 32)
    # checked once: the 32 openings are the 32 single openings
    check(lib.apk_kzg_open_multi_device(ctx, 32, ptrs, lens, zb, h, v))
    for i in range(32):
        check(lib.apk_kzg_open_device(ctx, d, L, zb[32 * i:32 * (i + 1)], h1, v1))
        assert (h.raw[i * w:(i + 1) * w], v.raw[32 * i:32 * (i + 1)]) == (h1.raw, v1.raw), "opening %d differs from apk_kzg_open_device" % i
    single_ms = timed(lambda: check(lib.apk_kzg_open_device(ctx, d, L, zb[:32], h1, v1)), calls)
    out = {"leg": "multi", "context": context, "curve": cv.name, "log_n": log_n, "len": L, "calls": calls, "single_open_ms": round(single_ms, 4)}
    for count in (4, 32):
        ms = timed(lambda: check(lib.apk_kzg_open_multi_device(ctx, count, ptrs, lens, zb, h, v)), calls)
        out["multi_%d_ms" % count] = round(ms, 4)
        out["per_opening_%d_ms" % count] = round(ms / count, 4)
        out["ratio_%d" % count] = round(ms / (count * single_ms), 4)      # against count single openings
    check(lib.apk_device_free(ctx, d))
    key.close()
    return out


def probe_multi_lagrange(cv, log_n: int, calls: int, device: int) -> dict:
    n, r = 1 << log_n, cv.r
    wl = workloads.random_circuit(cv, log_n, 0x9B0D)
    srs = setup.unsafe_srs(cv, n, wl.tau, device=device)
    key, _ = plonk.Setup(wl.ccs, srs, device=device)
    ctx = key.ctx
    g = SplitMix64(0x9B10)
    f = [g.fr(r) for _ in range(n)]
    zs = [g.fr(r) for _ in range(32)]
    buf = cv.fr_vector(f)
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    w = 2 * cv.fp_bytes
    h1, v1 = C.create_string_buffer(w), C.create_string_buffer(32)
    h, v = C.create_string_buffer(32 * w), C.create_string_buffer(32 * 32)
    zb = cv.fr_vector(zs)
    ptrs = (C.c_void_p * 32)(*[d.value] * 32)
    # checked once: the 32 openings are the 32 single openings
    check(lib.apk_kzg_open_multi_lagrange_device(ctx, 32, ptrs, zb, h, v))
    for i in range(32):
        check(lib.apk_kzg_open_lagrange_device(ctx, d, n, zb[32 * i:32 * (i + 1)], h1, v1))
        assert (h.raw[i * w:(i + 1) * w], v.raw[32 * i:32 * (i + 1)]) == (h1.raw, v1.raw), "opening %d differs from apk_kzg_open_lagrange_device" % i
    single_ms = timed(lambda: check(lib.apk_kzg_open_lagrange_device(ctx, d, n, zb[:32], h1, v1)), calls)
    out = {"leg": "multi-lagrange", "context": "circuit", "curve": cv.name, "log_n": log_n, "len": n, "calls": calls,
           "single_open_lagrange_ms": round(single_ms, 4)}
    for count in (4, 32):
        ms = timed(lambda: check(lib.apk_kzg_open_multi_lagrange_device(ctx, count, ptrs, zb, h, v)), calls)
        out["multi_%d_ms" % count] = round(ms, 4)
        out["per_opening_%d_ms" % count] = round(ms / count, 4)
        out["ratio_%d" % count] = round(ms / (count * single_ms), 4)      # against count single openings
    check(lib.apk_device_free(ctx, d))
    key.close()
    return out


def probe_all(cv, log_n: int, calls: int, device: int) -> dict:
    n, r = 1 << log_n, cv.r
    wl = workloads.random_circuit(cv, log_n, 0x9B0D)
    srs = setup.unsafe_srs(cv, n, wl.tau, device=device)
    g = SplitMix64(0x9B11)
    f = [g.fr(r) for _ in range(n)]
    buf = cv.fr_vector(f)
    w = 2 * cv.fp_bytes
    # one context per stage form (the knob is read at apk_kzg_all_prepare), side by side: their calls alternate below
    keys, d, prepare_ms = {}, {}, {}
    before = os.environ.get("APK_KZG_ALL_GLV")
    for form in ("glv", "plain"):
        os.environ["APK_KZG_ALL_GLV"] = "1" if form == "glv" else "0"
        keys[form], _ = plonk.Setup(wl.ccs, srs, device=device)
        t0 = time.perf_counter()
        check(lib.apk_kzg_all_prepare(keys[form].ctx, srs.g1, n + 3))
        prepare_ms[form] = (time.perf_counter() - t0) * 1e3
        d[form] = C.c_void_p()
        check(lib.apk_device_alloc(keys[form].ctx, len(buf), C.byref(d[form])))
        check(lib.apk_device_upload(keys[form].ctx, d[form], buf, len(buf)))
    if before is None:
        os.environ.pop("APK_KZG_ALL_GLV", None)
    else:
        os.environ["APK_KZG_ALL_GLV"] = before
    h = {form: C.create_string_buffer(w * n) for form in keys}
    v = {form: C.create_string_buffer(32 * n) for form in keys}
    ms = {form: [] for form in keys}
    for i in range(calls + 1):      # (the first pair warms up: scratch allocation, code load)
        for form in ("glv", "plain"):
            t0 = time.perf_counter()
            check(lib.apk_kzg_open_all_device(keys[form].ctx, d[form], n, h[form], v[form]))
            if i:
                ms[form].append((time.perf_counter() - t0) * 1e3)
    assert h["glv"].raw == h["plain"].raw and v["glv"].raw == v["plain"].raw, "the two stage forms differ"
    # the reference: 32 openings through apk_kzg_open_multi_device, at 32 points of the domain - checked against the call's own
    ctx = keys["glv"].ctx
    om = cv.omega(n)
    idx = [0, 1, n // 2, n - 1] + [2 + g.below(n // 2 - 2) for _ in range(28)]
    zb = cv.fr_vector([pow(om, i, r) for i in idx])
    ptrs, lens = (C.c_void_p * 32)(*[d["glv"].value] * 32), (C.c_uint64 * 32)(*[n] * 32)
    mh, mv = C.create_string_buffer(32 * w), C.create_string_buffer(32 * 32)
    check(lib.apk_kzg_open_multi_device(ctx, 32, ptrs, lens, zb, mh, mv))
    for k, i in enumerate(idx):
        assert (mh.raw[k * w:(k + 1) * w], mv.raw[32 * k:32 * (k + 1)]) == (h["glv"].raw[i * w:(i + 1) * w], v["glv"].raw[32 * i:32 * (i + 1)]), "opening %d differs from apk_kzg_open_multi_device" % i
    multi_ms = timed(lambda: check(lib.apk_kzg_open_multi_device(ctx, 32, ptrs, lens, zb, mh, mv)), 20)
    for form in keys:
        check(lib.apk_device_free(keys[form].ctx, d[form]))
        keys[form].close()
    ref = n / 32 * multi_ms
    out = {"leg": "all", "curve": cv.name, "log_n": log_n, "len": n, "calls": calls, "multi_32_ms": round(multi_ms, 4), "multi_calls": 20,
           "reference_ms": round(ref, 1)}
    for form in ("glv", "plain"):
        med = statistics.median(ms[form])
        out["open_all_%s_ms" % form] = round(med, 3)
        out["prepare_%s_ms" % form] = round(prepare_ms[form], 3)
        out["ratio_%s" % form] = round(med / ref, 5)
    return out


def probe_cosets(cv, log_n: int, calls: int, device: int, l: int = 64) -> dict:
    n, r = 1 << log_n, cv.r
    np = n // l
    wl = workloads.random_circuit(cv, log_n, 0x9B0D)
    srs = setup.unsafe_srs(cv, n, wl.tau, device=device)
    g = SplitMix64(0x9B12)
    f = [g.fr(r) for _ in range(n)]
    buf = cv.fr_vector(f)
    w = 2 * cv.fp_bytes
    key, _ = plonk.Setup(wl.ccs, srs, device=device)
    ctx = key.ctx
    t0 = time.perf_counter()
    check(lib.apk_kzg_cosets_prepare(ctx, srs.g1, n + 3, l))
    prepare_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    check(lib.apk_kzg_all_prepare(ctx, srs.g1, n + 3))
    prepare_all_ms = (time.perf_counter() - t0) * 1e3
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    h, v = C.create_string_buffer(w * np), C.create_string_buffer(32 * n)
    h1, v1 = C.create_string_buffer(w * n), C.create_string_buffer(32 * n)
    ms, all_ms = [], []
    for i in range(calls + 1):      # (the first pair warms up: scratch allocation, code load)
        t0 = time.perf_counter()
        check(lib.apk_kzg_open_cosets_device(ctx, d, n, h, v))
        t1 = time.perf_counter()
        check(lib.apk_kzg_open_all_device(ctx, d, n, h1, v1))
        t2 = time.perf_counter()
        if i:
            ms.append((t1 - t0) * 1e3)
            all_ms.append((t2 - t1) * 1e3)
    # the reference's second half: H_i = sum_j x_(i,j) / (l a_i) H1_(i + n' j), one segment per coset
    om = cv.omega(n)
    pw = [1] * n
    for k in range(1, n):
        pw[k] = pw[k - 1] * om % r
    l_inv = pow(l, -1, r)
    weights = [pw[(i + np * j) % n] * pw[(-i * l) % n] % r * l_inv % r for i in range(np) for j in range(l)]
    raw = h1.raw
    pts = b"".join(raw[(i + np * j) * w:(i + np * j + 1) * w] for i in range(np) for j in range(l))
    wb = cv.fr_vector(weights)
    seg = (C.c_uint64 * (np + 1))(*[i * l for i in range(np + 1)])
    out = C.create_string_buffer(w * np)
    check(lib.apk_g1_lincomb_segments(cv.abi, device, pts, wb, seg, np, out))
    assert out.raw == h.raw, "the composition of the single-point proofs differs from the coset proofs"
    assert v.raw == b"".join(v1.raw[32 * (i + np * j):32 * (i + np * j + 1)] for i in range(np) for j in range(l)), "the values differ"
    fold_ms = timed(lambda: check(lib.apk_g1_lincomb_segments(cv.abi, device, pts, wb, seg, np, out)), calls)
    check(lib.apk_device_free(ctx, d))
    key.close()
    med, ref = statistics.median(ms), statistics.median(all_ms) + fold_ms
    return {"leg": "cosets", "curve": cv.name, "log_n": log_n, "coset_size": l, "len": n, "calls": calls, "open_cosets_ms": round(med, 3),
            "prepare_ms": round(prepare_ms, 3), "table_bytes": 8 * n * w, "open_all_ms": round(statistics.median(all_ms), 3),
            "prepare_all_ms": round(prepare_all_ms, 3), "lincomb_segments_ms": round(fold_ms, 3), "reference_ms": round(ref, 3),
            "ratio": round(med / ref, 5)}


def probe_cosets_multi(cv, log_n: int, calls: int, device: int, counts, l: int = 64):
    n, r = 1 << log_n, cv.r
    np = n // l
    wl = workloads.random_circuit(cv, log_n, 0x9B0D)
    srs = setup.unsafe_srs(cv, n, wl.tau, device=device)
    w = 2 * cv.fp_bytes
    key, _ = plonk.Setup(wl.ccs, srs, device=device)
    ctx = key.ctx
    check(lib.apk_kzg_cosets_prepare(ctx, srs.g1, n + 3, l))
    most = max(counts)
    ds, want = [], []
    h, v = C.create_string_buffer(w * np), C.create_string_buffer(32 * n)
    for b in range(most):      # (any value below r is some scalar's stored form: 253 random bits each, from a fixed seed)
        raw = bytearray(hashlib.shake_256(b"kzg_probe cosets-multi %d %d %d" % (cv.abi, log_n, b)).digest(32 * n))
        raw[31::32] = bytes(x & 0x1f for x in raw[31::32])
        buf = bytes(raw)
        d = C.c_void_p()
        check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
        check(lib.apk_device_upload(ctx, d, buf, len(buf)))
        check(lib.apk_kzg_open_cosets_device(ctx, d, n, h, v))      # (the first of them warms the single call up)
        ds.append(d)
        want.append((h.raw, v.raw))
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        check(lib.apk_kzg_open_cosets_device(ctx, ds[0], n, h, v))
        ts.append((time.perf_counter() - t0) * 1e3)
    single = statistics.median(ts)
    for count in counts:
        ptrs = (C.c_void_p * count)(*[d.value for d in ds[:count]])
        lens = (C.c_uint64 * count)(*([n] * count))
        hm, vm = C.create_string_buffer(w * np * count), C.create_string_buffer(32 * n * count)
        ts = []
        for i in range(calls + 1):      # (the first call warms up: the scratch grows with the group)
            t0 = time.perf_counter()
            check(lib.apk_kzg_open_cosets_multi_device(ctx, count, ptrs, lens, hm, vm))
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        same = all(hm.raw[b * w * np:(b + 1) * w * np] == want[b][0] and vm.raw[b * 32 * n:(b + 1) * 32 * n] == want[b][1] for b in range(count))
        assert same, "the batched call differs from the single call at count %d" % count
        med = statistics.median(ts)
        yield {"leg": "cosets-multi", "curve": cv.name, "log_n": log_n, "coset_size": l, "len": n, "count": count, "calls": calls,
               "multi_ms": round(med, 3), "single_ms": round(single, 3), "reference_ms": round(count * single, 3),
               "ratio": round(med / (count * single), 5), "ms_per_polynomial": round(med / count, 3), "same_bytes": same}
    for d in ds:
        check(lib.apk_device_free(ctx, d))
    key.close()


def probe_cosets_verify(cv, log_n: int, calls: int, device: int, l: int = 64) -> dict:
    n, r = 1 << log_n, cv.r
    np = n // l
    wl = workloads.random_circuit(cv, log_n, 0x9B0D)
    srs = setup.unsafe_srs(cv, n, wl.tau, device=device)
    g = SplitMix64(0x9B13)
    buf = cv.fr_vector([g.fr(r) for _ in range(n)])
    w = 2 * cv.fp_bytes
    key, _ = plonk.Setup(wl.ccs, srs, device=device)
    ctx = key.ctx
    check(lib.apk_kzg_cosets_prepare(ctx, srs.g1, n + 3, l))
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    h, v, digest = C.create_string_buffer(w * np), C.create_string_buffer(32 * n), C.create_string_buffer(w)
    check(lib.apk_kzg_open_cosets_device(ctx, d, n, h, v))
    check(lib.apk_msm_g1(ctx, 0, buf, n, digest))
    check(lib.apk_device_free(ctx, d))
    vk = kzg.VerifyingKey(cv, cv.g1, setup.g2_from_tau(cv, wl.tau)).raw()
    g2_l = setup.g2_from_tau(cv, pow(wl.tau, l, r))[2 * w:4 * w]
    srs_l = bytes(srs.g1[:l * w])
    digest_of, indices = (C.c_uint32 * np)(), (C.c_uint64 * np)(*range(np))

    def batch(dev):
        check(lib.apk_kzg_batch_verify_cosets(C.byref(vk), dev, g2_l, srs_l, n, l, 1, digest, np, digest_of, indices, v, h))

    out = {"leg": "cosets-verify", "curve": cv.name, "log_n": log_n, "coset_size": l, "rows": np, "calls": calls}
    phases = ("checks_ms", "point_checks_ms", "hashing_ms", "fold_ms", "segmented_sum_ms", "pairing_ms")
    for name, dev in (("device", device), ("host", -1)):
        batch(dev)                    # (warms up: the pooled buffer, code load, the key's G2 subgroup test)
        ts, split = [], []
        for _ in range(calls):
            t0 = time.perf_counter()
            batch(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
            ms = (C.c_double * 6)()
            check(lib.apk_kzg_cosets_phase_ms(ms))
            split.append(list(ms))
        out["batch_%s_ms" % name] = round(statistics.median(ts), 3)
        out["split_%s" % name] = {p: round(statistics.median(s[i] for s in split), 3) for i, p in enumerate(phases)}
    # the reference: one apk_kzg_verify_coset per row, timed over 16 rows and EXTRAPOLATED to all of them
    ts = []
    for i in range(16):
        t0 = time.perf_counter()
        check(lib.apk_kzg_verify_coset(C.byref(vk), g2_l, srs_l, n, l, i, digest, v.raw[32 * l * i:32 * l * (i + 1)], h.raw[w * i:w * (i + 1)]))
        ts.append((time.perf_counter() - t0) * 1e3)
    key.close()
    one = statistics.median(ts)
    out.update(verify_coset_ms=round(one, 3), reference_ms=round(one * np, 3), reference="extrapolated: median of 16 single calls x rows",
               ratio_device=round(out["batch_device_ms"] / (one * np), 5), ratio_host=round(out["batch_host_ms"] / (one * np), 5))
    return out


def probe_recover(cv, log_n: int, calls: int, device: int, l: int = 64) -> dict:
    n, r = 1 << log_n, cv.r
    np, L = n // l, n // 2
    wl = workloads.random_circuit(cv, log_n, 0x9B0D)
    srs = setup.unsafe_srs(cv, n, wl.tau, device=device)
    g = SplitMix64(0x9B14)
    buf = cv.fr_vector([g.fr(r) for _ in range(L)])
    w = 2 * cv.fp_bytes
    key, _ = plonk.Setup(wl.ccs, srs, device=device)
    ctx = key.ctx
    check(lib.apk_kzg_cosets_prepare(ctx, srs.g1, n + 3, l))
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    h, v = C.create_string_buffer(w * np), C.create_string_buffer(32 * n)
    check(lib.apk_kzg_open_cosets_device(ctx, d, L, h, v))
    order = list(range(np))
    for i in range(np - 1, 0, -1):
        j = g.below(i + 1)
        order[i], order[j] = order[j], order[i]
    kept = order[:np // 2]
    rb = 32 * l
    forms = {"half": (kept, b"".join(v.raw[i * rb:(i + 1) * rb] for i in kept)), "all": (list(range(np)), v.raw)}
    d_out = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d_out)))
    got = C.create_string_buffer(len(buf))
    med, d_rows, idx = {}, {}, {}
    for name, (known, rows) in forms.items():
        d_rows[name] = C.c_void_p()
        check(lib.apk_device_alloc(ctx, len(rows), C.byref(d_rows[name])))
        check(lib.apk_device_upload(ctx, d_rows[name], rows, len(rows)))
        idx[name] = (C.c_uint64 * len(known))(*known)
        ts = []
        for i in range(calls + 1):      # (the first call warms up: the context's table, scratch allocation, code load)
            t0 = time.perf_counter()
            check(lib.apk_kzg_recover_cosets_device(ctx, l, len(known), idx[name], d_rows[name], L, d_out))
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        check(lib.apk_device_download(ctx, got, d_out, len(buf)))
        assert got.raw == buf, "the recovered polynomial differs from the one that was opened (%s cells)" % name
        med[name] = statistics.median(ts)
    # the three transforms inside one more call, event-timed (the statistics add a wait per transform: not part of the medians)
    key.enable_stats(True)
    key.stats(reset=True)
    check(lib.apk_kzg_recover_cosets_device(ctx, l, len(kept), idx["half"], d_rows["half"], L, d_out))
    inside_ms = key.stats(reset=True).ntt_ms
    key.enable_stats(False)
    # three size-n transforms through apk_ntt, host memory in and out
    work = C.create_string_buffer(v.raw, 32 * n)

    def three():
        check(lib.apk_ntt(ctx, 0, 1, 0, work))
        check(lib.apk_ntt(ctx, 0, 0, 0, work))
        check(lib.apk_ntt(ctx, 0, 1, 0, work))

    three()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        three()
        ts.append((time.perf_counter() - t0) * 1e3)
    ntt3 = statistics.median(ts)
    for p in (d, d_out, d_rows["half"], d_rows["all"]):
        check(lib.apk_device_free(ctx, p))
    key.close()
    return {"leg": "recover", "curve": cv.name, "log_n": log_n, "coset_size": l, "len": L, "cells": np, "known": len(kept), "calls": calls,
            "recover_ms": round(med["half"], 3), "recover_all_cells_ms": round(med["all"], 3), "three_apk_ntt_ms": round(ntt3, 3),
            "three_apk_ntt": "host memory in and out, copies included", "ratio_to_three_apk_ntt": round(med["half"] / ntt3, 4),
            "transforms_inside_ms": round(inside_ms, 3), "ratio_to_transforms_inside": round(med["half"] / inside_ms, 4) if inside_ms else None,
            "roots_and_vanish_ms": round(med["half"] - med["all"], 3), "roots_and_vanish_share": round((med["half"] - med["all"]) / med["half"], 4),
            "roots_and_vanish": "by difference of the two medians"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--leg", choices=["both", "canonical", "lagrange", "multi", "multi-lagrange", "all", "cosets", "cosets-verify", "recover", "cosets-multi"], default="both")
    ap.add_argument("--counts", default="1,2,4,8,16,32", help="--leg cosets-multi: the counts, comma-separated (each 1..64)")
    a = ap.parse_args()
    if a.leg == "all":
        for cv, log_n in ((ecc.BN254, 17), (ecc.BLS12_381, 14)):
            print(json.dumps(probe_all(cv, log_n, min(a.calls, 5), a.device)), flush=True)
    if a.leg == "cosets":
        for cv, log_n in ((ecc.BN254, 17), (ecc.BLS12_381, 14)):
            print(json.dumps(probe_cosets(cv, log_n, min(a.calls, 5), a.device)), flush=True)
    if a.leg == "cosets-verify":
        for cv, log_n in ((ecc.BN254, 17), (ecc.BLS12_381, 14)):
            print(json.dumps(probe_cosets_verify(cv, log_n, min(a.calls, 5), a.device)), flush=True)
    if a.leg == "recover":
        for cv, log_n in ((ecc.BN254, 17), (ecc.BLS12_381, 14)):
            print(json.dumps(probe_recover(cv, log_n, min(a.calls, 5), a.device)), flush=True)
    if a.leg == "cosets-multi":
        counts = [int(x) for x in a.counts.split(",")]
        for cv, log_n in ((ecc.BN254, 17), (ecc.BLS12_381, 14)):
            for line in probe_cosets_multi(cv, log_n, min(a.calls, 5), a.device, counts):
                print(json.dumps(line), flush=True)
    for leg, fn in (("canonical", probe), ("lagrange", probe_lagrange)):
        if a.leg in ("both", leg):
            for cv, log_n in ((ecc.BN254, 17), (ecc.BLS12_381, 14)):
                print(json.dumps(fn(cv, log_n, a.calls, a.device)), flush=True)
    if a.leg == "multi":
        for context in ("msm-only", "circuit"):
            for cv, log_n in ((ecc.BN254, 17), (ecc.BLS12_381, 14)):
                print(json.dumps(probe_multi(cv, log_n, a.calls, a.device, context)), flush=True)
    if a.leg == "multi-lagrange":
        for cv, log_n in ((ecc.BN254, 17), (ecc.BLS12_381, 14)):
            print(json.dumps(probe_multi_lagrange(cv, log_n, a.calls, a.device)), flush=True)


if __name__ == "__main__":
    main()

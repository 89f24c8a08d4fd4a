"""GPU tier: apk_kzg_open_cosets_multi* (csrc/kernels_kzg_cosets_multi.h, kzg_cosets_multi_run.h) on circuit contexts of both curves.
The specification is "the bytes of apk_kzg_open_cosets on every polynomial", so the reference is that call on the SAME context,
polynomial by polynomial, byte for byte on H and on the values; one check per shape goes to the big-integer model
(tests/kzg_cosets_model.py) as well.  Shapes (log n, l), the smallest at which each part can go wrong: (3, 2) n' = 4, where the single
call's gather has its special case; (3, 4) n' = 2, a block's only real point beside its infinity; (7, 2) a 2n'-point block is exactly
one stage workgroup; (7, 64) n' = 2 with a full lane group; (9, 16) the mid case.  Counts 1, 2, 3, 16 and 17 (groups of 9 + 8), 64
at (3, 2).  One model multiplication costs a few milliseconds: every test stays below about 1 500 of them."""
from __future__ import annotations

import ctypes as C
import dataclasses
import hashlib
import os
import subprocess
import sys
import threading

import pytest

import kzg_model as km
import test_gpu_kzg_cosets as base
from algoplonk_amd import _lib, batch, kzg as ap_kzg, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd._lib import check, lib
from helpers import CURVES, oracle_threads
from oracle.prng import SplitMix64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254", "bls12-381"]
ARG, STATE = _lib.APK_ERR_ARG, _lib.APK_ERR_STATE
SHAPES = [(3, 2), (3, 4), (7, 2), (7, 64), (9, 16)]      # (log n, l)
_POOL = {}


def _lengths(n, l):
    return [n, 1, l, l + 1, n // 2 + 1]


def pool(R, count):
    """`count` random polynomials of the context's five lengths in turn, with what apk_kzg_open_cosets returns for each: computed
    once per context and shared, never changed.  [(f, [H bytes], [value bytes])]"""
    key = (R.cv.name, R.n, R.l)
    have = _POOL.setdefault(key, [])
    g = SplitMix64(0xD100 + 16 * R.n + R.l + R.cv.abi + 1000 * len(have))
    while len(have) < count:
        L = _lengths(R.n, R.l)[len(have) % 5]
        f = km.polynomial("random", L, R.cv.r, g)
        have.append((f,) + _single(R, f))
    return have[:count]


def _single(R, f, ctx=None):
    rc, hs, vs = base._open(R, f, False, ctx=ctx)
    assert rc == 0, lib.apk_last_error()
    return hs, vs


def _multi(R, fs, device=False, values=True, ctx=None, lens=None, bufs=None):
    """(rc, [[H bytes] per polynomial], [[value bytes] per polynomial] or None); the out buffers pre-filled with 0xa5.  The same list
    object among fs is handed over as the same pointer."""
    cv, n, np = R.cv, R.n, R.np
    ctx = ctx or R.ctx
    count = len(fs)
    w = 2 * cv.fp_bytes
    h = C.create_string_buffer(b"\xa5" * (w * np * count), w * np * count)
    vals = C.create_string_buffer(b"\xa5" * (32 * n * count), 32 * n * count) if values else None
    encoded, freed = {}, []
    for f in fs:
        if id(f) in encoded:
            continue
        raw = cv.fr_vector(f)
        if device:
            d = base._upload(ctx, raw)
            encoded[id(f)] = d.value
            freed.append(d)
        else:
            keep = C.create_string_buffer(raw, len(raw))
            encoded[id(f)] = C.addressof(keep)
            freed.append(keep)
    ptrs = (C.c_void_p * max(count, 1))(*[encoded[id(f)] for f in fs])
    ls = (C.c_uint64 * max(count, 1))(*(lens if lens is not None else [len(f) for f in fs]))
    fn = lib.apk_kzg_open_cosets_multi_device if device else lib.apk_kzg_open_cosets_multi
    rc = fn(ctx, count, ptrs, ls, h, vals)
    if device:
        for d in freed:
            check(lib.apk_device_free(ctx, d))
    hs = [[h.raw[(b * np + i) * w:(b * np + i + 1) * w] for i in range(np)] for b in range(count)]
    vs = [[vals.raw[32 * (b * n + k):32 * (b * n + k + 1)] for k in range(n)] for b in range(count)] if values else None
    return rc, hs, vs


def _hold(R, rows, what, device=False, values=True, ctx=None):
    """one multi call over rows = [(f, want_h, want_v)] held to the single call's bytes"""
    rc, hs, vs = _multi(R, [r[0] for r in rows], device, values, ctx)
    assert rc == 0, (what, lib.apk_last_error())
    for b, (_, want_h, want_v) in enumerate(rows):
        bad = [i for i in range(R.np) if hs[b][i] != want_h[i]]
        assert not bad, "%s: H of polynomial %d of %d differs from the single call at cosets %s" % (what, b, len(rows), bad[:8])
        if values:
            bad = [k for k in range(R.n) if vs[b][k] != want_v[k]]
            assert not bad, "%s: values of polynomial %d of %d differ from the single call at %s" % (what, b, len(rows), bad[:8])
    return hs, vs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_counts_against_the_single_call(gpu, cname, shape):
    """counts 1, 2, 3, 16, 17 (and 64 at n = 8, l = 2): host pointers with the values, device pointers without, and at count 3 the
    other two combinations, and again at count 17 (two groups); every out buffer starts as 0xa5 and must come back as the single call's bytes (a row of len <= l: zeros)"""
    R = base.rig(cname, shape[0], shape[1], gpu)
    counts = [1, 2, 3, 16, 17] + ([64] if shape == (3, 2) else [])
    rows = pool(R, max(counts))
    assert any(not any(any(h) for h in r[1]) for r in rows[:2])      # the second polynomial has len 1: every H is infinity
    for count in counts:
        what = "%s n=%d l=%d count %d" % (cname, R.n, R.l, count)
        _hold(R, rows[:count], what + " host", device=False, values=True)
        _hold(R, rows[:count], what + " device", device=True, values=False)
        if count in (3, 17):      # (17: the second group's proofs and values are copied behind the first group's)
            _hold(R, rows[:count], what + " host, no values", device=False, values=False)
            _hold(R, rows[:count], what + " device, values", device=True, values=True)


@pytest.mark.parametrize("shape", [(3, 2), (7, 8)], ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_mixed_lengths_and_structured_rows(gpu, cname, shape):
    R = base.rig(cname, shape[0], shape[1], gpu)
    cv, r, n, l = R.cv, R.cv.r, R.n, R.l
    g = SplitMix64(0xD200 + cv.abi + n)
    what = "%s n=%d l=%d" % (cname, n, l)

    def row(f):
        return (f,) + _single(R, f)

    full_a, full_b = row(km.polynomial("random", n, r, g)), row(km.polynomial("random", n, r, g))
    zero, short = row([0] * n), row(km.polynomial("random", l, r, g))
    # the five lengths in one call
    _hold(R, [row(km.polynomial("random", L, r, g)) for L in (1, l, l + 1, n // 2 + 1, n)], what + " five lengths")
    # a zero polynomial and one of len <= l BETWEEN two full ones: an infinity block must not leak into its neighbours
    for device in (False, True):
        hs, _ = _hold(R, [full_a, zero, short, full_b], what + " infinity between full", device=device)
        assert not any(any(h) for h in hs[1] + hs[2]) and all(any(h) for h in hs[0][:1] + hs[3][:1])
    # X^(n-1) (the index plan) and X^l - w^(i l) (zero values on one coset)
    i = 1 if R.np == 4 else 5
    top, vanish = row([0] * (n - 1) + [1]), row([(-pow(R.w, i * l, r)) % r] + [0] * (l - 1) + [1])
    _, vs = _hold(R, [top, full_a, vanish], what + " X^(n-1), X^l - a_i")
    assert vs[2][i * l:(i + 1) * l] == [bytes(32)] * l
    # the same pointer twice: equal outputs
    for device in (False, True):
        rc, hs, vs = _multi(R, [full_a[0], full_b[0], full_a[0]], device)
        assert rc == 0 and hs[0] == hs[2] == full_a[1] and vs[0] == vs[2] == full_a[2] and hs[1] == full_b[1], (what, device)
    # [f, g] against [g, f]: the rows swap and nothing else changes
    rc1, h1, v1 = _multi(R, [full_a[0], short[0]])
    rc2, h2, v2 = _multi(R, [short[0], full_a[0]])
    assert rc1 == rc2 == 0 and (h1, v1) == (h2[::-1], v2[::-1]), what


@pytest.mark.parametrize("shape", [(3, 2), (7, 8), (9, 16)], ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_three_polynomials_against_the_model(gpu, cname, shape):
    """(at most 3 x 32 model multiplications for the proofs)"""
    R = base.rig(cname, shape[0], shape[1], gpu)
    g = SplitMix64(0xD300 + R.cv.abi + R.n)
    fs = [km.polynomial("random", L, R.cv.r, g) for L in (R.n, R.l + 1, R.n // 2 + 1)]
    rc, hs, vs = _multi(R, fs)
    assert rc == 0, lib.apk_last_error()
    for b, f in enumerate(fs):
        assert (hs[b], vs[b]) == R.model(f), (cname, shape, b)


@pytest.mark.parametrize("cname", NAMES)
def test_scratch_growth_on_one_slot(gpu, cname):
    """count 2, then 16 (the slot's scratch is released and allocated again), then 3, then the single call"""
    R = base.rig(cname, 7, 8, gpu)
    rows = pool(R, 16)
    for count in (2, 16, 3):
        _hold(R, rows[16 - count:], "%s count %d" % (cname, count), device=count == 16)
    assert _single(R, rows[0][0]) == rows[0][1:]


@pytest.mark.parametrize("cname", NAMES)
def test_end_to_end_with_the_batch_verifier(gpu, cname):
    """OpenCosetsMulti on three polynomials, their commitments, rows drawn from all three in ONE BatchVerifyCosets"""
    R = base.rig(cname, 9, 16, gpu)
    cv, r, n, l = R.cv, R.cv.r, R.n, R.l
    g = SplitMix64(0xD400 + cv.abi)
    fs = [km.polynomial("random", L, r, g) for L in (n, n // 2 + 1, l + 3)]
    ap_kzg.PrepareCosets(R.pk, R.srs, l)      # (the context is prepared: this tells the Python key its coset size)
    proofs = ap_kzg.OpenCosetsMulti(fs, R.pk)
    digests = [ap_kzg.Commit(f, R.pk) for f in fs]
    vk = ap_kzg.VerifyingKey(cv, cv.g1, R.srs.g2)
    g2_l = ap_setup.g2_from_tau(cv, pow(R.tau, l, r))[4 * cv.fp_bytes:]
    picks = [(0, 0), (1, 5), (2, R.np - 1), (0, 17), (2, 3), (1, 5)]      # (polynomial, coset)
    rows = [proofs[b][i] for b, i in picks]
    ap_kzg.BatchVerifyCosets(digests, [b for b, _ in picks], [i for _, i in picks], rows, l, vk, g2_l, R.srs, n=n, device=gpu)
    bad = list(rows)
    bad[4] = dataclasses.replace(bad[4], ClaimedValues=[(bad[4].ClaimedValues[0] + 1) % r] + list(bad[4].ClaimedValues[1:]))
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.BatchVerifyCosets(digests, [b for b, _ in picks], [i for _, i in picks], bad, l, vk, g2_l, R.srs, n=n, device=gpu)


_KNOB_CHILD = r"""
import ctypes as C, hashlib, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from algoplonk_amd._lib import check, lib
import test_gpu_kzg_cosets as base
import test_gpu_kzg_cosets_multi as multi
out = []
for cname in ("bn254", "bls12-381"):
    R = base.Rig(cname, 7, 8, %(gpu)d)
    out.append(multi.knob_digest(R))
    R.pk.close()
print("DIGEST " + " ".join(out))
"""


def knob_digest(R):
    """17 polynomials of fixed seeds through one multi call: the digest of its bytes"""
    g = SplitMix64(0xD500 + R.cv.abi)
    fs = [km.polynomial("random", _lengths(R.n, R.l)[b % 5], R.cv.r, g) for b in range(17)]
    rc, hs, vs = _multi(R, fs)
    assert rc == 0, lib.apk_last_error()
    d = hashlib.sha256()
    for b in range(17):
        d.update(b"".join(hs[b]) + b"".join(vs[b]))
    return d.hexdigest()


def test_plain_stage_form_gives_the_same_bytes(gpu):
    """APK_KZG_ALL_GLV=0 (lagrange_stage_kernel over plain tables) in a fresh process against the default form in this one"""
    here = [knob_digest(base.rig(cname, 7, 8, gpu)) for cname in NAMES]
    env = dict(os.environ, APK_KZG_ALL_GLV="0")
    code = _KNOB_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "gpu": gpu}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")][-1].split()[1:]
    assert got == here, (got, here)


@pytest.mark.parametrize("cname", NAMES)
def test_errors_and_the_call_after_them(gpu, cname):
    cv, _ = CURVES[cname]
    A = base.Rig(cname, 5, 0, gpu)
    n, l = A.n, 4
    A.l, A.np = l, n // l
    g = SplitMix64(0xD600 + cv.abi)
    fs = [km.polynomial("random", L, cv.r, g) for L in (n, l + 1, n - 1)]
    # before apk_kzg_cosets_prepare, and on an MSM-only context: the state comes first, whatever the other arguments are
    assert _multi(A, fs)[0] == STATE and b"apk_kzg_cosets_prepare" in lib.apk_last_error()
    assert _multi(A, fs, device=True)[0] == STATE
    assert _multi(A, [])[0] == STATE
    msm = ap_kzg.MsmContext(cv, A.srs.g1, device=gpu)
    assert _multi(A, fs, ctx=msm.ctx)[0] == STATE and b"MSM-only" in lib.apk_last_error()
    assert _multi(A, [], ctx=msm.ctx)[0] == STATE
    msm.close()
    check(lib.apk_kzg_cosets_prepare(A.ctx, A.srs.g1, n + 3, l))
    rows = [(f,) + _single(A, f) for f in fs]

    def still_right(what):
        _hold(A, rows, "%s after %s" % (cname, what))

    still_right("prepare")
    assert _multi(A, [])[0] == ARG and b"0 polynomials" in lib.apk_last_error()
    still_right("count 0")
    assert _multi(A, [fs[1]] * 65)[0] == ARG and b"65 polynomials" in lib.apk_last_error()
    still_right("count 65")
    for device in (False, True):
        for bad in (0, n + 1):
            big = [fs[0], fs[1], fs[0] + [1]]      # (n + 1 coefficients are there to be read, were the length let through)
            assert _multi(A, big, device, lens=[n, l + 1, bad])[0] == ARG
            assert lib.apk_last_error().startswith(b"polynomial 2: "), lib.apk_last_error()
            still_right("a length of %d in the last row" % bad)
    # host memory in the device form: the second row
    w = 2 * cv.fp_bytes
    d = base._upload(A.ctx, cv.fr_vector(fs[0]))
    host = C.create_string_buffer(cv.fr_vector(fs[1]), 32 * len(fs[1]))
    ptrs = (C.c_void_p * 2)(d.value, C.addressof(host))
    lens = (C.c_uint64 * 2)(n, len(fs[1]))
    h, v = C.create_string_buffer(w * A.np * 2), C.create_string_buffer(32 * n * 2)
    assert lib.apk_kzg_open_cosets_multi_device(A.ctx, 2, ptrs, lens, h, v) == ARG
    assert lib.apk_last_error() == b"kzg: polynomial 1 is not device memory"
    still_right("host memory in the device form")
    # null arguments
    assert lib.apk_kzg_open_cosets_multi_device(A.ctx, 2, None, lens, h, v) == ARG
    assert lib.apk_kzg_open_cosets_multi_device(A.ctx, 2, ptrs, None, h, v) == ARG
    assert lib.apk_kzg_open_cosets_multi_device(A.ctx, 2, ptrs, lens, None, v) == ARG
    assert lib.apk_kzg_open_cosets_multi(A.ctx, 2, (C.c_void_p * 2)(C.addressof(host), None), lens, h, v) == ARG
    assert lib.apk_last_error() == b"kzg: polynomial 1 is null"
    assert lib.apk_kzg_open_cosets_multi(None, 2, ptrs, lens, h, v) == ARG
    still_right("null arguments")
    check(lib.apk_device_free(A.ctx, d))
    A.pk.close()


@pytest.mark.parametrize("cname", NAMES)
def test_multi_openings_beside_proofs(gpu, cname):
    """Two threads open three polynomials on every coset at n = 2^11, l = 64 while two others prove, on a four-slot context: every
    proof is the lone proof's blob (the C oracle's); every opening is what the single call returns alone."""
    import test_gpu_kzg as kzg_base
    from bench_cpu import oracle_blobs
    cv, _ = CURVES[cname]
    r, l = cv.r, 64
    wl = workloads.random_circuit(cv, 11, 0xC180 + cv.abi)
    n = wl.ccs.domain_size()
    srs = ap_setup.unsafe_srs(cv, n, wl.tau, device=gpu)
    items = batch.WitnessSet(None, wl.ccs, workloads.variants(wl, 1, 0xC181), curve=cv).items
    want = oracle_blobs(cv, wl.ccs, srs, items, threads=oracle_threads())
    pk, _ = ap_plonk.Setup(wl.ccs, srs, device=gpu, slots=4)
    ws = batch.WitnessSet(pk, wl.ccs, [])
    ws.items = [dataclasses.replace(it, dev=None, pinned=None) for it in items]
    ws.to_device()
    check(lib.apk_kzg_cosets_prepare(pk.ctx, srs.g1, n + 3, l))

    class View:      # what _multi and base._open read of a Rig
        pass
    V = View()
    V.cv, V.n, V.l, V.np, V.ctx = cv, n, l, n // l, pk.ctx
    g = SplitMix64(0xD700 + cv.abi)
    fs = [km.polynomial("random", L, r, g) for L in (n, l, n // 2 + 1)]
    alone = [_single(V, f) for f in fs]
    errors, rounds = [], 3
    pk.paths(reset=True)

    def prover():
        pr = _lib.Proof()
        for _ in range(rounds):
            rc = ws.prove(0, pr, "device")
            if rc != 0 or kzg_base._marshal(pr) != want[0]:
                errors.append(("proof", rc, lib.apk_last_error()))

    def opener(device):
        for t in range(rounds):
            rc, hs, vs = _multi(V, fs, device)
            if rc != 0 or [(hs[b], vs[b]) for b in range(3)] != alone:
                errors.append(("openings", t, rc, lib.apk_last_error()))

    threads = [threading.Thread(target=prover), threading.Thread(target=prover), threading.Thread(target=opener, args=(False,)),
               threading.Thread(target=opener, args=(True,))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    pc = pk.paths()
    ws.close()
    pk.close()
    assert not errors, errors[:4]
    assert pc["proofs"] == 2 * rounds, pc


def test_python_mirror(gpu):
    R = base.rig("bn254", 7, 8, gpu)
    cv, r, n, l = R.cv, R.cv.r, R.n, R.l
    g = SplitMix64(0xD800)
    f, h = km.polynomial("random", n // 2 + 1, r, g), km.polynomial("random", l, r, g)
    ap_kzg.PrepareCosets(R.pk, R.srs, l)      # (a second time: nothing changes)
    got = ap_kzg.OpenCosetsMulti([f, h, f], R.pk)
    assert len(got) == 3 and got[0] == got[2] == ap_kzg.OpenCosets(f, R.pk) and got[1] == ap_kzg.OpenCosets(h, R.pk)
    assert all(p.H is None for p in got[1])
    with pytest.raises(ValueError):
        ap_kzg.OpenCosetsMulti([f] * 65, R.pk)
    with pytest.raises(ValueError):
        ap_kzg.OpenCosetsMulti([], R.pk)
    with pytest.raises(ValueError):
        ap_kzg.OpenCosetsMulti([f, [1] * (n + 1)], R.pk)
    with pytest.raises(ValueError):
        ap_kzg.OpenCosetsMulti([f, []], R.pk)

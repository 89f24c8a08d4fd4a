"""GPU tier: apk_kzg_open* / apk_kzg_batch_open* (csrc/kernels_kzg.h) against the big-integer model of tests/kzg_model.py, byte
for byte, on a circuit context (n = 2^13) and on an MSM-only context (2^13 + 3 bases) of both curves: every length at which the
kernels take another path (around the lane's chunk, a workgroup's span, n), every kind of point (random, 0, 1, r - 1, on the
domain, a root of the polynomial) and of polynomial; the batch call with and without digests and data transcript; and openings
beside proofs on a two-slot context."""
from __future__ import annotations

import ctypes as C
import dataclasses
import threading

import pytest

import kzg_model as km
from algoplonk_amd import _lib, batch, kzg as ap_kzg, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd._lib import check, lib
from helpers import CURVES, oracle_threads, random_chain_ccs
from oracle.prng import SplitMix64, tau_from_seed

pytestmark = pytest.mark.gpu

LOG_N = 13
N = 1 << LOG_N
NAMES = ["bn254", "bls12-381"]
KINDS = ["circuit", "msm-only"]
_RIG = {}


def _shape():
    a, b = C.c_int(0), C.c_int(0)
    check(lib.apk_kzg_shape(C.byref(a), C.byref(b)))
    return a.value, b.value


def _lengths():
    chunk, span = _shape()
    out = [1, 2, 3, chunk - 1, chunk, chunk + 1, span - 1, span, span + 1, N - 1, N, N + 1, N + 3]
    return sorted(set(x for x in out if 1 <= x <= N + 3))


class Rig:
    """One SRS per curve; a circuit context and an MSM-only context over it."""

    def __init__(self, cname, gpu):
        self.cv, self.ov = CURVES[cname]
        cv = self.cv
        self.tau = tau_from_seed(0x4B2A + cv.abi, cv.r)
        self.srs = ap_setup.unsafe_srs(cv, N, self.tau, device=gpu)
        ccs, _, _ = random_chain_ccs(cv, LOG_N, 0x4B2B)
        self.pk, _ = ap_plonk.Setup(ccs, self.srs, device=gpu)
        self.msm = ap_kzg.MsmContext(cv, self.srs.g1, device=gpu)
        self.vk = km.kzg_vk(cv, self.srs.g2)
        self.pows = [1] * (N + 3)
        for i in range(1, N + 3):
            self.pows[i] = self.pows[i - 1] * self.tau % cv.r

    def ctx(self, kind):
        return self.pk.ctx if kind == "circuit" else self.msm.ctx

    def at_tau(self, f):
        return sum(c * p for c, p in zip(f, self.pows)) % self.cv.r

    def model_open(self, f, z):
        r = self.cv.r
        v = km.horner(f, z, r)
        return self.ov.mul(self.ov.g1, (self.at_tau(f) - v) * pow((self.tau - z) % r, -1, r) % r), v


def rig(cname, gpu) -> Rig:
    if cname not in _RIG:
        _RIG[cname] = Rig(cname, gpu)
    return _RIG[cname]


def _open_host(R, ctx, f, z):
    cv = R.cv
    h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    check(lib.apk_kzg_open(ctx, cv.fr_vector(f), len(f), cv.fr_vector([z]), h, v))
    return h.raw, v.raw


def _upload(ctx, buf):
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    return d


def _open_device(R, ctx, f, z):
    cv = R.cv
    d = _upload(ctx, cv.fr_vector(f))
    h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    rc = lib.apk_kzg_open_device(ctx, d, len(f), cv.fr_vector([z]), h, v)
    check(lib.apk_device_free(ctx, d))
    check(rc)
    return h.raw, v.raw


def _with_root(f, z0, r):
    """(X - z0) * f: a polynomial of len(f) + 1 coefficients with the root z0"""
    out = [0] * (len(f) + 1)
    for i, c in enumerate(f):
        out[i + 1] = (out[i + 1] + c) % r
        out[i] = (out[i] - z0 * c) % r
    return out


def _check_open(R, ctx, f, z, what, device_too=True):
    cv, r = R.cv, R.cv.r
    if (R.tau - z) % r == 0:
        z = (z + 1) % r
    H, v = R.model_open(f, z)
    want = (cv.g1_to_bytes(H), cv.fr_to_mont_bytes(v))
    got = _open_host(R, ctx, f, z)
    assert got == want, "%s: host-pointer opening differs from the model (H %s, value %s)" % (what, got[0] == want[0], got[1] == want[1])
    if device_too:
        assert _open_device(R, ctx, f, z) == want, "%s: device-pointer opening differs from the model" % what
    digest = R.ov.mul(R.ov.g1, R.at_tau(f))
    assert km.verify(cv, R.vk, digest, z, v, H) == 0, (what, lib.apk_last_error())
    return v


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", NAMES)
def test_open_every_length_point_and_polynomial(gpu, cname, kind):
    R = rig(cname, gpu)
    cv, r = R.cv, R.cv.r
    ctx = R.ctx(kind)
    g = SplitMix64(0x09E7 + cv.abi)
    chunk, span = _shape()
    lengths = _lengths()
    # every length: a random polynomial at a random point, host and device pointers
    for L in lengths:
        _check_open(R, ctx, km.polynomial("random", L, r, g), g.fr(r), "%s %s len %d" % (cname, kind, L))
    # every kind of point at the lengths around each path: one lane, several lanes, several workgroups, the longest
    some = sorted(set([1, 3, chunk + 1, span, span + 1, N + 3]))
    w5 = pow(cv.omega(N), 5, r)
    for L in some:
        f = km.polynomial("random", L, r, g)
        for name, z in (("0", 0), ("1", 1), ("r-1", r - 1), ("omega^5", w5)):
            _check_open(R, ctx, f, z, "%s %s len %d point %s" % (cname, kind, L, name), device_too=False)
        if L >= 2:
            z0 = g.fr(r)
            v = _check_open(R, ctx, _with_root(km.polynomial("random", L - 1, r, g), z0, r), z0, "%s %s len %d at a root" % (cname, kind, L), device_too=False)
            assert v == 0
    # every kind of polynomial at those lengths, at a random point and on the domain
    for L in some:
        for pk in ("zero", "constant", "max", "top"):
            f = km.polynomial(pk, L, r, g)
            for z in (g.fr(r), w5):
                _check_open(R, ctx, f, z, "%s %s len %d %s" % (cname, kind, L, pk), device_too=False)
    # H of the zero polynomial and of a constant is the point at infinity
    h, v = _open_host(R, ctx, [0] * (span + 1), g.fr(r))
    assert not any(h) and not any(v)
    h, v = _open_host(R, ctx, [5], g.fr(r))
    assert not any(h) and cv.fr_from_mont_bytes(v) == 5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", NAMES)
def test_open_length_limits(gpu, cname, kind):
    R = rig(cname, gpu)
    cv = R.cv
    ctx = R.ctx(kind)
    f = cv.fr_vector([1] * (N + 4))
    h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    assert lib.apk_kzg_open(ctx, f, N + 4, cv.fr_vector([2]), h, v) == _lib.APK_ERR_ARG      # above n + 3 / the context's base count
    assert lib.apk_kzg_open(ctx, f, 0, cv.fr_vector([2]), h, v) == _lib.APK_ERR_ARG
    assert lib.apk_kzg_open(ctx, f, N + 3, cv.fr_vector([2]), h, v) == 0
    d = _upload(ctx, f)
    assert lib.apk_kzg_open_device(ctx, d, N + 4, cv.fr_vector([2]), h, v) == _lib.APK_ERR_ARG
    assert lib.apk_kzg_open_device(ctx, f, 4, cv.fr_vector([2]), h, v) == _lib.APK_ERR_ARG   # a host pointer is not device memory
    lens = (C.c_uint64 * 2)(4, N + 4)
    ptrs = (C.c_void_p * 2)(d.value, d.value)
    vals = C.create_string_buffer(64)
    assert lib.apk_kzg_batch_open_device(ctx, 2, ptrs, lens, None, cv.fr_vector([2]), None, 0, h, vals, None) == _lib.APK_ERR_ARG
    check(lib.apk_device_free(ctx, d))
    if kind == "msm-only":      # a shorter base set: its own limit
        small = ap_kzg.MsmContext(cv, R.srs.g1[: 2048 * 2 * cv.fp_bytes], device=gpu)
        assert lib.apk_kzg_open(small.ctx, f, 2049, cv.fr_vector([2]), h, v) == _lib.APK_ERR_ARG
        assert lib.apk_kzg_open(small.ctx, f, 2048, cv.fr_vector([2]), h, v) == 0
        small.close()


def _batch(R, ctx, polys, z, extra, digests, device):
    cv = R.cv
    k = len(polys)
    bufs = [cv.fr_vector(p) for p in polys]
    lens = (C.c_uint64 * k)(*[len(p) for p in polys])
    h, vals, gamma = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32 * k), C.create_string_buffer(32)
    dg = cv.g1_vector(digests) if digests is not None else None
    if device:
        ds = [_upload(ctx, b) for b in bufs]
        ptrs = (C.c_void_p * k)(*[d.value for d in ds])
        rc = lib.apk_kzg_batch_open_device(ctx, k, ptrs, lens, dg, cv.fr_vector([z]), extra or None, len(extra), h, vals, gamma)
        for d in ds:
            check(lib.apk_device_free(ctx, d))
    else:
        keep = [C.create_string_buffer(b, len(b)) for b in bufs]
        ptrs = (C.c_void_p * k)(*[C.addressof(b) for b in keep])
        rc = lib.apk_kzg_batch_open(ctx, k, ptrs, lens, dg, cv.fr_vector([z]), extra or None, len(extra), h, vals, gamma)
    return rc, h.raw, vals.raw, gamma.raw


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", NAMES)
def test_batch_open(gpu, cname, kind):
    R = rig(cname, gpu)
    cv, ov, r = R.cv, R.ov, R.cv.r
    ctx = R.ctx(kind)
    g = SplitMix64(0xBA7C + cv.abi)
    lengths = _lengths()
    extra100 = bytes(g.below(256) for _ in range(100))
    for count in (1, 2, 5, 32):
        # lengths 1 and n + 3 in one batch (from two polynomials on), the others walk the list
        ls = ([1, N + 3] + [lengths[(3 * i + count) % len(lengths)] for i in range(count)])[:count] if count > 1 else [N + 3]
        kinds = ["random", "random", "zero", "top", "max", "constant"]
        polys = [km.polynomial(kinds[i % len(kinds)], L, r, g) for i, L in enumerate(ls)]
        z = g.fr(r)
        digests = [ov.mul(ov.g1, R.at_tau(f)) for f in polys]
        # what the call commits when it is given no digests is what apk_msm_g1 commits
        out = C.create_string_buffer(2 * cv.fp_bytes)
        for f, d in list(zip(polys, digests))[:6]:
            check(lib.apk_msm_g1(ctx, 0, cv.fr_vector(f), len(f), out))
            assert out.raw == cv.g1_to_bytes(d)
        values = [km.horner(f, z, r) for f in polys]
        for extra, given, device in ((b"", True, True), (extra100, False, True), (extra100, True, False), (b"", False, False)):
            gamma = km.fold_challenge(ov, z, digests, values, extra)
            kq, gp = 0, 1
            for f, v in zip(polys, values):
                kq = (kq + gp * (R.at_tau(f) - v)) % r
                gp = gp * gamma % r
            H = ov.mul(ov.g1, kq * pow((R.tau - z) % r, -1, r) % r)
            rc, h, vals, gm = _batch(R, ctx, polys, z, extra, digests if given else None, device)
            what = "%s %s count %d extra %d digests %s device %s" % (cname, kind, count, len(extra), given, device)
            assert rc == 0, (what, lib.apk_last_error())
            assert vals == cv.fr_vector(values), what + ": values"
            assert gm == cv.fr_to_mont_bytes(gamma), what + ": gamma"
            assert h == cv.g1_to_bytes(H), what + ": H"
            assert km.batch_verify(cv, R.vk, digests, values, z, extra, H) == 0, (what, lib.apk_last_error())
    # 33 polynomials
    polys = [[1, 2]] * 33
    rc, _, _, _ = _batch(R, ctx, polys, 5, b"", None, True)
    assert rc == _lib.APK_ERR_ARG


def test_python_mirror(gpu):
    R = rig("bn254", gpu)
    cv, r = R.cv, R.cv.r
    g = SplitMix64(0x9171)
    vk = ap_kzg.VerifyingKey(cv, cv.g1, R.srs.g2)
    for key in (R.pk, R.msm):
        f, z = km.polynomial("random", 300, r, g), g.fr(r)
        com = ap_kzg.Commit(f, key)
        assert com == R.ov.mul(R.ov.g1, R.at_tau(f))
        pr = ap_kzg.Open(f, z, key)
        assert (pr.H, pr.ClaimedValue) == R.model_open(f, z)
        ap_kzg.Verify(com, pr, z, vk)
        with pytest.raises(ap_kzg.VerificationError):
            ap_kzg.Verify(com, ap_kzg.OpeningProof(pr.H, (pr.ClaimedValue + 1) % r), z, vk)
        polys = [f, km.polynomial("random", 7, r, g)]
        bp = ap_kzg.BatchOpenSinglePoint(polys, None, z, key, b"data")
        digs = [ap_kzg.Commit(p, key) for p in polys]
        assert bp.ClaimedValues == [km.horner(p, z, r) for p in polys]
        ap_kzg.BatchVerifySinglePoint(digs, bp, z, vk, b"data")
        with pytest.raises(ap_kzg.VerificationError):
            ap_kzg.BatchVerifySinglePoint(digs, bp, z, vk, b"datb")


def _marshal(pr) -> bytes:
    out = C.create_string_buffer(2048)
    ln = C.c_size_t(0)
    check(lib.apk_marshal_proof(C.byref(pr), out, 2048, C.byref(ln)))
    return out.raw[: ln.value]


@pytest.mark.parametrize("cname", NAMES)
def test_openings_beside_proofs_on_two_slots(gpu, cname):
    """Two threads prove distinct assignments while two threads open, on a two-slot context at n = 2^11: every proof is the C
    oracle's proof of its inputs, every opening the model's, and no call became a member of a gang."""
    from bench_cpu import oracle_blobs
    cv, ov = CURVES[cname]
    r = cv.r
    wl = workloads.random_circuit(cv, 11, 0x4B2C + cv.abi)
    n = wl.ccs.domain_size()
    srs = ap_setup.unsafe_srs(cv, n, wl.tau, device=gpu)
    items = batch.WitnessSet(None, wl.ccs, workloads.variants(wl, 2, 0x4B2D), curve=cv).items
    want = oracle_blobs(cv, wl.ccs, srs, items, threads=oracle_threads())
    assert want[0] != want[1]
    pk, _ = ap_plonk.Setup(wl.ccs, srs, device=gpu, slots=2)
    ws = batch.WitnessSet(pk, wl.ccs, [])
    ws.items = [dataclasses.replace(it, dev=None, pinned=None) for it in items]
    ws.to_device()
    g = SplitMix64(0x4B2E)
    pows = [pow(wl.tau, i, r) for i in range(n + 3)]
    jobs = []
    for L in (n + 3, 2049, 9, n):
        f, z = km.polynomial("random", L, r, g), g.fr(r)
        v = km.horner(f, z, r)
        k = (sum(c * p for c, p in zip(f, pows)) - v) * pow((wl.tau - z) % r, -1, r) % r
        jobs.append((cv.fr_vector(f), L, cv.fr_vector([z]), cv.g1_to_bytes(ov.mul(ov.g1, k)), cv.fr_to_mont_bytes(v)))
    errors, rounds = [], 6
    pk.paths(reset=True)

    def prover(i):
        pr = _lib.Proof()
        for _ in range(rounds):
            rc = ws.prove(i, pr, "device")
            if rc != 0 or _marshal(pr) != want[i]:
                errors.append(("proof", i, rc, lib.apk_last_error()))

    def opener(i):
        h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
        for t in range(rounds):
            buf, L, z, wh, wv = jobs[(2 * t + i) % len(jobs)]
            rc = lib.apk_kzg_open(pk.ctx, buf, L, z, h, v)
            if rc != 0 or h.raw != wh or v.raw != wv:
                errors.append(("opening", i, L, rc, lib.apk_last_error()))

    threads = [threading.Thread(target=prover, args=(i,)) for i in range(2)] + [threading.Thread(target=opener, args=(i,)) for i in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    pc = pk.paths()
    ws.close()
    pk.close()
    assert not errors, errors[:4]
    assert pc["proofs"] == 2 * rounds and pc["gang_proofs"] == 0 and pc["gang_kernel_launches"] == 0, pc

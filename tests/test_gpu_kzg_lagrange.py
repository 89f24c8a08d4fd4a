"""GPU tier: apk_kzg_open_lagrange* / apk_kzg_batch_open_lagrange* (csrc/kernels_kzg_lagrange.h) against the big-integer model of
tests/kzg_lagrange_model.py, byte for byte, on circuit contexts over one known-tau SRS per curve at every domain size at which
the kernels take another path (n = 8, a part of a workgroup's span, one span, two, four), every kind of point (random, 0, on
the domain at the lane and workgroup boundaries) and of value vector; the cross-check with apk_kzg_open of the coefficients; the
batch call with and without digests and data transcript; the refusals; and openings beside proofs on a two-slot context."""
from __future__ import annotations

import ctypes as C
import threading

import pytest

import kzg_lagrange_model as klm
import kzg_model as km
from algoplonk_amd import _lib, batch, kzg as ap_kzg, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd._lib import check, lib
from helpers import CURVES
from oracle.prng import SplitMix64

pytestmark = pytest.mark.gpu

_RIG = {}


def _shape():
    a, b = C.c_int(0), C.c_int(0)
    check(lib.apk_kzg_lagrange_shape(C.byref(a), C.byref(b)))
    return a.value, b.value


def _sizes(cname):
    _, span = _shape()
    return [8, 2 * span] if cname == "bls12-381" else [8, span // 4, span, 2 * span, 4 * span]


def _cases():
    return [(c, k) for c in ("bn254", "bls12-381") for k in range(len(_sizes(c)))]


CASES = _cases()
IDS = ["%s-n%d" % (c, _sizes(c)[k]) for c, k in CASES]


class Rig:
    """A circuit context of n rows over a known-tau SRS, with the model's view of the same SRS."""

    def __init__(self, cname, n, gpu, slots=1):
        self.cv, self.ov = CURVES[cname]
        cv = self.cv
        self.n = n
        self.wl = workloads.random_circuit(cv, n.bit_length() - 1, 0x1A9 + n + cv.abi)
        assert self.wl.ccs.domain_size() == n
        self.tau = self.wl.tau
        srs = ap_setup.unsafe_srs(cv, n, self.tau, device=gpu)
        self.pk, _ = ap_plonk.Setup(self.wl.ccs, srs, device=gpu, slots=slots)
        self.g2 = srs.g2
        self.vk = km.kzg_vk(cv, srs.g2)
        self.dom = klm.Domain(cv.omega(n), n, cv.r)
        self.srs = klm.Srs(self.dom, self.tau)
        self.w = {}

    @property
    def ctx(self):
        return self.pk.ctx

    def weights(self, z):
        if z not in self.w:
            self.w[z] = self.dom.weights(z)
        return self.w[z]

    def model_open(self, f, z, at_tau=None):
        r = self.cv.r
        v = klm.dot(f, self.weights(z), r)
        t = self.srs.at_tau(f) if at_tau is None else at_tau
        return self.ov.mul(self.ov.g1, (t - v) * pow((self.tau - z) % r, -1, r) % r), v

    def point(self, z):
        """the point, or another one when it hits tau"""
        return z if (self.tau - z) % self.cv.r else (z + 1) % self.cv.r


def rig(cname, k, gpu) -> Rig:
    key = (cname, _sizes(cname)[k])
    if key not in _RIG:
        _RIG[key] = Rig(cname, key[1], gpu)
    return _RIG[key]


def _upload(ctx, buf):
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    return d


def _open_host(R, buf, z):
    cv = R.cv
    h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    check(lib.apk_kzg_open_lagrange(R.ctx, buf, R.n, cv.fr_vector([z]), h, v))
    return h.raw, v.raw


def _open_device(R, d, z):
    cv = R.cv
    h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    check(lib.apk_kzg_open_lagrange_device(R.ctx, d, R.n, cv.fr_vector([z]), h, v))
    return h.raw, v.raw


def _commit(R, buf):
    out = C.create_string_buffer(2 * R.cv.fp_bytes)
    check(lib.apk_msm_g1(R.ctx, 1, buf, R.n, out))
    return out.raw


def _domain_points(R):
    """(name, point): 1, r - 1, omega^(n-1) and omega^m at the lane and workgroup boundaries below n"""
    chunk, span = _shape()
    n, r = R.n, R.cv.r
    out = [("1", 1), ("r-1", r - 1), ("omega^(n-1)", R.dom.pts[n - 1])]
    assert R.dom.find(1) == 0 and R.dom.find(r - 1) == n // 2
    for m in (chunk - 1, chunk, span - 1, span):
        if m < n:
            out.append(("omega^%d" % m, R.dom.pts[m]))
    return out


@pytest.mark.parametrize("cname,k", CASES, ids=IDS)
def test_open_every_point_and_vector(gpu, cname, k):
    R = rig(cname, k, gpu)
    cv, ov, r, n, dom = R.cv, R.ov, R.cv.r, R.n, R.dom
    g = SplitMix64(0x1A90 + n + cv.abi)
    points = [("random", R.point(g.fr(r))), ("0", 0)] + [(nm, R.point(z)) for nm, z in _domain_points(R)]
    m_hot = min(n - 1, _shape()[1] - 1)
    vectors = [("random", klm.vector("random", dom, g)), ("zero", klm.vector("zero", dom, g)), ("constant", klm.vector("constant", dom, g)),
               ("one-hot", klm.vector("one-hot", dom, g, m_hot)), ("max", klm.vector("max", dom, g)), ("top", klm.vector("top", dom, g))]
    for vname, f in vectors:
        buf = cv.fr_vector(f)
        at_tau = R.srs.at_tau(f)
        digest = ov.mul(ov.g1, at_tau)
        assert _commit(R, buf) == cv.g1_to_bytes(digest), "%s n %d %s: the basis-1 commitment is not [f(tau)]G1" % (cname, n, vname)
        d = _upload(R.ctx, buf)
        try:
            # the random vector at every point; the structured ones at a random point, at 0, at omega^(n-1) and - the one-hot
            # vector - at the point where it is not zero
            mine = points if vname == "random" else points[:2] + [points[4]] + ([("omega^m", R.point(dom.pts[m_hot]))] if vname == "one-hot" else [])
            for pname, z in mine:
                what = "%s n %d %s at %s" % (cname, n, vname, pname)
                H, v = R.model_open(f, z, at_tau)
                want = (cv.g1_to_bytes(H), cv.fr_to_mont_bytes(v))
                got = _open_host(R, buf, z)
                assert got == want, "%s: host-pointer opening differs from the model (H %s, value %s)" % (what, got[0] == want[0], got[1] == want[1])
                got = _open_device(R, d, z)
                assert got == want, "%s: device-pointer opening differs from the model (H %s, value %s)" % (what, got[0] == want[0], got[1] == want[1])
                assert km.verify(cv, R.vk, digest, z, v, H) == 0, (what, lib.apk_last_error())
                if vname in ("zero", "constant"):      # H is the point at infinity and the value is exact, off the domain too
                    assert not any(got[0]) and v == f[0], what
        finally:
            check(lib.apk_device_free(R.ctx, d))


@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_opening_equals_the_canonical_opening_of_the_coefficients(gpu, cname):
    sizes = _sizes(cname)
    _, span = _shape()
    for k, n in enumerate(sizes):
        if n > 2 * span or (n > span // 4 and n != 2 * span):
            continue
        R = rig(cname, k, gpu)
        cv, r = R.cv, R.cv.r
        g = SplitMix64(0x1A91 + n + cv.abi)
        f = klm.vector("random", R.dom, g)
        # the coefficients: computed here at the small sizes, by apk_ntt(inverse) at two spans
        coeffs = R.pk.ntt(f, which=0, inverse=True) if n == 2 * span else R.dom.interpolate(f)
        assert km.horner(coeffs, R.dom.pts[5], r) == f[5]
        for z in (R.point(g.fr(r)), 0, R.dom.pts[n - 1]):
            h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
            check(lib.apk_kzg_open(R.ctx, cv.fr_vector(coeffs), n, cv.fr_vector([z]), h, v))
            assert _open_host(R, cv.fr_vector(f), z) == (h.raw, v.raw), (cname, n, z)


def _batch(R, vectors, z, extra, digests, device):
    cv = R.cv
    k = len(vectors)
    bufs = [cv.fr_vector(p) for p in vectors]
    h, vals, gamma = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32 * k), C.create_string_buffer(32)
    dg = cv.g1_vector(digests) if digests is not None else None
    if device:
        ds = [_upload(R.ctx, b) for b in bufs]
        ptrs = (C.c_void_p * k)(*[d.value for d in ds])
        rc = lib.apk_kzg_batch_open_lagrange_device(R.ctx, k, ptrs, dg, cv.fr_vector([z]), extra or None, len(extra), h, vals, gamma)
        for d in ds:
            check(lib.apk_device_free(R.ctx, d))
    else:
        keep = [C.create_string_buffer(b, len(b)) for b in bufs]
        ptrs = (C.c_void_p * k)(*[C.addressof(b) for b in keep])
        rc = lib.apk_kzg_batch_open_lagrange(R.ctx, k, ptrs, dg, cv.fr_vector([z]), extra or None, len(extra), h, vals, gamma)
    return rc, h.raw, vals.raw, gamma.raw


@pytest.mark.parametrize("cname,k", [("bn254", 0), ("bn254", 3), ("bls12-381", 1)], ids=["bn254-n8", "bn254-2span", "bls12-381-2span"])
def test_batch_open(gpu, cname, k):
    R = rig(cname, k, gpu)
    cv, ov, r, n, dom = R.cv, R.ov, R.cv.r, R.n, R.dom
    _, span = _shape()
    g = SplitMix64(0x1A92 + n + cv.abi)
    extra100 = bytes(g.below(256) for _ in range(100))
    kinds = ["random", "random", "zero", "top", "max", "constant"]
    pool = [klm.vector(kinds[i % len(kinds)], dom, g) for i in range(32)]
    digests_all = [ov.mul(ov.g1, R.srs.at_tau(f)) for f in pool]
    for count in (1, 2, 5, 32):
        vectors, digests = pool[:count], digests_all[:count]
        for z in (R.point(g.fr(r)), R.point(dom.pts[min(span, n) - 1])):
            w = R.weights(z)
            values = [klm.dot(f, w, r) for f in vectors]
            for extra, given, device in ((b"", True, True), (extra100, False, True), (extra100, True, False), (b"", False, False)):
                want = klm.batch_open_at(ov, R.srs, vectors, z, extra, digests)
                assert want[1] == values
                rc, h, vals, gm = _batch(R, vectors, z, extra, digests if given else None, device)
                what = "%s n %d count %d extra %d digests %s device %s" % (cname, n, count, len(extra), given, device)
                assert rc == 0, (what, lib.apk_last_error())
                assert vals == cv.fr_vector(values), what + ": values"
                assert gm == cv.fr_to_mont_bytes(want[2]), what + ": gamma"
                assert h == cv.g1_to_bytes(want[3]), what + ": H"
                assert km.batch_verify(cv, R.vk, digests, values, z, extra, want[3]) == 0, (what, lib.apk_last_error())
            if count >= 2:      # the verifier rejects a wrong value and swapped digests
                bumped = [(values[0] + 1) % r] + values[1:]
                assert km.batch_verify(cv, R.vk, digests, bumped, z, b"", want[3]) == _lib.APK_ERR_VERIFY
                assert km.batch_verify(cv, R.vk, [digests[1], digests[0]] + digests[2:], values, z, b"", want[3]) == _lib.APK_ERR_VERIFY
    rc, _, _, _ = _batch(R, [pool[0]] * 33, 5, b"", None, True)
    assert rc == _lib.APK_ERR_ARG


def test_refusals(gpu):
    R = rig("bn254", 2, gpu)
    cv, n = R.cv, R.n
    f = cv.fr_vector([1] * (n + 3))
    z = cv.fr_vector([2])
    h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
    d = _upload(R.ctx, f)
    for ln in (n - 1, n + 3):
        assert lib.apk_kzg_open_lagrange(R.ctx, f, ln, z, h, v) == _lib.APK_ERR_ARG
        assert lib.apk_kzg_open_lagrange_device(R.ctx, d, ln, z, h, v) == _lib.APK_ERR_ARG
    assert lib.apk_kzg_open_lagrange_device(R.ctx, f, n, z, h, v) == _lib.APK_ERR_ARG      # a host pointer is not device memory
    assert lib.apk_kzg_open_lagrange_device(R.ctx, d, n, z, h, v) == 0
    check(lib.apk_device_free(R.ctx, d))
    # an MSM-only context has no domain
    msm = ap_kzg.MsmContext(cv, ap_setup.unsafe_srs(cv, 8, R.tau, device=gpu).g1, device=gpu)
    try:
        assert lib.apk_kzg_open_lagrange(msm.ctx, f, 8, z, h, v) == _lib.APK_ERR_STATE
        ptrs = (C.c_void_p * 1)(C.cast(C.c_char_p(f), C.c_void_p).value)
        assert lib.apk_kzg_batch_open_lagrange(msm.ctx, 1, ptrs, None, z, None, 0, h, v, None) == _lib.APK_ERR_STATE
    finally:
        msm.close()
    # the context is as usable as before
    assert lib.apk_kzg_open_lagrange(R.ctx, f, n, z, h, v) == 0


def test_python_mirror(gpu):
    R = rig("bn254", 1, gpu)
    cv, r = R.cv, R.cv.r
    g = SplitMix64(0x1A93)
    vk = ap_kzg.VerifyingKey(cv, cv.g1, R.g2)
    f = klm.vector("random", R.dom, g)
    for z in (R.point(g.fr(r)), R.dom.pts[7]):
        com = ap_kzg.CommitLagrange(f, R.pk)
        assert com == klm.commit(R.ov, R.srs, f)
        pr = ap_kzg.OpenLagrange(f, z, R.pk)
        assert (pr.H, pr.ClaimedValue) == klm.open_at(R.ov, R.srs, f, z)
        ap_kzg.Verify(com, pr, z, vk)
        with pytest.raises(ap_kzg.VerificationError):
            ap_kzg.Verify(com, ap_kzg.OpeningProof(pr.H, (pr.ClaimedValue + 1) % r), z, vk)
        vectors = [f, klm.vector("random", R.dom, g)]
        bp = ap_kzg.BatchOpenSinglePointLagrange(vectors, None, z, R.pk, b"data")
        digs = [ap_kzg.CommitLagrange(p, R.pk) for p in vectors]
        assert bp.ClaimedValues == [R.dom.evaluate(p, z) for p in vectors]
        assert bp.H == klm.batch_open_at(R.ov, R.srs, vectors, z, b"data")[3]
        ap_kzg.BatchVerifySinglePoint(digs, bp, z, vk, b"data")
        with pytest.raises(ap_kzg.VerificationError):
            ap_kzg.BatchVerifySinglePoint(digs, bp, z, vk, b"datb")


def _marshal(pr) -> bytes:
    out = C.create_string_buffer(2048)
    ln = C.c_size_t(0)
    check(lib.apk_marshal_proof(C.byref(pr), out, 2048, C.byref(ln)))
    return out.raw[: ln.value]


def test_openings_beside_proofs_on_two_slots(gpu):
    """One thread proves while one opens in evaluation form, on a two-slot context at four spans: every result is the one the
    same call gave alone (the openings also the model's), and the context is usable afterwards."""
    _, span = _shape()
    R = Rig("bn254", 4 * span, gpu, slots=2)
    cv, r, n = R.cv, R.cv.r, R.n
    ws = batch.WitnessSet(R.pk, R.wl.ccs, workloads.variants(R.wl, 1, 0x1A94))
    ws.to_device()
    g = SplitMix64(0x1A95)
    jobs = []
    for z in (R.point(g.fr(r)), R.dom.pts[span - 1], R.point(g.fr(r)), 0):
        f = klm.vector("random", R.dom, g)
        buf = cv.fr_vector(f)
        alone = _open_host(R, buf, z)
        H, v = R.model_open(f, z)
        assert alone == (cv.g1_to_bytes(H), cv.fr_to_mont_bytes(v))
        jobs.append((buf, cv.fr_vector([z]), alone))
    pr = _lib.Proof()
    assert ws.prove(0, pr, "device") == 0, lib.apk_last_error()
    want = _marshal(pr)
    errors, rounds = [], 6

    def prover():
        p = _lib.Proof()
        for _ in range(rounds):
            rc = ws.prove(0, p, "device")
            if rc != 0 or _marshal(p) != want:
                errors.append(("proof", rc, lib.apk_last_error()))

    def opener():
        h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
        for t in range(2 * rounds):
            buf, z, alone = jobs[t % len(jobs)]
            rc = lib.apk_kzg_open_lagrange(R.ctx, buf, n, z, h, v)
            if rc != 0 or (h.raw, v.raw) != alone:
                errors.append(("opening", t, rc, lib.apk_last_error()))

    threads = [threading.Thread(target=prover), threading.Thread(target=opener)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    try:
        assert not errors, errors[:4]
        # usable afterwards: a proof and an opening once more
        assert ws.prove(0, pr, "device") == 0 and _marshal(pr) == want
        assert _open_host(R, jobs[1][0], R.dom.pts[span - 1]) == jobs[1][2]
    finally:
        ws.close()
        R.pk.close()

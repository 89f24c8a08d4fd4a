"""GPU tier: apk_kzg_open_multi_lagrange* (csrc/kernels_kzg_lagrange.h KzgLagGroup*K, kzg_run.h kzg_lag_group_open) on the rigs of
tests/test_gpu_kzg_lagrange.py - circuit contexts over a known-tau SRS at the smallest sizes at which each path exists: n = 8 (a
part of one lane row), one span (exactly one workgroup) and two spans (the product of the OTHER workgroups and the
cross-workgroup partials exist), sizes taken from apk_kzg_lagrange_shape - against the big-integer model of
tests/kzg_lagrange_model.py, byte for byte and in both pointer forms: every group shape with ONE MSM batch per group, rows on
and off the domain in one group in every rotation, the on-domain edges of the lane map, one vector at many points, duplicates,
the agreement with the single calls and with the coefficient form, the multi-point verifier, openings beside proofs and the
refusals."""
from __future__ import annotations

import ctypes as C
import threading

import pytest

import kzg_lagrange_model as klm
import test_gpu_kzg_lagrange as base
from algoplonk_amd import _lib, batch, kzg as ap_kzg, setup as ap_setup, workloads
from algoplonk_amd._lib import check, lib
from oracle.prng import SplitMix64

pytestmark = pytest.mark.gpu

GROUP = 4      # MSMs per launch sequence of a circuit context


def _shape():
    return base._shape()


def _sizes(cname):
    _, span = _shape()
    return [8, 2 * span] if cname == "bls12-381" else [8, span, 2 * span]


CASES = [(c, n) for c in ("bn254", "bls12-381") for n in _sizes(c)]
IDS = ["%s-n%d" % cn for cn in CASES]
BIG = [(c, _sizes(c)[-1]) for c in ("bn254", "bls12-381")]      # two spans
BIG_IDS = ["%s-n%d" % cn for cn in BIG]


def rig(cname, n, gpu):
    return base.rig(cname, base._sizes(cname).index(n), gpu)


def _msm_batches(ctx) -> int:
    pc = _lib.PathCounts()
    check(lib.apk_paths_read(ctx, C.byref(pc), 0))
    return pc.as_dict()["msm_batches"]


def _multi(R, vectors, zs, device, ctx=None):
    """(rc, [H bytes], [value bytes]); list objects that occur several times in `vectors` are ONE buffer, handed in several times"""
    cv = R.cv
    ctx = ctx or R.ctx
    k, w = len(vectors), 2 * cv.fp_bytes
    h, vals = C.create_string_buffer(w * k), C.create_string_buffer(32 * k)
    bufs = {}
    for p in vectors:
        if id(p) not in bufs:
            bufs[id(p)] = cv.fr_vector(p)
    if device:
        ds = {i: base._upload(ctx, b) for i, b in bufs.items()}
        ptrs = (C.c_void_p * k)(*[ds[id(p)].value for p in vectors])
        rc = lib.apk_kzg_open_multi_lagrange_device(ctx, k, ptrs, cv.fr_vector(zs), h, vals)
        for d in ds.values():
            check(lib.apk_device_free(ctx, d))
    else:
        keep = {i: C.create_string_buffer(b, len(b)) for i, b in bufs.items()}
        ptrs = (C.c_void_p * k)(*[C.addressof(keep[id(p)]) for p in vectors])
        rc = lib.apk_kzg_open_multi_lagrange(ctx, k, ptrs, cv.fr_vector(zs), h, vals)
    return rc, [h.raw[i * w:(i + 1) * w] for i in range(k)], [vals.raw[32 * i:32 * (i + 1)] for i in range(k)]


_AT_TAU = {}


def _model(R, f, z):
    """the model's (H, value) of one pair; f(tau) once per vector object"""
    assert (R.tau - z) % R.cv.r != 0
    if id(f) not in _AT_TAU:
        _AT_TAU[id(f)] = (f, R.srs.at_tau(f))      # (f is kept: its id stays its own)
    return R.model_open(f, z, _AT_TAU[id(f)][1])


def _check_multi(R, vectors, zs, what, forms=(False, True), ctx=None):
    """Both pointer forms against the model, byte for byte; returns the model's (H, values) and the call's H bytes"""
    cv = R.cv
    want = [_model(R, f, z) for f, z in zip(vectors, zs)]
    want_h = [cv.g1_to_bytes(H) for H, _ in want]
    want_v = [cv.fr_to_mont_bytes(v) for _, v in want]
    for device in forms:
        rc, hs, vs = _multi(R, vectors, zs, device, ctx)
        assert rc == 0, (what, device, lib.apk_last_error())
        bad = [(i, hs[i] == want_h[i], vs[i] == want_v[i]) for i in range(len(vectors)) if hs[i] != want_h[i] or vs[i] != want_v[i]]
        assert not bad, "%s (%s pointers): openings (index, H equal, value equal) %s differ from the model" % (what, "device" if device else "host", bad)
    return [H for H, _ in want], [v for _, v in want], want_h


def _point(g, R):
    return R.point(g.fr(R.cv.r))


_POOL = {}


def _pool(R, cname):
    """32 random vectors per rig, shared by the tests (and by the model's cache)"""
    key = (cname, R.n)
    if key not in _POOL:
        g = SplitMix64(0x1AC0 + R.n + R.cv.abi)
        _POOL[key] = [klm.vector("random", R.dom, g) for _ in range(32 if R.n > 8 else 8)]
    return _POOL[key]


# ---- 1. group shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 8, 9, 32])
@pytest.mark.parametrize("cname,n", BIG, ids=BIG_IDS)
def test_group_shapes(gpu, cname, n, count):
    R = rig(cname, n, gpu)
    g = SplitMix64(0x1AC1 + 64 * R.cv.abi + count)
    vectors = _pool(R, cname)[:count]
    zs = [_point(g, R) for _ in range(count)]
    what = "%s n %d count %d" % (cname, n, count)
    _check_multi(R, vectors[:1], zs[:1], what + " (first use)", forms=(True,))      # (the Lagrange table and the scratch exist from here on)
    groups = (count + GROUP - 1) // GROUP
    for device in (False, True):
        before = _msm_batches(R.ctx)
        _check_multi(R, vectors, zs, what, forms=(device,))
        assert _msm_batches(R.ctx) - before == groups, "%s: ONE launch sequence of the MSM per group" % what


# ---- 2. rows on and off the domain in one group -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,n", CASES, ids=IDS)
def test_mixed_rows_in_one_group_every_rotation(gpu, cname, n):
    R = rig(cname, n, gpu)
    r, dom = R.cv.r, R.dom
    g = SplitMix64(0x1AC2 + n + R.cv.abi)
    chunk, span = _shape()
    edge = span if n == 2 * span else n - 1
    assert chunk < n and edge < n
    rows = _pool(R, cname)[:4]
    zs = [_point(g, R), 0, R.point(dom.pts[chunk]), R.point(dom.pts[edge])]
    assert [dom.find(z) for z in zs] == [None, None, chunk, edge]
    _check_multi(R, rows[:1], zs[:1], "%s n %d (first use)" % (cname, n), forms=(True,))      # (the Lagrange table and the scratch exist from here on)
    for rot in range(4):
        before = _msm_batches(R.ctx)
        _check_multi(R, rows[rot:] + rows[:rot], zs[rot:] + zs[:rot], "%s n %d rotation %d" % (cname, n, rot))
        assert _msm_batches(R.ctx) - before == 2
    # every row on the domain (no sum launch), every row off it (no fill launch)
    _check_multi(R, rows, [R.point(dom.pts[m]) for m in (0, chunk, edge, n // 2)], "%s n %d all on the domain" % (cname, n))
    _check_multi(R, rows, [_point(g, R), 0, _point(g, R), r - 2], "%s n %d all off the domain" % (cname, n))


# ---- 3. the on-domain edges of the lane map, one per row ----------------------------------------------------------------------------
@pytest.mark.parametrize("cname,n", CASES, ids=IDS)
def test_on_domain_edges_and_structured_vectors(gpu, cname, n):
    R = rig(cname, n, gpu)
    cv, r, dom = R.cv, R.cv.r, R.dom
    g = SplitMix64(0x1AC3 + n + cv.abi)
    chunk, span = _shape()
    ms = sorted({m for m in (0, chunk - 1, chunk, span - 1, span, n // 2, n - 1) if m < n})
    zs = [R.point(dom.pts[m]) for m in ms]
    assert [dom.find(z) for z in zs] == ms and zs[ms.index(n // 2)] == r - 1
    inf = bytes(2 * cv.fp_bytes)
    _check_multi(R, _pool(R, cname)[:len(ms)], zs, "%s n %d random vectors at omega^%s" % (cname, n, ms))
    for kind in ("zero", "constant", "max", "top"):
        f = klm.vector(kind, dom, g)
        _, vs, hs = _check_multi(R, [f] * len(ms), zs, "%s n %d %s at omega^%s" % (cname, n, kind, ms))
        if kind in ("zero", "constant", "max"):      # constants: H is the point at infinity and the value is exact
            assert all(h == inf for h in hs) and vs == [f[0]] * len(ms)
    hots = [klm.vector("one-hot", dom, g, m) for m in ms]
    _, vs, _ = _check_multi(R, hots, zs, "%s n %d one-hot at the opened index" % (cname, n))
    assert vs == [f[m] for f, m in zip(hots, ms)] and all(vs)
    # ... and with the one-hot index one row off: the value is zero, H is not
    _, vs, hs = _check_multi(R, hots[1:] + hots[:1], zs, "%s n %d one-hot beside the opened index" % (cname, n), forms=(True,))
    assert vs == [0] * len(ms) and all(h != inf for h in hs)


# ---- 4. one vector at many points, duplicates ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,n", BIG, ids=BIG_IDS)
def test_one_vector_at_many_points_and_duplicates(gpu, cname, n):
    R = rig(cname, n, gpu)
    dom = R.dom
    g = SplitMix64(0x1AC4 + R.cv.abi)
    chunk, span = _shape()
    pool = _pool(R, cname)
    f, f2 = pool[5], pool[6]
    # the same buffer nine times: distinct points, on and off the domain
    zs = [_point(g, R) for _ in range(5)] + [0, R.point(dom.pts[span]), R.point(dom.pts[span - 1]), R.point(dom.pts[n - 1])]
    assert len(set(zs)) == 9
    _check_multi(R, [f] * 9, zs, "%s one vector at nine points" % cname)
    # the same (vector, point) pair twice in one group and across two groups - off the domain and on it
    for z in (zs[0], zs[6]):
        z2 = _point(g, R)
        vectors, pts = [f, f2, f, pool[7], f], [z, z2, z, z2, z]
        for device in (False, True):
            rc, hs, vs = _multi(R, vectors, pts, device)
            assert rc == 0 and hs[0] == hs[2] == hs[4] and vs[0] == vs[2] == vs[4]
        _check_multi(R, vectors, pts, "%s duplicates at %s" % (cname, "a random point" if z == zs[0] else "omega^span"))
    # two different vectors at the same point in one group
    for z in (zs[1], zs[7]):
        _, vs, hs = _check_multi(R, [f, f2, f2, f], [z, z, zs[2], zs[2]], "%s two vectors at one point" % cname)
        assert hs[0] != hs[1] and vs[0] != vs[1]


# ---- 5. agreement with the existing calls -------------------------------------------------------------------------------------------
def _verify(R, device, digests: bytes, points, values, hs: bytes) -> int:
    cv = R.cv
    return lib.apk_kzg_batch_verify_multi(C.byref(R.vk), device, len(points), digests, cv.fr_vector(points), cv.fr_vector(values), hs)


@pytest.mark.parametrize("cname,n", CASES, ids=IDS)
def test_agreement_with_the_single_calls_and_the_verifier(gpu, cname, n):
    R = rig(cname, n, gpu)
    cv, r, dom = R.cv, R.cv.r, R.dom
    g = SplitMix64(0x1AC5 + n + cv.abi)
    chunk, span = _shape()
    pool = _pool(R, cname)
    vectors = [pool[0], pool[1], pool[0], pool[2], pool[3]]
    zs = [_point(g, R), R.point(dom.pts[n - 1]), 0, _point(g, R), R.point(dom.pts[chunk])]
    _, vs, want_h = _check_multi(R, vectors, zs, "%s n %d five pairs" % (cname, n))
    rc, hs, vals = _multi(R, vectors, zs, True)
    assert rc == 0 and hs == want_h
    for i, (f, z) in enumerate(zip(vectors, zs)):
        assert base._open_host(R, cv.fr_vector(f), z) == (hs[i], vals[i]), "%s n %d: apk_kzg_open_lagrange of pair %d" % (cname, n, i)
    if n == 2 * span:      # the coefficient form on the coefficients apk_ntt(inverse) gives
        coeffs = {}
        for i, (f, z) in enumerate(zip(vectors, zs)):
            if id(f) not in coeffs:
                coeffs[id(f)] = cv.fr_vector(R.pk.ntt(f, which=0, inverse=True))
            h, v = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(32)
            check(lib.apk_kzg_open(R.ctx, coeffs[id(f)], n, cv.fr_vector([z]), h, v))
            assert (h.raw, v.raw) == (hs[i], vals[i]), "%s n %d: apk_kzg_open of the coefficients of pair %d" % (cname, n, i)
    # the multi-point verifier takes the outputs against the basis-1 commitments, folding on the host and on the GPU
    digests = b"".join(base._commit(R, cv.fr_vector(f)) for f in vectors)
    assert digests == b"".join(cv.g1_to_bytes(klm.commit(R.ov, R.srs, f)) for f in vectors)
    for device in (-1, gpu):
        assert _verify(R, device, digests, zs, vs, b"".join(hs)) == 0, (device, lib.apk_last_error())
        for pos in (0, 2, 4):
            bumped = list(vs)
            bumped[pos] = (bumped[pos] + 1) % r
            assert _verify(R, device, digests, zs, bumped, b"".join(hs)) == _lib.APK_ERR_VERIFY, (device, pos)


# ---- 6. the Python mirror -----------------------------------------------------------------------------------------------------------
def test_python_mirror(gpu):
    cname = "bn254"
    R = rig(cname, _sizes(cname)[1], gpu)
    cv, r, dom = R.cv, R.cv.r, R.dom
    g = SplitMix64(0x1AC6)
    vk = ap_kzg.VerifyingKey(cv, cv.g1, R.g2)
    pool = _pool(R, cname)
    f = pool[0]
    vectors, zs = [f, f, pool[1], klm.vector("constant", dom, g), f], [_point(g, R), R.point(dom.pts[7]), 0, _point(g, R), R.point(dom.pts[R.n - 1])]
    proofs = ap_kzg.OpenMultiPointsLagrange(vectors, zs, R.pk)
    assert [(p.H, p.ClaimedValue) for p in proofs] == [_model(R, p, z) for p, z in zip(vectors, zs)]
    assert proofs == [ap_kzg.OpenLagrange(p, z, R.pk) for p, z in zip(vectors, zs)]
    assert proofs[3].H is None
    digests = [ap_kzg.CommitLagrange(p, R.pk) for p in vectors]
    for device in (-1, gpu):
        ap_kzg.BatchVerifyMultiPoints(digests, proofs, zs, vk, device=device)
        bad = list(proofs)
        bad[4] = ap_kzg.OpeningProof(bad[4].H, (bad[4].ClaimedValue + 1) % r)
        with pytest.raises(ap_kzg.VerificationError):
            ap_kzg.BatchVerifyMultiPoints(digests, bad, zs, vk, device=device)
    with pytest.raises(ValueError):
        ap_kzg.OpenMultiPointsLagrange([f], [1, 2], R.pk)


# ---- 7. beside proofs ---------------------------------------------------------------------------------------------------------------
def test_multi_point_openings_beside_proofs_on_two_slots(gpu):
    """One thread proves while one opens five (vector, point) pairs per call in evaluation form, on a two-slot context at two
    spans: every proof is the lone proof's blob, every opening the model's, and the context is usable afterwards."""
    _, span = _shape()
    R = base.Rig("bn254", 2 * span, gpu, slots=2)
    cv, r, dom = R.cv, R.cv.r, R.dom
    ws = batch.WitnessSet(R.pk, R.wl.ccs, workloads.variants(R.wl, 1, 0x1AC7))
    ws.to_device()
    g = SplitMix64(0x1AC8)
    w = 2 * cv.fp_bytes
    jobs = []
    for pts in ((_point(g, R), R.point(dom.pts[span - 1]), 0, _point(g, R), R.point(dom.pts[span])),
                (R.point(dom.pts[1]), _point(g, R), _point(g, R), R.point(dom.pts[R.n - 1]), _point(g, R))):
        vecs = [klm.vector("random", dom, g) for _ in range(3)]
        vectors = [vecs[0], vecs[1], vecs[0], vecs[2], vecs[1]]
        want = [R.model_open(f, z) for f, z in zip(vectors, pts)]
        bufs = [C.create_string_buffer(cv.fr_vector(f), 32 * R.n) for f in vecs]
        ptrs = (C.c_void_p * 5)(*[C.addressof(bufs[vecs.index(f)]) for f in vectors])
        jobs.append((bufs, ptrs, cv.fr_vector(list(pts)), b"".join(cv.g1_to_bytes(H) for H, _ in want), b"".join(cv.fr_to_mont_bytes(v) for _, v in want)))
    pr = _lib.Proof()
    assert ws.prove(0, pr, "device") == 0, lib.apk_last_error()
    want_proof = base._marshal(pr)
    errors, rounds = [], 6
    R.pk.paths(reset=True)

    def prover():
        p = _lib.Proof()
        for _ in range(rounds):
            rc = ws.prove(0, p, "device")
            if rc != 0 or base._marshal(p) != want_proof:
                errors.append(("proof", rc, lib.apk_last_error()))

    def opener():
        h, v = C.create_string_buffer(5 * w), C.create_string_buffer(5 * 32)
        for t in range(rounds):
            _, ptrs, zs, wh, wv = jobs[t % len(jobs)]
            rc = lib.apk_kzg_open_multi_lagrange(R.ctx, 5, ptrs, zs, h, v)
            if rc != 0 or h.raw != wh or v.raw != wv:
                errors.append(("openings", t, rc, lib.apk_last_error()))

    threads = [threading.Thread(target=prover), threading.Thread(target=opener)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    try:
        assert not errors, errors[:4]
        pc = R.pk.paths()
        assert pc["proofs"] == rounds and pc["gang_proofs"] == 0 and pc["gang_kernel_launches"] == 0, pc      # no call joined a gang
        # usable afterwards: a proof and the openings once more
        assert ws.prove(0, pr, "device") == 0 and base._marshal(pr) == want_proof
        h, v = C.create_string_buffer(5 * w), C.create_string_buffer(5 * 32)
        check(lib.apk_kzg_open_multi_lagrange(R.ctx, 5, jobs[0][1], jobs[0][2], h, v))
        assert (h.raw, v.raw) == (jobs[0][3], jobs[0][4])
    finally:
        ws.close()
        R.pk.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(gpu):
    cname = "bn254"
    R = rig(cname, _sizes(cname)[1], gpu)
    cv, n = R.cv, R.n
    g = SplitMix64(0x1AC9)
    ARG, STATE = _lib.APK_ERR_ARG, _lib.APK_ERR_STATE
    k, w = 5, 2 * cv.fp_bytes
    pool = _pool(R, cname)
    good, good_zs = [pool[0], pool[1]], [_point(g, R), R.point(R.dom.pts[3])]
    buf = C.create_string_buffer(cv.fr_vector([1] * n), 32 * n)
    ptrs = (C.c_void_p * k)(*[C.addressof(buf)] * k)
    d = base._upload(R.ctx, buf.raw)
    dptrs = (C.c_void_p * k)(*[d.value] * k)
    zs, h, vals = cv.fr_vector([2] * k), C.create_string_buffer(w * k), C.create_string_buffer(32 * k)
    try:
        # an MSM-only context has no domain
        msm = ap_kzg.MsmContext(cv, ap_setup.unsafe_srs(cv, 8, R.tau, device=gpu).g1, device=gpu)
        try:
            assert lib.apk_kzg_open_multi_lagrange(msm.ctx, k, ptrs, zs, h, vals) == STATE
            assert lib.apk_kzg_open_multi_lagrange_device(msm.ctx, k, dptrs, zs, h, vals) == STATE
        finally:
            msm.close()
        _check_multi(R, good, good_zs, "after the MSM-only refusal")
        # a host pointer in the _device form
        assert lib.apk_kzg_open_multi_lagrange_device(R.ctx, k, ptrs, zs, h, vals) == ARG
        mixed = (C.c_void_p * k)(d.value, d.value, ptrs[0], d.value, d.value)
        assert lib.apk_kzg_open_multi_lagrange_device(R.ctx, k, mixed, zs, h, vals) == ARG
        _check_multi(R, good, good_zs, "after the host-pointer refusal")
        # a null vector in the middle of the list
        for fn, pp in ((lib.apk_kzg_open_multi_lagrange, ptrs), (lib.apk_kzg_open_multi_lagrange_device, dptrs)):
            holes = (C.c_void_p * k)(pp[0], pp[0], None, pp[0], pp[0])
            assert fn(R.ctx, k, holes, zs, h, vals) == ARG
            assert fn(R.ctx, 0, pp, zs, h, vals) == ARG and fn(R.ctx, 33, pp, zs, h, vals) == ARG
            _check_multi(R, good, good_zs, "after the null-vector refusal")
            assert fn(R.ctx, k, pp, zs, h, vals) == 0
    finally:
        check(lib.apk_device_free(R.ctx, d))

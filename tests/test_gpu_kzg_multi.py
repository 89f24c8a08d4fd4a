"""GPU tier: apk_kzg_open_multi* (csrc/kernels_kzg.h KzgGroup*K, kzg_run.h kzg_group_divide) and apk_kzg_batch_verify_multi on the
rig of tests/test_gpu_kzg.py - n = 2^13, both curves, a circuit context and an MSM-only context of n + 3 bases over a known-tau
SRS - against the big-integer model of tests/kzg_model.py, byte for byte: every group shape (a partial group, a full one, a
full one plus one, several, the maximum), rows of every kind in one group in every rotation, the carry over three workgroups,
every kind of point, one polynomial at many points, duplicates, the verifier on the host and on the GPU, openings beside proofs
and the argument errors."""
from __future__ import annotations

import ctypes as C
import dataclasses
import threading

import pytest

import kzg_model as km
import test_gpu_kzg as base
from algoplonk_amd import _lib, batch, kzg as ap_kzg, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd._lib import check, lib
from helpers import CURVES, oracle_threads
from oracle.prng import SplitMix64

pytestmark = pytest.mark.gpu

N = base.N
NAMES = base.NAMES
KINDS = base.KINDS
GROUP = 4      # MSMs per launch sequence of a circuit context (an MSM-only context's workspace takes one)


def _msm_batches(ctx) -> int:
    pc = _lib.PathCounts()
    check(lib.apk_paths_read(ctx, C.byref(pc), 0))
    return pc.as_dict()["msm_batches"]


def _multi(R, ctx, polys, zs, device):
    """(rc, [H bytes], [value bytes]); list objects that occur several times in `polys` are ONE buffer, handed in several times"""
    cv = R.cv
    k, w = len(polys), 2 * cv.fp_bytes
    lens = (C.c_uint64 * k)(*[len(p) for p in polys])
    h, vals = C.create_string_buffer(w * k), C.create_string_buffer(32 * k)
    bufs = {}
    for p in polys:
        if id(p) not in bufs:
            bufs[id(p)] = cv.fr_vector(p)
    if device:
        ds = {i: base._upload(ctx, b) for i, b in bufs.items()}
        ptrs = (C.c_void_p * k)(*[ds[id(p)].value for p in polys])
        rc = lib.apk_kzg_open_multi_device(ctx, k, ptrs, lens, cv.fr_vector(zs), h, vals)
        for d in ds.values():
            check(lib.apk_device_free(ctx, d))
    else:
        keep = {i: C.create_string_buffer(b, len(b)) for i, b in bufs.items()}
        ptrs = (C.c_void_p * k)(*[C.addressof(keep[id(p)]) for p in polys])
        rc = lib.apk_kzg_open_multi(ctx, k, ptrs, lens, cv.fr_vector(zs), h, vals)
    return rc, [h.raw[i * w:(i + 1) * w] for i in range(k)], [vals.raw[32 * i:32 * (i + 1)] for i in range(k)]


class Model:
    """The model's openings, computed once per (polynomial, point) and shared by the tests of a curve"""

    def __init__(self, R):
        self.R, self.at_tau, self.done = R, {}, {}

    def open(self, f, z):
        R, r = self.R, self.R.cv.r
        assert (R.tau - z) % r != 0
        key = (id(f), z)
        if key not in self.done:
            if id(f) not in self.at_tau:
                ft = R.at_tau(f)
                self.at_tau[id(f)] = (f, ft, R.ov.mul(R.ov.g1, ft))      # (f is kept: its id stays its own)
            ft = self.at_tau[id(f)][1]
            v = km.horner(f, z, r)
            H = R.ov.mul(R.ov.g1, (ft - v) * pow((R.tau - z) % r, -1, r) % r)
            self.done[key] = (H, v, self.at_tau[id(f)][2])
        return self.done[key]


_MODEL = {}


def model(cname, gpu) -> Model:
    if cname not in _MODEL:
        _MODEL[cname] = Model(base.rig(cname, gpu))
    return _MODEL[cname]


def _check_multi(M, ctx, polys, zs, what, forms=(False, True), single=True):
    """Both pointer forms against the model and against apk_kzg_open of every pair; returns the model's (digests, H, values)"""
    R, cv = M.R, M.R.cv
    want = [M.open(f, z) for f, z in zip(polys, zs)]
    want_h = [cv.g1_to_bytes(H) for H, _, _ in want]
    want_v = [cv.fr_to_mont_bytes(v) for _, v, _ in want]
    for device in forms:
        rc, hs, vs = _multi(R, ctx, polys, zs, device)
        assert rc == 0, (what, device, lib.apk_last_error())
        bad = [i for i in range(len(polys)) if hs[i] != want_h[i] or vs[i] != want_v[i]]
        assert not bad, "%s (%s pointers): openings %s differ from the model (lengths %s)" % (what, "device" if device else "host", bad, [len(polys[i]) for i in bad])
    if single:
        for i, (f, z) in enumerate(zip(polys, zs)):
            assert base._open_host(R, ctx, f, z) == (want_h[i], want_v[i]), "%s: apk_kzg_open of pair %d" % (what, i)
    return [d for _, _, d in want], [H for H, _, _ in want], [v for _, v, _ in want]


def _point(g, R):
    z = g.fr(R.cv.r)
    return z if (R.tau - z) % R.cv.r else (z + 1) % R.cv.r


_POLYS = {}


def _poly(cname, L, g, tag=0):
    """one random polynomial per (curve, length, tag), shared by the tests (and by the model's cache)"""
    key = (cname, L, tag)
    if key not in _POLYS:
        _POLYS[key] = km.polynomial("random", L, CURVES[cname][0].r, g)
    return _POLYS[key]


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 8, 9, 32])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", NAMES)
def test_group_shapes(gpu, cname, kind, count):
    R, M = base.rig(cname, gpu), model(cname, gpu)
    ctx = R.ctx(kind)
    g = SplitMix64(0x6D01 + 64 * R.cv.abi + count)
    chunk, span = base._shape()
    lengths = [N + 3, chunk + 1, span + 1, 3, 2 * span, span, N, 2, chunk, N + 1, span - 1]      # (no constant: every row is an operand)
    polys = [_poly(cname, lengths[(i + count) % len(lengths)], g) for i in range(count)]
    zs = [_point(g, R) for _ in range(count)]
    before = _msm_batches(ctx)
    _check_multi(M, ctx, polys, zs, "%s %s count %d" % (cname, kind, count), single=False)
    # ONE launch sequence of the MSM per group, in both pointer forms (an MSM-only context's workspace takes one MSM: groups of one)
    per = GROUP if kind == "circuit" else 1
    assert _msm_batches(ctx) - before == 2 * ((count + per - 1) // per)
    _check_multi(M, ctx, polys, zs, "%s %s count %d" % (cname, kind, count), forms=())      # ... and apk_kzg_open of every pair


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", NAMES)
def test_mixed_rows_in_one_group_and_groups_of_constants(gpu, cname, kind):
    """A constant (H = infinity, no operand of the batch), a row of one workgroup (no apply), of two and of five workgroups in one
    group, in every rotation of the four positions; four constants run no MSM at all."""
    R, M = base.rig(cname, gpu), model(cname, gpu)
    cv = R.cv
    ctx = R.ctx(kind)
    g = SplitMix64(0x6D02 + cv.abi)
    chunk, span = base._shape()
    assert (N + 3 + span - 1) // span == 5
    rows = [_poly(cname, L, g) for L in (1, chunk + 1, span + 1, N + 3)]
    zs = [_point(g, R) for _ in range(4)]
    for rot in range(4):
        polys, pts = rows[rot:] + rows[:rot], zs[rot:] + zs[:rot]
        before = _msm_batches(ctx)
        _, hs, _ = _check_multi(M, ctx, polys, pts, "%s %s rotation %d" % (cname, kind, rot), single=(rot == 0))
        assert _msm_batches(ctx) - before == 2 * (1 if kind == "circuit" else 3) + (3 if rot == 0 else 0)
        assert hs[(4 - rot) % 4] is None
    # a group of four constants, and five of them (a group of four and a group of one): no MSM
    consts = [[g.fr(cv.r)] for _ in range(5)]
    for k in (4, 5):
        before = _msm_batches(ctx)
        for device in (False, True):
            rc, hs, vs = _multi(R, ctx, consts[:k], zs[:1] * k, device)
            assert rc == 0, lib.apk_last_error()
            assert all(not any(h) for h in hs) and vs == [cv.fr_to_mont_bytes(c[0]) for c in consts[:k]]
        assert _msm_batches(ctx) == before
    # constants and the others in two groups: [c, c, c, c] [f, c, f] - the second batch has two operands
    polys = consts[:4] + [rows[2], consts[4], rows[3]]
    before = _msm_batches(ctx)
    _check_multi(M, ctx, polys, [_point(g, R) for _ in polys], "%s %s constants then a mixed group" % (cname, kind), single=False)
    assert _msm_batches(ctx) - before == 2 * (1 if kind == "circuit" else 2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", NAMES)
def test_carry_over_three_workgroups_and_every_kind_of_point(gpu, cname, kind):
    R, M = base.rig(cname, gpu), model(cname, gpu)
    cv, r = R.cv, R.cv.r
    ctx = R.ctx(kind)
    g = SplitMix64(0x6D03 + cv.abi)
    chunk, span = base._shape()
    # 2 span: two full workgroups; 2 span + 1: a third workgroup of one coefficient, whose total is carried over two others
    polys = [_poly(cname, 2 * span, g), _poly(cname, 2 * span + 1, g), _poly(cname, 2 * span + 1, g, tag=1), _poly(cname, 2 * span, g, tag=1)]
    _check_multi(M, ctx, polys, [_point(g, R), _point(g, R), 0, r - 1], "%s %s lengths around two spans" % (cname, kind))
    # every kind of point, each row of a group another kind: random, 0, 1, r - 1 | omega^5, omega^(n-1), a root, random
    z0 = _point(g, R)
    rooted = base._with_root(km.polynomial("random", span + 2, r, g), z0, r)
    w = cv.omega(N)
    polys = [_poly(cname, N + 3, g), _poly(cname, span + 1, g), _poly(cname, N, g), _poly(cname, chunk + 1, g),
             _poly(cname, N + 3, g), _poly(cname, N, g), rooted, _poly(cname, 3, g)]
    zs = [_point(g, R), 0, 1, r - 1, pow(w, 5, r), pow(w, N - 1, r), z0, _point(g, R)]
    _, _, vs = _check_multi(M, ctx, polys, zs, "%s %s kinds of points" % (cname, kind))
    assert vs[6] == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", NAMES)
def test_one_polynomial_at_many_points_and_duplicates(gpu, cname, kind):
    R, M = base.rig(cname, gpu), model(cname, gpu)
    cv = R.cv
    ctx = R.ctx(kind)
    g = SplitMix64(0x6D04 + cv.abi)
    f = _poly(cname, N + 3, g)
    for k in (4, 9):      # the same pointer k times: one buffer (one upload), k openings
        _check_multi(M, ctx, [f] * k, [_point(g, R) for _ in range(k)], "%s %s one polynomial at %d points" % (cname, kind, k), single=(k == 4))
    # one pointer under two lengths: the shorter use reads a prefix of the same staged vector
    short = f[:base._shape()[1] + 1]
    z = _point(g, R)
    want = M.open(short, z)
    k, w = 2, 2 * cv.fp_bytes
    buf = C.create_string_buffer(cv.fr_vector(f), 32 * len(f))
    ptrs = (C.c_void_p * k)(C.addressof(buf), C.addressof(buf))
    h, vals = C.create_string_buffer(w * k), C.create_string_buffer(32 * k)
    check(lib.apk_kzg_open_multi(ctx, k, ptrs, (C.c_uint64 * k)(len(short), len(f)), cv.fr_vector([z, z]), h, vals))
    assert (h.raw[:w], vals.raw[:32]) == (cv.g1_to_bytes(want[0]), cv.fr_to_mont_bytes(want[1]))
    assert (h.raw[w:], vals.raw[32:]) == base._open_host(R, ctx, f, z)
    # the same (polynomial, point) twice, inside one group and across two: identical outputs
    z2 = _point(g, R)
    polys, zs = [f, short, f, _poly(cname, 9, g), f], [z, z2, z, z2, z]
    rc, hs, vs = _multi(R, ctx, polys, zs, True)
    assert rc == 0 and hs[0] == hs[2] == hs[4] and vs[0] == vs[2] == vs[4]
    _check_multi(M, ctx, polys, zs, "%s %s duplicates" % (cname, kind), single=False)


def _verify(R, device, digests, points, values, hs) -> int:
    cv = R.cv
    return lib.apk_kzg_batch_verify_multi(C.byref(R.vk), device, len(digests), cv.g1_vector(digests), cv.fr_vector(points),
                                          cv.fr_vector(values), cv.g1_vector(hs))


@pytest.mark.parametrize("count", [1, 2, 5, 32])
@pytest.mark.parametrize("cname", NAMES)
def test_verifier_on_the_host_and_on_the_gpu(gpu, cname, count):
    """What apk_kzg_open_multi produced (the model's bytes: asserted) goes through apk_kzg_batch_verify_multi with the fold on
    the host and on the GPU: the unaltered batch, ONE altered value, H, point or digest at the first, a middle and the last
    position, and two errors that cancel under equal weights - the same verdict from both, every time."""
    R, M = base.rig(cname, gpu), model(cname, gpu)
    cv, r = R.cv, R.cv.r
    g = SplitMix64(0x6D05 + 64 * cv.abi + count)
    chunk, span = base._shape()
    lengths = [N + 3, chunk + 1, 1, span + 1, 3]      # (a constant among them from three openings on)
    polys = [_poly(cname, lengths[i % len(lengths)], g) for i in range(count)]
    zs = [_point(g, R) for _ in range(count)]
    digests, hs, vs = _check_multi(M, R.ctx("circuit"), polys, zs, "%s count %d" % (cname, count), forms=(True,), single=False)
    other = R.ov.mul(R.ov.g1, g.fr(r))
    for device in (-1, gpu):
        assert _verify(R, device, digests, zs, vs, hs) == 0, (device, lib.apk_last_error())
    for pos in sorted({0, count // 2, count - 1}):
        for what in ("value", "H", "point", "digest"):
            if what == "point" and hs[pos] is None:
                continue      # (a constant opens to itself at every point)
            d, z, v, h = list(digests), list(zs), list(vs), list(hs)
            if what == "value":
                v[pos] = (v[pos] + 1) % r
            elif what == "H":
                h[pos] = other
            elif what == "point":
                z[pos] = (z[pos] + 1) % r
            else:
                d[pos] = other
            got = [_verify(R, device, d, z, v, h) for device in (-1, gpu)]
            assert got == [_lib.APK_ERR_VERIFY] * 2, (what, pos, got)
    if count >= 2:
        v = list(vs)
        v[0], v[count - 1] = (v[0] + 77) % r, (v[count - 1] - 77) % r
        got = [_verify(R, device, digests, zs, v, hs) for device in (-1, gpu)]
        assert got == [_lib.APK_ERR_VERIFY] * 2, got
    # a device that does not exist is an error of its own, never a verdict
    assert _verify(R, 1 << 20, digests, zs, vs, hs) not in (0, _lib.APK_ERR_VERIFY)


def test_python_mirror(gpu):
    R, M = base.rig("bn254", gpu), model("bn254", gpu)
    cv, r = R.cv, R.cv.r
    g = SplitMix64(0x6D06)
    vk = ap_kzg.VerifyingKey(cv, cv.g1, R.srs.g2)
    f = _poly("bn254", base._shape()[1] + 1, g)
    for key in (R.pk, R.msm):
        polys, zs = [f, f, _poly("bn254", 3, g), [7], f], [_point(g, R) for _ in range(5)]
        proofs = ap_kzg.OpenMultiPoints(polys, zs, key)
        assert [(p.H, p.ClaimedValue) for p in proofs] == [M.open(p, z)[:2] for p, z in zip(polys, zs)]
        assert proofs == [ap_kzg.Open(p, z, key) for p, z in zip(polys, zs)]
        digests = [M.open(p, z)[2] for p, z in zip(polys, zs)]
        for device in (-1, gpu):
            ap_kzg.BatchVerifyMultiPoints(digests, proofs, zs, vk, device=device)
            bad = list(proofs)
            bad[4] = ap_kzg.OpeningProof(bad[4].H, (bad[4].ClaimedValue + 1) % r)
            with pytest.raises(ap_kzg.VerificationError):
                ap_kzg.BatchVerifyMultiPoints(digests, bad, zs, vk, device=device)
    with pytest.raises(ValueError):
        ap_kzg.OpenMultiPoints([f], [1, 2], R.pk)


@pytest.mark.parametrize("cname", NAMES)
def test_multi_point_openings_beside_proofs_on_two_slots(gpu, cname):
    """One thread proves while one opens five (polynomial, point) pairs per call, on a two-slot context at n = 2^11: every proof
    is the lone proof's blob (the C oracle's), every opening the model's, and no call became a member of a gang."""
    from bench_cpu import oracle_blobs
    cv, ov = CURVES[cname]
    r = cv.r
    wl = workloads.random_circuit(cv, 11, 0x4B2C + cv.abi)
    n = wl.ccs.domain_size()
    srs = ap_setup.unsafe_srs(cv, n, wl.tau, device=gpu)
    items = batch.WitnessSet(None, wl.ccs, workloads.variants(wl, 1, 0x4B2D), curve=cv).items
    want = oracle_blobs(cv, wl.ccs, srs, items, threads=oracle_threads())
    pk, _ = ap_plonk.Setup(wl.ccs, srs, device=gpu, slots=2)
    ws = batch.WitnessSet(pk, wl.ccs, [])
    ws.items = [dataclasses.replace(it, dev=None, pinned=None) for it in items]
    ws.to_device()
    g = SplitMix64(0x6D07)
    pows = [pow(wl.tau, i, r) for i in range(n + 3)]
    w = 2 * cv.fp_bytes
    jobs = []
    for lens in ((n + 3, 2049, 9, 1, n), (9, n + 3, n + 3, 2049, 2)):
        polys = [km.polynomial("random", L, r, g) for L in lens]
        zs = [g.fr(r) for _ in lens]
        wh, wv = b"", b""
        for f, z in zip(polys, zs):
            v = km.horner(f, z, r)
            k = (sum(c * p for c, p in zip(f, pows)) - v) * pow((wl.tau - z) % r, -1, r) % r
            wh += cv.g1_to_bytes(ov.mul(ov.g1, k)); wv += cv.fr_to_mont_bytes(v)
        bufs = [C.create_string_buffer(cv.fr_vector(f), 32 * len(f)) for f in polys]
        jobs.append((bufs, (C.c_void_p * 5)(*[C.addressof(b) for b in bufs]), (C.c_uint64 * 5)(*lens), cv.fr_vector(zs), wh, wv))
    errors, rounds = [], 6
    pk.paths(reset=True)

    def prover():
        pr = _lib.Proof()
        for _ in range(rounds):
            rc = ws.prove(0, pr, "device")
            if rc != 0 or base._marshal(pr) != want[0]:
                errors.append(("proof", rc, lib.apk_last_error()))

    def opener():
        h, v = C.create_string_buffer(5 * w), C.create_string_buffer(5 * 32)
        for t in range(rounds):
            _, ptrs, lens, zs, wh, wv = jobs[t % len(jobs)]
            rc = lib.apk_kzg_open_multi(pk.ctx, 5, ptrs, lens, zs, h, v)
            if rc != 0 or h.raw != wh or v.raw != wv:
                errors.append(("openings", t, rc, lib.apk_last_error()))

    threads = [threading.Thread(target=prover), threading.Thread(target=opener)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    pc = pk.paths()
    ws.close()
    pk.close()
    assert not errors, errors[:4]
    assert pc["proofs"] == rounds and pc["gang_proofs"] == 0 and pc["gang_kernel_launches"] == 0, pc


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", NAMES)
def test_argument_errors_leave_the_context_usable(gpu, cname, kind):
    R, M = base.rig(cname, gpu), model(cname, gpu)
    cv = R.cv
    ctx = R.ctx(kind)
    g = SplitMix64(0x6D08 + cv.abi)
    ARG = _lib.APK_ERR_ARG
    k, w = 33, 2 * cv.fp_bytes
    buf = C.create_string_buffer(cv.fr_vector([1] * (N + 4)), 32 * (N + 4))
    ptrs = (C.c_void_p * k)(*[C.addressof(buf)] * k)
    lens = (C.c_uint64 * k)(*[5] * k)
    zs, h, vals = cv.fr_vector([2] * k), C.create_string_buffer(w * k), C.create_string_buffer(32 * k)
    d = base._upload(ctx, buf.raw)
    dptrs = (C.c_void_p * k)(*[d.value] * k)
    good_poly, good_z = _poly(cname, base._shape()[1] + 1, g), _point(g, R)

    def lens_with(i, L):
        out = (C.c_uint64 * k)(*[5] * k)
        out[i] = L
        return out

    for fn, pp in ((lib.apk_kzg_open_multi, ptrs), (lib.apk_kzg_open_multi_device, dptrs)):
        assert fn(ctx, 0, pp, lens, zs, h, vals) == ARG
        assert fn(ctx, 33, pp, lens, zs, h, vals) == ARG
        assert fn(ctx, 5, pp, lens_with(3, 0), zs, h, vals) == ARG                  # a length of 0
        assert fn(ctx, 5, pp, lens_with(4, N + 4), zs, h, vals) == ARG              # a length above the SRS
        assert fn(ctx, 5, pp, lens_with(0, 1 << 40), zs, h, vals) == ARG
        holes = (C.c_void_p * 5)(pp[0], pp[0], None, pp[0], pp[0])
        assert fn(ctx, 5, holes, lens, zs, h, vals) == ARG                          # a null pointer among the polynomials
        assert fn(ctx, 5, pp, lens, zs, None, vals) == ARG                          # null outputs
        assert fn(ctx, 5, pp, lens, zs, h, None) == ARG
        assert fn(ctx, 5, None, lens, zs, h, vals) == ARG
        assert fn(ctx, 5, pp, None, zs, h, vals) == ARG
        assert fn(ctx, 5, pp, lens, None, h, vals) == ARG
        assert fn(None, 5, pp, lens, zs, h, vals) == ARG
        assert fn(ctx, 5, pp, lens_with(4, N + 3), zs, h, vals) == 0                # the longest the SRS takes
        # a valid call right afterwards on the same context: the model's bytes
        _check_multi(M, ctx, [good_poly] * 2, [good_z, good_z], "%s %s after the errors" % (cname, kind), single=False)
    assert lib.apk_kzg_open_multi_device(ctx, 5, ptrs, lens, zs, h, vals) == ARG     # host pointers are not device memory
    check(lib.apk_device_free(ctx, d))
    _check_multi(M, ctx, [good_poly], [good_z], "%s %s at the end" % (cname, kind), single=False)

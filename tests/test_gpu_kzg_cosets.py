"""GPU tier: apk_kzg_cosets_prepare / apk_kzg_open_cosets* (csrc/kernels_kzg_cosets.h, kzg_cosets_run.h) on circuit contexts of both
curves over a known-tau SRS, against the model H_i = [(f - I_i)(tau) / (tau^l - w^(i l))] G1 (tests/kzg_cosets_model.py) byte for
byte: every coset and every value at (n, l) = (8, 2), (8, 4) (n' = 2: one-term sequences, 2n' = 4), (128, 2) (the size-2n' stage is
exactly one workgroup), (128, 8), (128, 64) (n' = 2 with a full lane group), (512, 16), (512, 64), at seven lengths each;
structured polynomials that put infinity, zero scalars, equal and opposite terms into the pointwise sums; one larger sample at
(2048, 64) held to the model, to apk_kzg_open_all + apk_g1_lincomb_segments and to apk_kzg_verify_coset; the stage knob in fresh
processes; the prepare orders and states; scratch reuse; the call beside proofs; the Python mirror.  One model multiplication
costs a few milliseconds: every test stays below about 1 500 of them."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess
import sys
import threading

import pytest

import kzg_all_model as kam
import kzg_cosets_model as kcm
import kzg_model as km
from algoplonk_amd import _lib, batch, kzg as ap_kzg, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd._lib import check, lib
from helpers import CURVES, oracle_threads, random_chain_ccs
from oracle.prng import SplitMix64, tau_from_seed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254", "bls12-381"]
ARG, STATE, VERIFY = _lib.APK_ERR_ARG, _lib.APK_ERR_STATE, _lib.APK_ERR_VERIFY
SHAPES = [(3, 2), (3, 4), (7, 2), (7, 8), (7, 64), (9, 16), (9, 64)]      # (log n, l)
_RIG = {}


class Rig:
    """A circuit context of 2^log_n rows over a known-tau SRS, prepared for the openings on cosets of l points (l = 0: not)"""

    def __init__(self, cname, log_n, l, gpu, slots=1):
        self.cv, self.ov = CURVES[cname]
        cv = self.cv
        self.n, self.l = 1 << log_n, l
        self.np = self.n // l if l else 0
        self.tau = tau_from_seed(0xC0D + cv.abi + log_n, cv.r)
        self.srs = ap_setup.unsafe_srs(cv, self.n, self.tau, device=gpu)
        ccs, _, _ = random_chain_ccs(cv, log_n, 0xC0E)
        self.pk, _ = ap_plonk.Setup(ccs, self.srs, device=gpu, slots=slots)
        self.ctx = self.pk.ctx
        self.w = cv.omega(self.n)
        if l:
            check(lib.apk_kzg_cosets_prepare(self.ctx, self.srs.g1, self.n + 3, l))

    def model(self, f):
        """([H bytes] per coset, [value bytes] coset-major) of the model"""
        cv, ov, r = self.cv, self.ov, self.cv.r
        hs = kcm.direct(f, self.n, self.l, self.w, self.tau, r)
        vs = kcm.values_by_coset(f, self.n, self.l, self.w, r)
        return [cv.g1_to_bytes(ov.mul(ov.g1, k) if k else None) for k in hs], [cv.fr_to_mont_bytes(v) for v in vs]


def rig(cname, log_n, l, gpu) -> Rig:
    if (cname, log_n, l) not in _RIG:
        _RIG[(cname, log_n, l)] = Rig(cname, log_n, l, gpu)
    return _RIG[(cname, log_n, l)]


def _upload(ctx, buf):
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    return d


def _open(R, f, device=False, ctx=None, np=None):
    """(rc, [H bytes], [value bytes])"""
    cv, n = R.cv, R.n
    np = np or R.np
    ctx = ctx or R.ctx
    w = 2 * cv.fp_bytes
    h, vals = C.create_string_buffer(b"\xa5" * (w * np), w * np), C.create_string_buffer(b"\xa5" * (32 * n), 32 * n)
    buf = cv.fr_vector(f)
    if device:
        d = _upload(ctx, buf)
        rc = lib.apk_kzg_open_cosets_device(ctx, d, len(f), h, vals)
        check(lib.apk_device_free(ctx, d))
    else:
        rc = lib.apk_kzg_open_cosets(ctx, buf, len(f), h, vals)
    return rc, [h.raw[i * w:(i + 1) * w] for i in range(np)], [vals.raw[32 * i:32 * (i + 1)] for i in range(n)]


def _check(R, f, what, forms=(False, True)):
    want_h, want_v = R.model(f)
    for device in forms:
        rc, hs, vs = _open(R, f, device)
        assert rc == 0, (what, device, lib.apk_last_error())
        bad = [i for i in range(R.np) if hs[i] != want_h[i]]
        assert not bad, "%s (%s pointers): H differs from the model at %d cosets, first %s" % (what, "device" if device else "host", len(bad), bad[:8])
        bad = [i for i in range(R.n) if vs[i] != want_v[i]]
        assert not bad, "%s (%s pointers): values differ from the model at %s" % (what, "device" if device else "host", bad[:8])
    return want_h, want_v


LENGTHS = {"1": lambda n, l: 1, "l": lambda n, l: l, "l+1": lambda n, l: l + 1, "2l": lambda n, l: 2 * l, "n/2+1": lambda n, l: n // 2 + 1,
           "n-1": lambda n, l: n - 1, "n": lambda n, l: n}


@pytest.mark.parametrize("length", sorted(LENGTHS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_every_coset_against_the_model(gpu, cname, shape, length):
    R = rig(cname, shape[0], shape[1], gpu)
    L = LENGTHS[length](R.n, R.l)
    g = SplitMix64(0xC100 + 16 * shape[0] + shape[1] + L % 16 + R.cv.abi)
    f = km.polynomial("random", L, R.cv.r, g)
    want_h, _ = _check(R, f, "%s n=%d l=%d len %d" % (cname, R.n, R.l, L))
    if L <= R.l:
        assert not any(any(h) for h in want_h)


STRUCTURED = ["zero", "short", "X^l", "X^(n-1)", "vanishing", "class", "equal-8", "opposite-8", "equal-128", "opposite-128"]


@pytest.mark.parametrize("kind", STRUCTURED)
@pytest.mark.parametrize("cname", NAMES)
def test_structured_polynomials(gpu, cname, kind):
    cv, _ = CURVES[cname]
    r = cv.r
    g = SplitMix64(0xC130 + cv.abi)
    what = "%s %s" % (cname, kind)
    if kind.startswith(("equal", "opposite")):
        # l = 2: the two terms of output i* are equal, then opposite (tests/test_kzg_cosets_host.py holds the construction)
        log_n = 3 if kind.endswith("-8") else 7
        R = rig(cname, log_n, 2, gpu)
        n, w_2n = R.n, cv.omega(2 * R.n)
        i_star = 3 if n == 8 else 77
        t0, t1 = kcm.t_hat(n, 2, 0, w_2n, R.tau, r)[i_star], kcm.t_hat(n, 2, 1, w_2n, R.tau, r)[i_star]
        assert t0 and t1
        alpha = g.fr(r) or 1
        f3 = alpha * t0 % r * pow(t1, -1, r) % r
        f = [g.fr(r), g.fr(r), alpha, (-f3) % r if kind.startswith("opposite") else f3]
        a0 = kam.dft(kcm.sequences(f, n, 2, 0, R.tau, r)[0], pow(w_2n, 2, r), r)[i_star]
        a1 = kam.dft(kcm.sequences(f, n, 2, 1, R.tau, r)[0], pow(w_2n, 2, r), r)[i_star]
        assert a0 * t0 % r == ((-a1 * t1) % r if kind.startswith("opposite") else a1 * t1 % r) != 0
        _check(R, f, what)
        return
    R = rig(cname, 7, 8, gpu)
    n, l, np = R.n, R.l, R.np
    if kind in ("zero", "short"):
        f = [0] * n if kind == "zero" else [g.fr(r) for _ in range(l)] + [0] * (n // 2)      # (not the len <= l shortcut: the transforms run)
        for device in (False, True):
            rc, hs, vs = _open(R, f, device)
            assert rc == 0, lib.apk_last_error()
            assert not any(any(h) for h in hs), what
            assert vs == R.model(f)[1]
        return
    if kind == "X^l":
        f = [0] * l + [1]
        rc, hs, _ = _open(R, f)
        assert rc == 0 and hs == [cv.g1_to_bytes(cv.g1)] * np, what      # every H = s_0
    elif kind == "X^(n-1)":
        f = [0] * (n - 1) + [1]      # h_m = s_(n-1-l(m+1)): the index plan
    elif kind == "vanishing":
        i = 5
        f = [(-pow(R.w, i * l, r)) % r] + [0] * (l - 1) + [1]      # X^l - w^(i l)
    else:
        f = [0 if k % l == 3 else g.fr(r) for k in range(n)]      # a whole A^_c is zero
        assert kcm.sequences(f, n, l, 3, R.tau, r)[0] == [0] * (2 * np)
    _, want_v = _check(R, f, what)
    if kind == "vanishing":
        assert want_v[5 * l:6 * l] == [bytes(32)] * l


@pytest.mark.parametrize("cname", NAMES)
def test_larger_sample_at_2048(gpu, cname):
    """(2048, 64), n' = 32, a random f: all 32 proofs are the model's, the bytes apk_kzg_open_all + apk_g1_lincomb_segments give
    with the weights x_(i,j) / (l a_i), and accepted by apk_kzg_verify_coset - and rejected with two neighbouring H swapped."""
    R = rig(cname, 11, 64, gpu)
    cv, ov, r, n, l, np = R.cv, R.ov, R.cv.r, R.n, R.l, R.np
    g = SplitMix64(0xC140 + cv.abi)
    f = km.polynomial("random", n, r, g)
    want_h, want_v = R.model(f)
    for device in (False, True):
        rc, hs, vs = _open(R, f, device)
        assert rc == 0, lib.apk_last_error()
        assert hs == want_h and vs == want_v, (cname, device)
    # (b) the single-point openings, composed
    w = 2 * cv.fp_bytes
    check(lib.apk_kzg_all_prepare(R.ctx, R.srs.g1, n + 3))
    h1 = C.create_string_buffer(w * n)
    check(lib.apk_kzg_open_all(R.ctx, cv.fr_vector(f), n, h1, None))
    pts = b"".join(h1.raw[(i + np * j) * w:(i + np * j + 1) * w] for i in range(np) for j in range(l))
    seg = (C.c_uint64 * (np + 1))(*[i * l for i in range(np + 1)])
    out = C.create_string_buffer(w * np)
    check(lib.apk_g1_lincomb_segments(cv.abi, gpu, pts, cv.fr_vector(kcm.composition_weights(n, l, R.w, r)), seg, np, out))
    assert [out.raw[i * w:(i + 1) * w] for i in range(np)] == hs
    # (c) the verifier
    vk = km.kzg_vk(cv, R.srs.g2)
    g2_l = ap_setup.g2_from_tau(cv, pow(R.tau, l, r))[2 * w:4 * w]
    digest = cv.g1_to_bytes(ov.mul(ov.g1, km.horner(f, R.tau, r)))
    srs_l = bytes(R.srs.g1[:l * w])

    def verify(i, h):
        return lib.apk_kzg_verify_coset(C.byref(vk), g2_l, srs_l, n, l, i, digest, b"".join(vs[i * l:(i + 1) * l]), h)

    for i in range(np):
        assert verify(i, hs[i]) == 0, (i, lib.apk_last_error())
    assert verify(7, hs[8]) == VERIFY and verify(8, hs[7]) == VERIFY


_KNOB_CHILD = r"""
import ctypes as C, hashlib, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from algoplonk_amd import plonk as ap_plonk, setup as ap_setup
from algoplonk_amd._lib import check, lib
from helpers import CURVES, random_chain_ccs
from oracle.prng import SplitMix64, tau_from_seed
import kzg_model as km
out = []
for cname in ("bn254", "bls12-381"):
    cv, _ = CURVES[cname]
    n, l = 512, 16
    srs = ap_setup.unsafe_srs(cv, n, tau_from_seed(0xC150, cv.r), device=%(gpu)d)
    ccs, _, _ = random_chain_ccs(cv, 9, 0xC151)
    pk, _ = ap_plonk.Setup(ccs, srs, device=%(gpu)d)
    check(lib.apk_kzg_cosets_prepare(pk.ctx, srs.g1, n + 3, l))
    g = SplitMix64(0xC152)
    d = hashlib.sha256()
    for L in (n, n // 2 + 1, l + 1):
        f = km.polynomial("random", L, cv.r, g)
        w = 2 * cv.fp_bytes
        h, v = C.create_string_buffer(w * (n // l)), C.create_string_buffer(32 * n)
        check(lib.apk_kzg_open_cosets(pk.ctx, cv.fr_vector(f), L, h, v))
        d.update(h.raw); d.update(v.raw)
    out.append(d.hexdigest())
    pk.close()
print("DIGEST " + " ".join(out))
"""


def test_both_stage_forms_give_the_same_bytes(gpu):
    """APK_KZG_ALL_GLV = 0 (lagrange_stage_kernel over plain tables) and 1 (the split stage), each in a fresh process"""
    got = {}
    for knob in ("0", "1"):
        env = dict(os.environ, APK_KZG_ALL_GLV=knob)
        code = _KNOB_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "gpu": gpu}
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, (knob, r.stdout[-2000:], r.stderr[-3000:])
        got[knob] = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")][-1]
    assert got["0"] == got["1"] and len(got["0"].split()) == 3, got


def _open_all(R, f):
    w = 2 * R.cv.fp_bytes
    h, v = C.create_string_buffer(w * R.n), C.create_string_buffer(32 * R.n)
    check(lib.apk_kzg_open_all(R.ctx, R.cv.fr_vector(f), len(f), h, v))
    return h.raw, v.raw


@pytest.mark.parametrize("cname", NAMES)
def test_prepare_orders_and_states(gpu, cname):
    cv, _ = CURVES[cname]
    r = cv.r
    g = SplitMix64(0xC160 + cv.abi)
    # cosets first, then every point; and the other way round: the same bytes from both calls on both contexts
    A, B = Rig(cname, 5, 0, gpu), Rig(cname, 5, 0, gpu)
    n, l, w = A.n, 4, 2 * cv.fp_bytes
    A.l = B.l = l
    A.np = B.np = n // l
    f = km.polynomial("random", n, r, g)
    buf, h, vals = cv.fr_vector(f + [1]), C.create_string_buffer(w * n), C.create_string_buffer(32 * n)
    d = _upload(A.ctx, buf)
    # a call before prepare
    assert lib.apk_kzg_open_cosets(A.ctx, buf, n, h, vals) == STATE
    assert lib.apk_kzg_open_cosets_device(A.ctx, d, n, h, vals) == STATE
    # an MSM-only context has no domain
    msm = ap_kzg.MsmContext(cv, A.srs.g1, device=gpu)
    assert lib.apk_kzg_cosets_prepare(msm.ctx, A.srs.g1, n + 3, l) == STATE
    assert lib.apk_kzg_open_cosets(msm.ctx, buf, n, h, vals) == STATE
    msm.close()
    # too few SRS points, a size out of range; then the smallest SRS that will do
    assert lib.apk_kzg_cosets_prepare(A.ctx, A.srs.g1, n - l - 1, l) == ARG
    assert lib.apk_kzg_cosets_prepare(A.ctx, A.srs.g1, n + 3, n) == ARG
    assert lib.apk_kzg_cosets_prepare(A.ctx, A.srs.g1, n + 3, 3) == ARG
    assert lib.apk_kzg_open_cosets(A.ctx, buf, n, h, vals) == STATE
    assert lib.apk_kzg_cosets_prepare(A.ctx, A.srs.g1, n - l, l) == 0, lib.apk_last_error()
    check(lib.apk_kzg_all_prepare(A.ctx, A.srs.g1, n + 3))
    check(lib.apk_kzg_all_prepare(B.ctx, B.srs.g1, n + 3))
    all_before = _open_all(B, f)
    check(lib.apk_kzg_cosets_prepare(B.ctx, B.srs.g1, n + 3, l))
    assert _open_all(B, f) == all_before == _open_all(A, f)
    want = _check(A, f, "%s cosets before every point" % cname)
    assert _check(B, f, "%s cosets after every point" % cname) == want
    hs1, _ = kam.direct(f, n, A.w, A.tau, r), None
    assert all_before[0][:3 * w] == b"".join(cv.g1_to_bytes(A.ov.mul(A.ov.g1, k)) for k in hs1[:3])
    # prepare twice; another size
    assert lib.apk_kzg_cosets_prepare(A.ctx, A.srs.g1, n + 3, l) == 0
    assert lib.apk_kzg_cosets_prepare(A.ctx, A.srs.g1, n + 3, 2 * l) == STATE
    assert b"one coset size" in lib.apk_last_error()
    for fn, p in ((lib.apk_kzg_open_cosets, buf), (lib.apk_kzg_open_cosets_device, d)):
        assert fn(A.ctx, p, n + 1, h, vals) == ARG
        assert fn(A.ctx, p, 0, h, vals) == ARG
        assert fn(A.ctx, None, n, h, vals) == ARG
        assert fn(A.ctx, p, n, None, vals) == ARG
        assert fn(None, p, n, h, vals) == ARG
        assert fn(A.ctx, p, n, h, None) == 0, lib.apk_last_error()      # the values are optional
    assert lib.apk_kzg_open_cosets_device(A.ctx, buf, n, h, vals) == ARG     # host memory is not device memory
    check(lib.apk_device_free(A.ctx, d))
    _check(A, km.polynomial("random", n - 1, r, g), "%s after the errors" % cname)
    A.pk.close()
    B.pk.close()


@pytest.mark.parametrize("cname", NAMES)
def test_scratch_reuse(gpu, cname):
    """A full-length polynomial, then a short one on the same slot (the context has one): nothing of the first shows in the
    second, and the same call twice gives the same bytes."""
    R = rig(cname, 7, 8, gpu)
    g = SplitMix64(0xC170 + R.cv.abi)
    full, short = km.polynomial("random", R.n, R.cv.r, g), km.polynomial("random", R.l + 2, R.cv.r, g)
    rc, h1, v1 = _open(R, full)
    assert rc == 0
    _check(R, short, "%s short after full" % cname)
    rc, h2, v2 = _open(R, full, device=True)
    assert rc == 0 and (h2, v2) == (h1, v1)
    _check(R, short, "%s short after full, again" % cname, forms=(False,))


@pytest.mark.parametrize("cname", NAMES)
def test_coset_openings_beside_proofs(gpu, cname):
    """Two threads open every coset at n = 2^11, l = 64 while a third proves, on a three-slot context: every proof is the lone
    proof's blob (the C oracle's); every opening is, byte for byte, what the call returns alone, which is held to the model."""
    import test_gpu_kzg as base
    from bench_cpu import oracle_blobs
    cv, ov = CURVES[cname]
    r, l = cv.r, 64
    wl = workloads.random_circuit(cv, 11, 0xC180 + cv.abi)
    n = wl.ccs.domain_size()
    np = n // l
    srs = ap_setup.unsafe_srs(cv, n, wl.tau, device=gpu)
    items = batch.WitnessSet(None, wl.ccs, workloads.variants(wl, 1, 0xC181), curve=cv).items
    want = oracle_blobs(cv, wl.ccs, srs, items, threads=oracle_threads())
    pk, _ = ap_plonk.Setup(wl.ccs, srs, device=gpu, slots=3)
    ws = batch.WitnessSet(pk, wl.ccs, [])
    ws.items = [dataclasses.replace(it, dev=None, pinned=None) for it in items]
    ws.to_device()
    check(lib.apk_kzg_cosets_prepare(pk.ctx, srs.g1, n + 3, l))
    g = SplitMix64(0xC182)
    f = km.polynomial("random", n, r, g)
    w = 2 * cv.fp_bytes
    buf = cv.fr_vector(f)
    h0, v0 = C.create_string_buffer(w * np), C.create_string_buffer(32 * n)
    check(lib.apk_kzg_open_cosets(pk.ctx, buf, n, h0, v0))
    om = cv.omega(n)
    assert h0.raw == b"".join(cv.g1_to_bytes(ov.mul(ov.g1, k) if k else None) for k in kcm.direct(f, n, l, om, wl.tau, r))
    assert v0.raw[:32 * l] == b"".join(cv.fr_to_mont_bytes(km.horner(f, pow(om, (n // l) * j, r), r)) for j in range(l))
    errors, rounds = [], 4
    pk.paths(reset=True)

    def prover():
        pr = _lib.Proof()
        for _ in range(rounds):
            rc = ws.prove(0, pr, "device")
            if rc != 0 or base._marshal(pr) != want[0]:
                errors.append(("proof", rc, lib.apk_last_error()))

    def opener():
        h, v = C.create_string_buffer(w * np), C.create_string_buffer(32 * n)
        for t in range(rounds):
            rc = lib.apk_kzg_open_cosets(pk.ctx, buf, n, h, v)
            if rc != 0 or h.raw != h0.raw or v.raw != v0.raw:
                errors.append(("openings", t, rc, lib.apk_last_error()))

    threads = [threading.Thread(target=prover), threading.Thread(target=opener), threading.Thread(target=opener)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    pc = pk.paths()
    ws.close()
    pk.close()
    assert not errors, errors[:4]
    assert pc["proofs"] == rounds and pc["gang_proofs"] == 0 and pc["gang_kernel_launches"] == 0, pc


def test_python_mirror(gpu):
    R = rig("bn254", 7, 8, gpu)
    cv, r, n, l = R.cv, R.cv.r, R.n, R.l
    g = SplitMix64(0xC190)
    f = km.polynomial("random", n // 2 + 1, r, g)
    ap_kzg.PrepareCosets(R.pk, R.srs, l)      # (a second time: nothing changes)
    proofs = ap_kzg.OpenCosets(f, R.pk)
    assert len(proofs) == R.np
    want_h, want_v = R.model(f)
    assert [cv.g1_to_bytes(p.H) for p in proofs] == want_h
    assert [cv.fr_to_mont_bytes(v) for p in proofs for v in p.ClaimedValues] == want_v
    vk = ap_kzg.VerifyingKey(cv, cv.g1, R.srs.g2)
    digest = ap_kzg.Commit(f, R.pk)
    g2_l = ap_setup.g2_from_tau(cv, pow(R.tau, l, r))[4 * cv.fp_bytes:]
    for i in (0, 5, R.np - 1):
        ap_kzg.VerifyCoset(digest, proofs[i], i, l, vk, g2_l, R.srs)
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.VerifyCoset(digest, proofs[4], 5, l, vk, g2_l, R.srs)
    with pytest.raises(_lib.ApkError):
        ap_kzg.PrepareCosets(R.pk, R.srs, 2 * l)
    with pytest.raises(ValueError):
        ap_kzg.OpenCosets([1] * (n + 1), R.pk)

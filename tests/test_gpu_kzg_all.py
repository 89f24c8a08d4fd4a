"""GPU tier: apk_kzg_all_prepare / apk_kzg_open_all* (csrc/kernels_kzg_all.h, kzg_all_run.h) on circuit contexts of both curves over
a known-tau SRS, against the model H_i = [(f(tau) - f(w^i)) / (tau - w^i)] G1 byte for byte: every i at n = 8 (2n is a quarter of
a wave), 128 (the size-2n stage is exactly one workgroup) and 512, at every length; structured polynomials that put infinity,
equal and opposite operands into the transforms; a sampled compare at n = 2048 against the model, apk_kzg_open_multi and the
multi-point verifier; the stage knob in fresh processes; scratch reuse; states and errors; openings beside proofs; the Python
mirror.  One model multiplication costs a few milliseconds: every test stays below about 1 500 of them."""
from __future__ import annotations

import ctypes as C
import dataclasses
import hashlib
import os
import subprocess
import sys
import threading

import pytest

import kzg_all_model as kam
import kzg_model as km
from algoplonk_amd import _lib, batch, kzg as ap_kzg, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd._lib import check, lib
from helpers import CURVES, oracle_threads, random_chain_ccs
from oracle.prng import SplitMix64, tau_from_seed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254", "bls12-381"]
ARG, STATE = _lib.APK_ERR_ARG, _lib.APK_ERR_STATE
_RIG = {}


class Rig:
    """A circuit context of 2^log_n rows over a known-tau SRS, prepared for the openings at every point"""

    def __init__(self, cname, log_n, gpu, prepare=True):
        self.cv, self.ov = CURVES[cname]
        cv = self.cv
        self.n = 1 << log_n
        self.tau = tau_from_seed(0xA11D + cv.abi + log_n, cv.r)
        self.srs = ap_setup.unsafe_srs(cv, self.n, self.tau, device=gpu)
        ccs, _, _ = random_chain_ccs(cv, log_n, 0xA11E)
        self.pk, _ = ap_plonk.Setup(ccs, self.srs, device=gpu)
        self.ctx = self.pk.ctx
        self.w = cv.omega(self.n)
        if prepare:
            check(lib.apk_kzg_all_prepare(self.ctx, self.srs.g1, self.n + 3))

    def model(self, f, indices=None):
        """([H bytes], [value bytes]) of the model at w^i for i in indices (default: every i)"""
        cv, ov, r = self.cv, self.ov, self.cv.r
        ft = km.horner(f, self.tau, r)
        hs, vs = [], []
        for i in (range(self.n) if indices is None else indices):
            z = pow(self.w, i, r)
            v = km.horner(f, z, r)
            k = (ft - v) * pow((self.tau - z) % r, -1, r) % r
            hs.append(cv.g1_to_bytes(ov.mul(ov.g1, k) if k else None))
            vs.append(cv.fr_to_mont_bytes(v))
        return hs, vs


def rig(cname, log_n, gpu) -> Rig:
    if (cname, log_n) not in _RIG:
        _RIG[(cname, log_n)] = Rig(cname, log_n, gpu)
    return _RIG[(cname, log_n)]


def _upload(ctx, buf):
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    return d


def _open_all(R, f, device=False, ctx=None):
    """(rc, [H bytes], [value bytes])"""
    cv, n = R.cv, R.n
    ctx = ctx or R.ctx
    w = 2 * cv.fp_bytes
    h, vals = C.create_string_buffer(b"\xa5" * (w * n), w * n), C.create_string_buffer(b"\xa5" * (32 * n), 32 * n)
    buf = cv.fr_vector(f)
    if device:
        d = _upload(ctx, buf)
        rc = lib.apk_kzg_open_all_device(ctx, d, len(f), h, vals)
        check(lib.apk_device_free(ctx, d))
    else:
        rc = lib.apk_kzg_open_all(ctx, buf, len(f), h, vals)
    return rc, [h.raw[i * w:(i + 1) * w] for i in range(n)], [vals.raw[32 * i:32 * (i + 1)] for i in range(n)]


def _check_all(R, f, what, forms=(False, True)):
    want_h, want_v = R.model(f)
    for device in forms:
        rc, hs, vs = _open_all(R, f, device)
        assert rc == 0, (what, device, lib.apk_last_error())
        bad = [i for i in range(R.n) if hs[i] != want_h[i]]
        assert not bad, "%s (%s pointers): H differs from the model at %d indices, first %s" % (what, "device" if device else "host", len(bad), bad[:8])
        bad = [i for i in range(R.n) if vs[i] != want_v[i]]
        assert not bad, "%s (%s pointers): values differ from the model at %s" % (what, "device" if device else "host", bad[:8])
    return want_h, want_v


LENGTHS = {"1": lambda n: 1, "2": lambda n: 2, "3": lambda n: 3, "n/2+1": lambda n: n // 2 + 1, "n-1": lambda n: n - 1, "n": lambda n: n}


@pytest.mark.parametrize("length", sorted(LENGTHS))
@pytest.mark.parametrize("log_n", [3, 7, 9])
@pytest.mark.parametrize("cname", NAMES)
def test_every_opening_against_the_model(gpu, cname, log_n, length):
    R = rig(cname, log_n, gpu)
    L = LENGTHS[length](R.n)
    g = SplitMix64(0xA120 + 16 * log_n + L % 16 + R.cv.abi)
    f = km.polynomial("random", L, R.cv.r, g)
    want_h, _ = _check_all(R, f, "%s n=%d len %d" % (cname, R.n, L))
    if L == 1:
        assert not any(any(h) for h in want_h)


STRUCTURED = ["zero", "constant", "X", "X^(n-1)", "X+X^(n/2+1)", "roots", "equal", "opposite"]


@pytest.mark.parametrize("kind", STRUCTURED)
@pytest.mark.parametrize("cname", NAMES)
def test_structured_polynomials(gpu, cname, kind):
    R = rig(cname, 7, gpu)
    cv, r, n = R.cv, R.cv.r, R.n
    g = SplitMix64(0xA130 + cv.abi)
    what = "%s %s" % (cname, kind)
    if kind in ("zero", "constant"):
        f = [0] * n if kind == "zero" else [g.fr(r)] + [0] * (n // 2)      # (not the len = 1 shortcut: the transforms run)
        for device in (False, True):
            rc, hs, vs = _open_all(R, f, device)
            assert rc == 0, lib.apk_last_error()
            assert not any(any(h) for h in hs), what
            assert vs == [cv.fr_to_mont_bytes(f[0])] * n
        return
    if kind == "X":
        f = [0, 1]
        rc, hs, _ = _open_all(R, f)
        assert rc == 0 and hs == [cv.g1_to_bytes(cv.g1)] * n, what      # every H = s_0
    elif kind == "X^(n-1)":
        f = [0] * (n - 1) + [1]      # h_k = s_(n-2-k): the index plan
    elif kind == "X+X^(n/2+1)":
        f = [0] * (n // 2 + 2)
        f[1] = f[n // 2 + 1] = 1
        a, _ = kam.sequences(f, n, R.tau, r)
        assert kam.dft(a, cv.omega(2 * n), r).count(0) == n // 2      # a quarter of A^ is zero: infinity operands in the transform
    elif kind == "roots":
        f = km.polynomial("random", n - 2, r, g)
        for i in (3, 70):
            z0 = pow(R.w, i, r)
            f = [(a - z0 * b) % r for a, b in zip([0] + f, f + [0])]
        assert km.horner(f, pow(R.w, 70, r), r) == 0 and len(f) == n
    else:
        tail = [g.fr(r) for _ in range(n - 1 - n // 2)]
        f = kam.meeting_points(n, R.tau, r, tail, kind == "opposite")
        h = kam.h_terms(f, n, R.tau, r)
        assert h[0] == (-h[n // 2] % r if kind == "opposite" else h[n // 2]) != 0
    _, want_v = _check_all(R, f, what)
    if kind == "roots":
        assert want_v[3] == want_v[70] == bytes(32)


@pytest.mark.parametrize("cname", NAMES)
def test_sampled_compare_at_2048(gpu, cname):
    """32 indices of a whole-domain opening at n = 2048: the model's bytes, apk_kzg_open_multi's at those w^i, accepted by ONE
    pairing check against the commitment - and rejected with two neighbouring H swapped."""
    R = rig(cname, 11, gpu)
    cv, ov, r, n = R.cv, R.ov, R.cv.r, R.n
    g = SplitMix64(0xA140 + cv.abi)
    f = km.polynomial("random", n, r, g)
    idx = {0, 1, n // 2, n - 1}
    while len(idx) < 32:
        idx.add(g.below(n))
    idx = sorted(idx)
    want_h, want_v = R.model(f, idx)
    for device in (False, True):
        rc, hs, vs = _open_all(R, f, device)
        assert rc == 0, lib.apk_last_error()
        assert [hs[i] for i in idx] == want_h and [vs[i] for i in idx] == want_v, (cname, device)
    # apk_kzg_open_multi on the same polynomial at those points
    k, w = 32, 2 * cv.fp_bytes
    buf = C.create_string_buffer(cv.fr_vector(f), 32 * n)
    ptrs = (C.c_void_p * k)(*[C.addressof(buf)] * k)
    zs = [pow(R.w, i, r) for i in idx]
    mh, mv = C.create_string_buffer(w * k), C.create_string_buffer(32 * k)
    check(lib.apk_kzg_open_multi(R.ctx, k, ptrs, (C.c_uint64 * k)(*[n] * k), cv.fr_vector(zs), mh, mv))
    assert mh.raw == b"".join(hs[i] for i in idx) and mv.raw == b"".join(vs[i] for i in idx)
    # one pairing check for the 32
    vk = km.kzg_vk(cv, R.srs.g2)
    digest = cv.g1_to_bytes(ov.mul(ov.g1, km.horner(f, R.tau, r)))
    for device in (-1, gpu):
        assert lib.apk_kzg_batch_verify_multi(C.byref(vk), device, k, digest * k, cv.fr_vector(zs), mv.raw, mh.raw) == 0, lib.apk_last_error()
        swapped = [hs[i] for i in idx]
        swapped[7], swapped[8] = swapped[8], swapped[7]
        assert lib.apk_kzg_batch_verify_multi(C.byref(vk), device, k, digest * k, cv.fr_vector(zs), mv.raw, b"".join(swapped)) == _lib.APK_ERR_VERIFY


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
    n = 512
    srs = ap_setup.unsafe_srs(cv, n, tau_from_seed(0xA150, cv.r), device=%(gpu)d)
    ccs, _, _ = random_chain_ccs(cv, 9, 0xA151)
    pk, _ = ap_plonk.Setup(ccs, srs, device=%(gpu)d)
    check(lib.apk_kzg_all_prepare(pk.ctx, srs.g1, n + 3))
    g = SplitMix64(0xA152)
    d = hashlib.sha256()
    for L in (n, n // 2 + 1, 2):
        f = km.polynomial("random", L, cv.r, g)
        w = 2 * cv.fp_bytes
        h, v = C.create_string_buffer(w * n), C.create_string_buffer(32 * n)
        check(lib.apk_kzg_open_all(pk.ctx, cv.fr_vector(f), L, h, v))
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
        got[knob] = [l for l in r.stdout.splitlines() if l.startswith("DIGEST ")][-1]
    assert got["0"] == got["1"] and len(got["0"].split()) == 3, got


@pytest.mark.parametrize("cname", NAMES)
def test_scratch_reuse(gpu, cname):
    """A full-length polynomial, then a short one on the same slot (the context has one): nothing of the first shows in the
    second, and the same call twice gives the same bytes."""
    R = rig(cname, 7, gpu)
    g = SplitMix64(0xA160 + R.cv.abi)
    full, short = km.polynomial("random", R.n, R.cv.r, g), km.polynomial("random", 3, R.cv.r, g)
    rc, h1, v1 = _open_all(R, full)
    assert rc == 0
    _check_all(R, short, "%s short after full" % cname)
    rc, h2, v2 = _open_all(R, full, device=True)
    assert rc == 0 and (h2, v2) == (h1, v1)
    _check_all(R, short, "%s short after full, again" % cname, forms=(False,))


@pytest.mark.parametrize("cname", NAMES)
def test_states_and_errors(gpu, cname):
    cv, _ = CURVES[cname]
    R = Rig(cname, 5, gpu, prepare=False)
    n, w = R.n, 2 * cv.fp_bytes
    f = [1] * (n + 1)
    buf, h, vals = cv.fr_vector(f), C.create_string_buffer(w * n), C.create_string_buffer(32 * n)
    d = _upload(R.ctx, buf)
    # before prepare
    assert lib.apk_kzg_open_all(R.ctx, buf, n, h, vals) == STATE
    assert lib.apk_kzg_open_all_device(R.ctx, d, n, h, vals) == STATE
    # an MSM-only context has no domain
    msm = ap_kzg.MsmContext(cv, R.srs.g1, device=gpu)
    assert lib.apk_kzg_all_prepare(msm.ctx, R.srs.g1, n + 3) == STATE
    assert lib.apk_kzg_open_all(msm.ctx, buf, n, h, vals) == STATE
    msm.close()
    # too few SRS points; then prepare, twice
    assert lib.apk_kzg_all_prepare(R.ctx, R.srs.g1, n - 2) == ARG
    assert lib.apk_kzg_open_all(R.ctx, buf, n, h, vals) == STATE
    assert lib.apk_kzg_all_prepare(R.ctx, R.srs.g1, n - 1) == 0, lib.apk_last_error()
    assert lib.apk_kzg_all_prepare(R.ctx, R.srs.g1, n + 3) == 0
    for fn, p in ((lib.apk_kzg_open_all, buf), (lib.apk_kzg_open_all_device, d)):
        assert fn(R.ctx, p, n + 1, h, vals) == ARG
        assert fn(R.ctx, p, 0, h, vals) == ARG
        assert fn(R.ctx, None, n, h, vals) == ARG
        assert fn(R.ctx, p, n, None, vals) == ARG
        assert fn(None, p, n, h, vals) == ARG
        assert fn(R.ctx, p, n, h, None) == 0, lib.apk_last_error()      # the values are optional
    assert lib.apk_kzg_open_all_device(R.ctx, buf, n, h, vals) == ARG     # host memory is not device memory
    check(lib.apk_device_free(R.ctx, d))
    # the context is usable after the errors (prepared over n - 1 points: all the call reads)
    _check_all(R, km.polynomial("random", n, cv.r, SplitMix64(0xA170)), "%s after the errors" % cname)
    R.pk.close()


@pytest.mark.parametrize("cname", NAMES)
def test_whole_domain_openings_beside_proofs_on_two_slots(gpu, cname):
    """One thread opens the whole domain at n = 2^11 while another proves, on a two-slot context: every proof is the lone proof's
    blob (the C oracle's); every opening is, byte for byte, what the call returns alone, which is held to the model at 32 indices."""
    import test_gpu_kzg as base
    from bench_cpu import oracle_blobs
    cv, ov = CURVES[cname]
    r = cv.r
    wl = workloads.random_circuit(cv, 11, 0xA180 + cv.abi)
    n = wl.ccs.domain_size()
    srs = ap_setup.unsafe_srs(cv, n, wl.tau, device=gpu)
    items = batch.WitnessSet(None, wl.ccs, workloads.variants(wl, 1, 0xA181), curve=cv).items
    want = oracle_blobs(cv, wl.ccs, srs, items, threads=oracle_threads())
    pk, _ = ap_plonk.Setup(wl.ccs, srs, device=gpu, slots=2)
    ws = batch.WitnessSet(pk, wl.ccs, [])
    ws.items = [dataclasses.replace(it, dev=None, pinned=None) for it in items]
    ws.to_device()
    check(lib.apk_kzg_all_prepare(pk.ctx, srs.g1, n + 3))
    g = SplitMix64(0xA182)
    f = km.polynomial("random", n, r, g)
    w = 2 * cv.fp_bytes
    buf = cv.fr_vector(f)
    h0, v0 = C.create_string_buffer(w * n), C.create_string_buffer(32 * n)
    check(lib.apk_kzg_open_all(pk.ctx, buf, n, h0, v0))
    ft, om = km.horner(f, wl.tau, r), cv.omega(n)
    for i in sorted({0, 1, n // 2, n - 1} | {g.below(n) for _ in range(28)}):
        z = pow(om, i, r)
        v = km.horner(f, z, r)
        H = ov.mul(ov.g1, (ft - v) * pow((wl.tau - z) % r, -1, r) % r)
        assert h0.raw[i * w:(i + 1) * w] == cv.g1_to_bytes(H) and v0.raw[32 * i:32 * (i + 1)] == cv.fr_to_mont_bytes(v), i
    errors, rounds = [], 4
    pk.paths(reset=True)

    def prover():
        pr = _lib.Proof()
        for _ in range(rounds):
            rc = ws.prove(0, pr, "device")
            if rc != 0 or base._marshal(pr) != want[0]:
                errors.append(("proof", rc, lib.apk_last_error()))

    def opener():
        h, v = C.create_string_buffer(w * n), C.create_string_buffer(32 * n)
        for t in range(rounds):
            rc = lib.apk_kzg_open_all(pk.ctx, buf, n, h, v)
            if rc != 0 or h.raw != h0.raw or v.raw != v0.raw:
                errors.append(("openings", t, rc, lib.apk_last_error()))

    threads = [threading.Thread(target=prover), threading.Thread(target=opener)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    pc = pk.paths()
    ws.close()
    pk.close()
    assert not errors, errors[:4]
    assert pc["proofs"] == rounds and pc["gang_proofs"] == 0 and pc["gang_kernel_launches"] == 0, pc


def test_python_mirror(gpu):
    R = rig("bn254", 7, gpu)
    cv, r, n = R.cv, R.cv.r, R.n
    g = SplitMix64(0xA190)
    f = km.polynomial("random", n // 2 + 1, r, g)
    ap_kzg.PrepareAllDomain(R.pk, R.srs)      # (a second time: nothing changes)
    proofs = ap_kzg.OpenAllDomain(f, R.pk)
    assert len(proofs) == n
    want_h, want_v = R.model(f)
    assert [cv.g1_to_bytes(p.H) for p in proofs] == want_h and [cv.fr_to_mont_bytes(p.ClaimedValue) for p in proofs] == want_v
    for i in (0, 5, n - 1):
        assert proofs[i] == ap_kzg.Open(f, pow(R.w, i, r), R.pk)
    vk = ap_kzg.VerifyingKey(cv, cv.g1, R.srs.g2)
    digest = ap_kzg.Commit(f, R.pk)
    idx = list(range(0, n, n // 32))
    ap_kzg.BatchVerifyMultiPoints([digest] * 32, [proofs[i] for i in idx], [pow(R.w, i, r) for i in idx], vk)
    with pytest.raises(ValueError):
        ap_kzg.OpenAllDomain([1] * (n + 1), R.pk)

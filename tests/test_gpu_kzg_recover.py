"""GPU tier: apk_kzg_recover_cosets* (csrc/kernels_kzg_recover.h, kzg_recover_run.h) on circuit contexts of both curves.  The
input cells are what apk_kzg_open_cosets on the same context returned for a seeded random polynomial; the expected output is that
polynomial's own bytes and apk_kzg_recover_cosets_host's (held to the big-integer model in tests/test_kzg_recover_host.py) - neither
is the code under test.  Shapes (log n, l): (3, 2); (3, 4) (n' = 2: k is 1 or 2); (7, 2); (7, 64) (n' = 2 with full rows); (9, 16);
(10, 2) (n' = 512: more roots than one LDS tile and more than one workgroup in the vanish kernel, m up to 511).  Per shape, with host
and device pointers: all cells, one cell, exactly ceil(len / l) cells (the first, the last, the even ones, a seeded random set), rows
shuffled, len in {1, l, k l - 1, k l}.  Then structured polynomials and arbitrary rows against the model; the verdict with the
destination untouched and the slot reusable; the round trip through RecoverCosetsAndProofs and the batched verifier; contexts that
never ran apk_kzg_cosets_prepare, two coset sizes on one context, an MSM-only context; the call beside proofs; the Python mirror."""
from __future__ import annotations

import ctypes as C
import dataclasses
import threading

import pytest

import kzg_model as km
import kzg_recover_model as krm
from algoplonk_amd import _lib, batch, kzg as ap_kzg, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd._lib import check, lib
from helpers import CURVES, oracle_threads, random_chain_ccs
from oracle.prng import SplitMix64, tau_from_seed

pytestmark = pytest.mark.gpu

NAMES = ["bn254", "bls12-381"]
ARG, STATE, VERIFY = _lib.APK_ERR_ARG, _lib.APK_ERR_STATE, _lib.APK_ERR_VERIFY
SHAPES = [(3, 2), (3, 4), (7, 2), (7, 64), (9, 16), (10, 2)]      # (log n, l)
_RIG = {}


class Rig:
    """A circuit context of 2^log_n rows over a known-tau SRS, prepared for the openings on cosets of l points (l = 0: not)"""

    def __init__(self, cname, log_n, l, gpu, slots=1):
        self.cv, self.ov = CURVES[cname]
        cv = self.cv
        self.n, self.l = 1 << log_n, l
        self.np = self.n // l if l else 0
        self.tau = tau_from_seed(0xEC0D + cv.abi + log_n, cv.r)
        self.srs = ap_setup.unsafe_srs(cv, self.n, self.tau, device=gpu)
        ccs, _, _ = random_chain_ccs(cv, log_n, 0xEC0E)
        self.pk, _ = ap_plonk.Setup(ccs, self.srs, device=gpu, slots=slots)
        self.ctx = self.pk.ctx
        self.w = cv.omega(self.n)
        self._cells = {}
        if l:
            ap_kzg.PrepareCosets(self.pk, self.srs, l)

    def cells(self, f):
        """([H bytes], [row bytes]) per coset: what apk_kzg_open_cosets returns for f, once per polynomial"""
        key = tuple(f)
        if key not in self._cells:
            w = 2 * self.cv.fp_bytes
            h, vals = C.create_string_buffer(w * self.np), C.create_string_buffer(32 * self.n)
            check(lib.apk_kzg_open_cosets(self.ctx, self.cv.fr_vector(f), len(f), h, vals))
            rb = 32 * self.l
            self._cells[key] = ([h.raw[i * w:(i + 1) * w] for i in range(self.np)], [vals.raw[i * rb:(i + 1) * rb] for i in range(self.np)])
        return self._cells[key]


def rig(cname, log_n, l, gpu) -> Rig:
    if (cname, log_n, l) not in _RIG:
        _RIG[(cname, log_n, l)] = Rig(cname, log_n, l, gpu)
    return _RIG[(cname, log_n, l)]


def _upload(ctx, buf):
    d = C.c_void_p()
    check(lib.apk_device_alloc(ctx, len(buf), C.byref(d)))
    check(lib.apk_device_upload(ctx, d, buf, len(buf)))
    return d


def _recover(ctx, l, known, rows, length, device=False):
    """(rc, the destination's bytes - pre-filled with 0xa5); rows: the bytes of each row"""
    k = len(known)
    idx = (C.c_uint64 * k)(*known)
    buf, mark = b"".join(rows), b"\xa5" * (32 * length)
    if not device:
        out = C.create_string_buffer(mark, len(mark))
        return lib.apk_kzg_recover_cosets(ctx, l, k, idx, buf, length, out), out.raw
    d_rows, d_out = _upload(ctx, buf), _upload(ctx, mark)
    rc = lib.apk_kzg_recover_cosets_device(ctx, l, k, idx, d_rows, length, d_out)
    out = C.create_string_buffer(len(mark))
    check(lib.apk_device_download(ctx, out, d_out, len(mark)))
    check(lib.apk_device_free(ctx, d_rows))
    check(lib.apk_device_free(ctx, d_out))
    return rc, out.raw


def _host(cv, n, l, known, rows, length):
    k = len(known)
    out = C.create_string_buffer(32 * length)
    rc = lib.apk_kzg_recover_cosets_host(cv.abi, n, l, k, (C.c_uint64 * k)(*known), b"".join(rows), length, out)
    return rc, out.raw


def _shuffled(xs, g):
    xs = list(xs)
    for i in range(len(xs) - 1, 0, -1):
        j = g.next() % (i + 1)
        xs[i], xs[j] = xs[j], xs[i]
    return xs


def _cases(np, l, g):
    """(name, known cosets in row order, len): all cells; one cell where len <= l; exactly ceil(len / l) cells"""
    out = []
    for length in sorted({1, l, np * l - 1, np * l}):
        out.append(("all", _shuffled(range(np), g), length))
    for k in sorted({1, max(np // 2, 1), np - 1}):
        sets = {"first": list(range(k)), "last": list(range(np - k, np)), "random": sorted(_shuffled(range(np), g)[:k])}
        if 2 * k == np:
            sets["even"] = list(range(0, np, 2))
        for name, known in sets.items():
            for length in sorted({k * l - 1, k * l} | ({1, l} if k == 1 else set())):
                if length >= 1 and -(-length // l) == k:
                    out.append(("%s-%d" % (name, k), known, length))
                    out.append(("%s-%d shuffled" % (name, k), _shuffled(known, g), length))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_recover_from_the_cells_the_opening_returned(gpu, cname, shape):
    R = rig(cname, shape[0], shape[1], gpu)
    cv, n, l, np = R.cv, R.n, R.l, R.np
    g = SplitMix64(0xEC10 + 16 * shape[0] + l + cv.abi)
    f_full = km.polynomial("random", n, cv.r, g)
    cases = _cases(np, l, g)
    assert {c[0].split()[0].split("-")[0] for c in cases} >= {"all", "first", "last", "random", "even"}
    assert max(np - len(c[1]) for c in cases) == np - 1 and min(np - len(c[1]) for c in cases) == 0      # m from 0 to n' - 1
    hosted = set()
    for name, known, length in cases:
        f = f_full[:length]
        want = cv.fr_vector(f)
        _, cells = R.cells(f)
        rows = [cells[i] for i in known]
        what = "%s n=%d l=%d %s len %d" % (cname, n, l, name, length)
        for device in (False, True):
            rc, got = _recover(R.ctx, l, known, rows, length, device)
            assert rc == 0, (what, device, lib.apk_last_error())
            assert got == want, "%s (%s pointers): differs from the polynomial that was opened" % (what, "device" if device else "host")
        if n <= 512 or name.split()[0] not in hosted:      # (the host form is quadratic in n' on ONE thread: once per set at n' = 512)
            hosted.add(name.split()[0])
            assert _host(cv, n, l, known, rows, length) == (0, want), what


STRUCTURED = ["zero", "top", "zero-row"]


@pytest.mark.parametrize("kind", STRUCTURED)
@pytest.mark.parametrize("cname", NAMES)
def test_structured_polynomials(gpu, cname, kind):
    R = rig(cname, 9, 16, gpu)
    cv, r, n, l, np = R.cv, R.cv.r, R.n, R.l, R.np
    known = [30, 3, 7, 0, 31, 12, 13, 21]
    kl = len(known) * l
    if kind == "zero":
        f = [0] * kl
    elif kind == "top":
        f = [0] * (kl - 1) + [1]                                      # X^(k l - 1)
    else:
        f = [(-pow(R.w, 7 * l, r)) % r] + [0] * (l - 1) + [1]         # X^l - a_7: it vanishes on the known coset 7
        f += [0] * (kl - len(f))
    _, cells = R.cells(f)
    if kind == "zero-row":
        assert cells[7] == bytes(32 * l) and all(any(cells[i]) for i in known if i != 7)
    rows = [cells[i] for i in known]
    for device in (False, True):
        assert _recover(R.ctx, l, known, rows, kl, device) == (0, cv.fr_vector(f)), (cname, kind, device, lib.apk_last_error())
    assert _host(cv, n, l, known, rows, kl) == (0, cv.fr_vector(f))
    if kind != "top":      # the same with the length the polynomial has
        short = 1 if kind == "zero" else l + 1
        assert _recover(R.ctx, l, known, rows, short, True) == (0, cv.fr_vector(f[:short]))


@pytest.mark.parametrize("shape", [(3, 2), (7, 8)], ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_arbitrary_rows_against_the_model(gpu, cname, shape):
    """Rows that are no polynomial's cells, on a context that never ran apk_kzg_cosets_prepare: the k l coefficients are the
    model's - the polynomial below degree k l through the points - and a destination of n coefficients (the widest the rules admit,
    with all cells) shows nothing above."""
    R = rig(cname, shape[0], 0, gpu)
    cv, r, n, l = R.cv, R.cv.r, R.n, shape[1]
    np = n // l
    g = SplitMix64(0xEC20 + shape[0] + cv.abi)
    for known in ([np - 1], _shuffled(range(np), g)[:np // 2], _shuffled(range(np), g)[:np - 1], _shuffled(range(np), g)):
        vals = [[g.fr(r) for _ in range(l)] for _ in known]
        rows = [cv.fr_vector(v) for v in vals]
        kl = len(known) * l
        want = krm.steps(n, l, known, vals, R.w, cv.coset_shift, r)
        assert not any(want[kl:])
        for device in (False, True):
            assert _recover(R.ctx, l, known, rows, kl, device) == (0, cv.fr_vector(want[:kl])), (cname, shape, known, device, lib.apk_last_error())
        assert _host(cv, n, l, known, rows, kl) == (0, cv.fr_vector(want[:kl]))


@pytest.mark.parametrize("cname", NAMES)
def test_verdict_leaves_the_destination_and_the_slot_as_they_were(gpu, cname):
    R = rig(cname, 9, 16, gpu)
    cv, n, l, np = R.cv, R.n, R.l, R.np
    g = SplitMix64(0xEC30 + cv.abi)
    known = _shuffled(range(np), g)[:np // 2]
    kl = len(known) * l
    f = km.polynomial("random", kl - 1, cv.r, g) + [g.fr(cv.r) or 1]
    _, cells = R.cells(f)
    rows = [cells[i] for i in known]
    mark = b"\xa5" * (32 * (kl - 1))
    for device in (False, True):
        assert _recover(R.ctx, l, known, rows, kl - 1, device) == (VERIFY, mark), (cname, device)
        assert b"not those of one polynomial" in lib.apk_last_error()
        # the very next call on the same slot (the context has one)
        assert _recover(R.ctx, l, known, rows, kl, device) == (0, cv.fr_vector(f)), (cname, device, lib.apk_last_error())
    # one changed value in a row of a shorter polynomial
    f2 = f[:kl - l]
    _, cells2 = R.cells(f2)
    rows2 = [cells2[i] for i in known]
    assert _recover(R.ctx, l, known, rows2, kl - l, True) == (0, cv.fr_vector(f2))
    bad = list(rows2)
    bad[3] = bad[3][:32] + cv.fr_vector([1 + cv.fr_vector_decode(bad[3][32:64])[0]]) + bad[3][64:]
    assert _recover(R.ctx, l, known, bad, kl - l, True) == (VERIFY, b"\xa5" * (32 * (kl - l)))
    assert _host(cv, n, l, known, bad, kl - l)[0] == VERIFY


@pytest.mark.parametrize("shape", [(9, 16), (11, 64)], ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_round_trip_through_recover_cosets_and_proofs(gpu, cname, shape):
    """open, drop half of the cells, RecoverCosetsAndProofs: all n' proofs and values are the direct opening's bytes, and
    apk_kzg_batch_verify_cosets accepts the recovered set"""
    R = rig(cname, shape[0], shape[1], gpu)
    cv, r, n, l, np = R.cv, R.cv.r, R.n, R.l, R.np
    g = SplitMix64(0xEC40 + shape[0] + cv.abi)
    f = km.polynomial("random", n // 2, r, g)
    want_h, want_rows = R.cells(f)
    direct = ap_kzg.OpenCosets(f, R.pk)
    kept = sorted(_shuffled(range(np), g)[:np // 2])
    got = ap_kzg.RecoverCosetsAndProofs(kept, [direct[i] for i in kept], l, n // 2, R.pk)
    assert len(got) == np
    assert [cv.g1_to_bytes(p.H) for p in got] == want_h
    assert [cv.fr_vector(p.ClaimedValues) for p in got] == want_rows
    vk = ap_kzg.VerifyingKey(cv, cv.g1, R.srs.g2)
    g2_l = ap_setup.g2_from_tau(cv, pow(R.tau, l, r))[4 * cv.fp_bytes:]
    digest = ap_kzg.Commit(f, R.pk)
    ap_kzg.BatchVerifyCosets([digest], [0] * np, list(range(np)), got, l, vk, g2_l, R.srs, n=n, device=gpu)
    swapped = list(got)
    swapped[1], swapped[2] = swapped[2], swapped[1]
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.BatchVerifyCosets([digest], [0] * np, list(range(np)), swapped, l, vk, g2_l, R.srs, n=n, device=gpu)


@pytest.mark.parametrize("cname", NAMES)
def test_states_and_argument_rules_on_a_context(gpu, cname):
    R = rig(cname, 7, 0, gpu)      # never prepared for openings
    cv, r, n = R.cv, R.cv.r, R.n
    g = SplitMix64(0xEC50 + cv.abi)
    f = km.polynomial("random", n // 2, r, g)
    # two coset sizes on one context, one after the other (a larger n' second: the scratch grows), and the first again
    for l in (8, 2, 8):
        np = n // l
        cs = krm.cells(f, n, l, R.w, r)
        known = _shuffled(range(np), g)[:np // 2]
        rows = [cv.fr_vector(cs[i]) for i in known]
        for device in (False, True):
            assert _recover(R.ctx, l, known, rows, n // 2, device) == (0, cv.fr_vector(f)), (cname, l, device, lib.apk_last_error())
    l, np = 8, n // 8
    rows = [cv.fr_vector(c) for c in krm.cells(f, n, l, R.w, r)]
    buf = b"".join(rows) + bytes(32 * l)
    out = C.create_string_buffer(32 * (n + 1))
    d_rows, d_out = _upload(R.ctx, buf), _upload(R.ctx, out.raw)

    def call(fn=lib.apk_kzg_recover_cosets, ctx=R.ctx, l=l, idx=tuple(range(8)), rows=buf, length=64, out=out):
        return fn(ctx, l, len(idx), (C.c_uint64 * max(len(idx), 1))(*idx), rows, length, out)

    for fn, rw, o in ((lib.apk_kzg_recover_cosets, buf, out), (lib.apk_kzg_recover_cosets_device, d_rows, d_out)):
        kw = dict(fn=fn, rows=rw, out=o)
        assert call(**kw) == 0, lib.apk_last_error()
        assert call(idx=tuple(range(np)), length=n, **kw) == 0                  # count = n'
        assert call(idx=tuple(range(np + 1)), length=n, **kw) == ARG            # count = n' + 1
        assert call(length=65, **kw) == ARG and b"too few cells" in lib.apk_last_error() and b"need 9 cells" in lib.apk_last_error()
        assert call(idx=(0, np - 1), length=16, **kw) == 0                      # index = n' - 1
        assert call(idx=(0, np), length=16, **kw) == ARG                        # index = n'
        assert call(idx=(3, 5, 3), length=16, **kw) == ARG                      # a repeated index
        assert call(l=1, **kw) == ARG and call(l=n, idx=(0,), length=1, **kw) == ARG and call(l=3, **kw) == ARG
        assert call(l=n // 2, idx=(1,), length=n // 2, **kw) == 0               # l = n / 2
        assert call(idx=(), **kw) == ARG and call(length=0, **kw) == ARG
        assert call(ctx=None, **kw) == ARG
    assert call(fn=lib.apk_kzg_recover_cosets_device, rows=buf, out=d_out) == ARG          # host memory is not device memory
    assert call(fn=lib.apk_kzg_recover_cosets_device, rows=d_rows, out=out) == ARG
    check(lib.apk_device_free(R.ctx, d_rows))
    check(lib.apk_device_free(R.ctx, d_out))
    # an MSM-only context has no domain
    msm = ap_kzg.MsmContext(cv, R.srs.g1, device=gpu)
    assert call(ctx=msm.ctx) == STATE
    msm.close()
    assert call() == 0, lib.apk_last_error()


@pytest.mark.parametrize("cname", NAMES)
def test_recovery_beside_proofs(gpu, cname):
    """Two threads recover while two others prove, on a four-slot context at n = 2^9, l = 16: every proof is the lone proof's blob
    (the C oracle's), every recovery the polynomial, byte for byte; the recoveries join no gang."""
    import test_gpu_kzg as base
    from bench_cpu import oracle_blobs
    cv, _ = CURVES[cname]
    r, l = cv.r, 16
    wl = workloads.random_circuit(cv, 9, 0xEC60 + cv.abi)
    n = wl.ccs.domain_size()
    np = n // l
    srs = ap_setup.unsafe_srs(cv, n, wl.tau, device=gpu)
    items = batch.WitnessSet(None, wl.ccs, workloads.variants(wl, 2, 0xEC61), curve=cv).items
    want = oracle_blobs(cv, wl.ccs, srs, items, threads=oracle_threads())
    pk, _ = ap_plonk.Setup(wl.ccs, srs, device=gpu, slots=4)
    ws = batch.WitnessSet(pk, wl.ccs, [])
    ws.items = [dataclasses.replace(it, dev=None, pinned=None) for it in items]
    ws.to_device()
    g = SplitMix64(0xEC62)
    f = km.polynomial("random", n // 2, r, g)
    cs = krm.cells(f, n, l, cv.omega(n), r)
    sets = [sorted(_shuffled(range(np), g)[:np // 2]) for _ in range(2)]
    rows = [[cv.fr_vector(cs[i]) for i in known] for known in sets]
    want_f = cv.fr_vector(f)
    for t in range(2):
        assert _recover(pk.ctx, l, sets[t], rows[t], n // 2) == (0, want_f), lib.apk_last_error()
    errors, rounds = [], 4
    pk.paths(reset=True)

    def prover(t):
        pr = _lib.Proof()
        for _ in range(rounds):
            rc = ws.prove(t, pr, "device")
            if rc != 0 or base._marshal(pr) != want[t]:
                errors.append(("proof", t, rc, lib.apk_last_error()))

    def recoverer(t):
        for i in range(rounds):
            rc, got = _recover(pk.ctx, l, sets[t], rows[t], n // 2, device=bool(i & 1))
            if rc != 0 or got != want_f:
                errors.append(("recovery", t, i, rc, lib.apk_last_error()))

    threads = [threading.Thread(target=prover, args=(0,)), threading.Thread(target=prover, args=(1,)), threading.Thread(target=recoverer, args=(0,)),
               threading.Thread(target=recoverer, args=(1,))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    pc = pk.paths()
    ws.close()
    pk.close()
    assert not errors, errors[:4]
    assert pc["proofs"] == 2 * rounds, pc


def test_python_mirror(gpu):
    R = rig("bn254", 9, 16, gpu)
    cv, r, n, l, np = R.cv, R.cv.r, R.n, R.l, R.np
    g = SplitMix64(0xEC70)
    f = km.polynomial("random", n // 2 - 3, r, g)
    proofs = ap_kzg.OpenCosets(f, R.pk)
    kept = _shuffled(range(np), g)[:np // 2]
    assert ap_kzg.RecoverCosets(kept, [proofs[i] for i in kept], l, len(f), R.pk) == f
    assert ap_kzg.RecoverCosets(kept, [proofs[i].ClaimedValues for i in kept], l, n // 2, R.pk) == f + [0] * 3
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.RecoverCosets(kept, [proofs[i] for i in kept], l, len(f) - 1, R.pk)
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.RecoverCosetsAndProofs(kept, [proofs[i] for i in kept], l, len(f) - 1, R.pk)
    with pytest.raises(_lib.ApkError):
        ap_kzg.RecoverCosets(kept[:-1] + kept[:1], [proofs[i] for i in kept], l, len(f), R.pk)      # a repeated index
    with pytest.raises(ValueError):
        ap_kzg.RecoverCosets(kept, [proofs[i] for i in kept], l, n // 2 + 1, R.pk)
    again = ap_kzg.RecoverCosetsAndProofs(kept, [proofs[i] for i in kept], l, len(f), R.pk)
    assert [(cv.g1_to_bytes(p.H), p.ClaimedValues) for p in again] == [(cv.g1_to_bytes(p.H), p.ClaimedValues) for p in proofs]

"""GPU tier of the batched coset verifier (include/apk.h apk_kzg_cosets_fold, apk_kzg_batch_verify_cosets; csrc/kernels_kzg_cosets_fold.h):
the fold kernel against the host fold byte for byte at the row counts where its lane map can go wrong - one row, one row short of a
tile, a full tile, one row past it, a second grid-stride pass with a ragged last tile, the coset sizes 2, 64, 512, 1 024 and (the
host interpolation behind the device path) 2 048 - with structured weights, values and indices in the first rows; weights that
cancel; the rule on the rows apk_kzg_open_cosets returns at (128, 8), (512, 64) and (2048, 64), one and two polynomials, with device
0 and device -1; the host tier's rejections with device 0; points off the curve and off the subgroup through the device check; the
pooled buffer's reuse; the Python mirror."""
from __future__ import annotations

import ctypes as C

import pytest

import kzg_model as km
from algoplonk_amd import _lib, kzg as ap_kzg, setup as ap_setup
from algoplonk_amd._lib import lib
from helpers import CURVES
from oracle import curves as ocurves
from oracle.prng import SplitMix64
from test_gpu_kzg_cosets import _open, rig

pytestmark = pytest.mark.gpu

NAMES = ["bn254", "bls12-381"]
OK, ERR_ARG, ERR_VERIFY = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_VERIFY
# (l, n, count): rows per tile = 1024 / l
FOLDS = [(2, 1 << 20, 1), (2, 1 << 20, 511), (2, 1 << 20, 512), (2, 1 << 20, 513),
         (64, 1 << 20, 1), (64, 1 << 20, 15), (64, 1 << 20, 17), (64, 1 << 20, 16 * 256 + 1),
         (512, 1 << 20, 1), (512, 1 << 20, 3), (1024, 4096, 1), (1024, 1 << 20, 257), (2048, 8192, 3)]


def u32s(xs):
    return (C.c_uint32 * len(xs))(*xs)


def u64s(xs):
    return (C.c_uint64 * len(xs))(*xs)


def fold(cv, device, n, l, indices, weights: bytes, values: bytes):
    out = C.create_string_buffer(b"\xa5" * (32 * l), 32 * l)
    rc = lib.apk_kzg_cosets_fold(cv.abi, device, n, l, len(indices), u64s(indices), weights, values, out)
    assert rc == OK, (device, lib.apk_last_error())
    return out.raw


def fold_rows(cv, n, l, count, seed):
    """(indices, weights, values) as the call takes them.  Any integer below r is a canonical Montgomery residue, so the random
    rows are drawn as bytes; the first rows are the host tier's structured ones: weights 1, 0, r - 1, values random, zeros, r - 1,
    indices n / l - 1, 0, n / l - 1."""
    r, np = cv.r, n // l
    g = SplitMix64(seed)
    raw = lambda: g.fr(r).to_bytes(32, "little")
    indices = [[np - 1, 0, np - 1][k] if k < 3 else g.fr(r) % np for k in range(count)]
    weights = b"".join(cv.fr_vector([[1, 0, r - 1][k]]) if k < 3 and count > 1 else raw() for k in range(count))
    rows = []
    for k in range(count):
        if k == 1:
            rows.append(bytes(32 * l))
        elif k == 2:
            rows.append(cv.fr_vector([r - 1]) * l)
        else:
            rows.append(b"".join(raw() for _ in range(l)))
    return indices, weights, b"".join(rows)


@pytest.mark.parametrize("shape", FOLDS, ids=lambda s: "l%d-n%d-rows%d" % s)
@pytest.mark.parametrize("cname", NAMES)
def test_fold_on_the_device_gives_the_hosts_bytes(gpu, cname, shape):
    cv, _ = CURVES[cname]
    l, n, count = shape
    indices, weights, values = fold_rows(cv, n, l, count, 0xF0D0 + cv.abi + l + count)
    want = fold(cv, -1, n, l, indices, weights, values)
    assert fold(cv, gpu, n, l, indices, weights, values) == want
    assert any(want)


@pytest.mark.parametrize("l", [2, 64, 1024])
@pytest.mark.parametrize("cname", NAMES)
def test_equal_rows_under_weights_that_cancel_fold_to_zero(gpu, cname, l):
    cv, _ = CURVES[cname]
    r, n = cv.r, 1 << 14
    count = 2 * (1024 // l) + 1                                    # three tiles, the last one ragged
    g = SplitMix64(0xF0D1 + cv.abi + l)
    row = b"".join(g.fr(r).to_bytes(32, "little") for _ in range(l))
    ws = [g.fr(r) for _ in range(count - 1)]
    ws.append((-sum(ws)) % r)
    for device in (-1, gpu):
        assert fold(cv, device, n, l, [n // l - 1] * count, cv.fr_vector(ws), row * count) == bytes(32 * l), device


# ---- the rule on the rows apk_kzg_open_cosets returns ------------------------------------------------------------------------------------
class Opened:
    """Two polynomials opened on every coset by the GPU, the key and [tau^l]G2 for the rig's tau"""

    def __init__(self, cname, log_n, l, gpu):
        R = self.R = rig(cname, log_n, l, gpu)
        cv, ov, r = R.cv, R.ov, R.cv.r
        self.cv, self.ov, self.n, self.l, self.np = cv, ov, R.n, l, R.np
        g = SplitMix64(0xF0D2 + cv.abi + log_n + l)
        w = 4 * cv.fp_bytes
        g2 = ap_setup.g2_from_tau(cv, R.tau)
        self.vk = km.kzg_vk(cv, g2)
        self.g2_l = ap_setup.g2_from_tau(cv, pow(R.tau, l, r))[w:2 * w]
        self.g2_half = ap_setup.g2_from_tau(cv, pow(R.tau, l // 2, r))[w:2 * w]
        self.srs = bytes(R.srs.g1[:l * 2 * cv.fp_bytes])
        self.digests, self.rows = [], []
        for p in range(2):
            f = [g.fr(r) for _ in range(R.n - p)]
            rc, hs, vs = _open(R, f)
            assert rc == OK, lib.apk_last_error()
            self.digests.append(cv.g1_to_bytes(km.commit(ov, f, R.tau)))
            self.rows.append([(p, i, b"".join(vs[i * l:(i + 1) * l]), hs[i]) for i in range(R.np)])

    def both(self):
        return [self.rows[p][i if p == 0 else self.np - 1 - i] for i in range(self.np) for p in (0, 1)]

    def verify(self, rows, device, digests=None, g2_tau_l=None):
        digests = self.digests[:1 + max(r[0] for r in rows)] if digests is None else digests
        return lib.apk_kzg_batch_verify_cosets(C.byref(self.vk), device, g2_tau_l or self.g2_l, self.srs, self.n, self.l, len(digests),
                                               b"".join(digests), len(rows), u32s([r[0] for r in rows]), u64s([r[1] for r in rows]),
                                               b"".join(r[2] for r in rows), b"".join(r[3] for r in rows))


_OPENED = {}


def opened(cname, log_n, l, gpu) -> Opened:
    if (cname, log_n, l) not in _OPENED:
        _OPENED[(cname, log_n, l)] = Opened(cname, log_n, l, gpu)
    return _OPENED[(cname, log_n, l)]


@pytest.mark.parametrize("shape", [(7, 8), (9, 64), (11, 64)], ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_opened_rows_are_accepted_on_the_device_and_on_the_host(gpu, cname, shape):
    o = opened(cname, shape[0], shape[1], gpu)
    for device in (gpu, -1):
        assert o.verify(o.rows[0], device) == OK, (device, lib.apk_last_error())
        assert o.verify(o.both(), device) == OK, (device, lib.apk_last_error())
    # a second call reuses the pooled buffer
    assert o.verify(o.both(), gpu) == OK
    bad = list(o.rows[0])
    v = bytearray(bad[o.np // 2][2])
    v[32 * (o.l - 1)] ^= 1
    bad[o.np // 2] = (0, o.np // 2, bytes(v), bad[o.np // 2][3])
    assert o.verify(bad, gpu) == ERR_VERIFY and o.verify(bad, gpu) == ERR_VERIFY
    assert o.verify(o.rows[0], gpu) == OK


def _shift(cv, ov, h: bytes, k: int) -> bytes:
    """H + [k]G1"""
    return cv.g1_to_bytes(ov.add(cv.g1_from_bytes(h), ov.mul(ov.g1, k % cv.r)))


def _outside_subgroup(cv, ov):
    x = 1
    while True:      # the first x with a point on the curve: with a cofactor of ~2^126 such a point is outside the subgroup
        x += 1
        y = ocurves.sqrt_mod((x ** 3 + 4) % cv.p, cv.p)
        if y is not None and ov.add(ov.mul((x, y), cv.r - 1), (x, y)) is not None:
            return (x, y)


@pytest.mark.parametrize("cname", NAMES)
def test_the_host_tiers_rejections_on_the_device(gpu, cname):
    o = opened(cname, 7, 8, gpu)
    cv, ov, np, l = o.cv, o.ov, o.np, o.l
    rows, both = o.rows[0], o.both()

    def changed(rs, k, **kw):
        out = list(rs)
        d = dict(zip(("digest_of", "index", "values", "h"), out[k]), **kw)
        out[k] = (d["digest_of"], d["index"], d["values"], d["h"])
        return out

    v = bytearray(both[5][2])
    v[0] ^= 1
    cases = {
        "one changed value": changed(both, 5, values=bytes(v)),
        "two rows' H swapped": changed(changed(rows, 0, h=rows[np - 1][3]), np - 1, h=rows[0][3]),
        "a row pointing at the other polynomial": changed(both, 1, digest_of=0),
        "an index off by one": changed(rows, np - 1, index=np - 2),
        "H + P and H - P in two copies of a row": [changed(rows, 0, h=_shift(cv, ov, rows[0][3], 5))[0], changed(rows, 0, h=_shift(cv, ov, rows[0][3], -5))[0]],
    }
    for what, rs in cases.items():
        for device in (gpu, -1):
            assert o.verify(rs, device) == ERR_VERIFY, (what, device)
            assert b"do not verify" in lib.apk_last_error(), what
    assert o.verify(rows, gpu, g2_tau_l=o.g2_half) == ERR_VERIFY
    assert o.verify([rows[0], rows[0]], gpu) == OK
    # a proof moved off the curve, a digest moved off the curve: the device's check, and the message says which kind
    off = bytearray(rows[3][3])
    off[0] ^= 1
    assert o.verify(changed(rows, 3, h=bytes(off)), gpu) == ERR_VERIFY and b"proof is not a point" in lib.apk_last_error()
    off = bytearray(o.digests[0])
    off[0] ^= 1
    assert o.verify(rows, gpu, digests=[bytes(off)]) == ERR_VERIFY and b"digest is not a point" in lib.apk_last_error()
    if cname == "bls12-381":
        P = cv.g1_to_bytes(_outside_subgroup(cv, ov))
        assert o.verify(changed(rows, np - 1, h=P), gpu) == ERR_VERIFY and b"proof is not a point" in lib.apk_last_error()
        assert o.verify(changed(rows, np - 1, h=P), -1) == ERR_VERIFY and b"proof is not a point" in lib.apk_last_error()
    # the argument errors still come first
    assert o.verify(changed(rows, 0, index=np), gpu) == ERR_ARG
    assert o.verify(rows, gpu) == OK


def test_python_mirror(gpu):
    R = rig("bn254", 7, 8, gpu)
    cv, r = R.cv, R.cv.r
    o = opened("bn254", 7, 8, gpu)
    R.pk.kzg_coset_size = 8
    g = SplitMix64(0xF0D3)
    f = [g.fr(r) for _ in range(R.n)]
    proofs = ap_kzg.OpenCosets(f, R.pk)
    digest = km.commit(R.ov, f, R.tau)
    vk = ap_kzg.VerifyingKey(cv, cv.g1, ap_setup.g2_from_tau(cv, R.tau))
    idx = list(range(R.np))
    for device in (gpu, -1):
        ap_kzg.BatchVerifyCosets([digest], [0] * R.np, idx, proofs, 8, vk, o.g2_l, R.srs, n=R.n, device=device)
    proofs[3].ClaimedValues[2] = (proofs[3].ClaimedValues[2] + 1) % r
    with pytest.raises(ap_kzg.VerificationError):
        ap_kzg.BatchVerifyCosets([digest], [0] * R.np, idx, proofs, 8, vk, o.g2_l, R.srs, n=R.n, device=gpu)

"""CPU tier: the big-integer model of the G1 point kernels (tests/point_model.py) held to the oracle's own encoder, to the
rejections tests/test_gpu_setup.py pins on the device, to the reference's known answers and to the closed form of L_i(tau), so
that the GPU tests built on it (tests/test_gpu_point_kernels.py) cannot pass vacuously."""
from __future__ import annotations

import json
import os

import pytest

import point_model as pm
from helpers import CURVES
from oracle.prng import SplitMix64, tau_from_seed

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("cname", list(CURVES))
def test_accepts_inverts_the_oracle_encoder(cname):
    cv, ov = CURVES[cname]
    g = SplitMix64(0x90D)
    pts = [None, ov.g1, ov.neg(ov.g1)] + [ov.mul(ov.g1, g.fr(cv.r)) for _ in range(200)]
    for P in pts:
        enc = ov.compress(P)
        assert pm.accepts(ov, enc) == P == ov.decompress(enc)
        if P is not None:
            assert pm.accepts(ov, pm.wrong_sign(ov, P)) == ov.neg(P)


def test_accepts_rejects_what_the_device_test_rejects():
    """The four BLS12-381 encodings of test_decompress_rejects_what_gnark_rejects, built the same way, and BN254's flags 00."""
    cv, ov = CURVES["bls12-381"]
    p = cv.p
    x = 5
    while True:                                   # a point of E(Fp) that is NOT in the order-r subgroup
        rhs = (x * x * x + 4) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p == rhs and ov.add(ov.mul((x, y), cv.r - 1), (x, y)) is not None:
            break
        x += 1
    off_subgroup = ov.compress((x, y))
    inf_payload = bytes([0xC0]) + bytes(46) + b"\x01"
    too_big = bytes([0x9F]) + b"\xff" * 47
    x2 = 5
    while pow((x2 ** 3 + 4) % p, (p - 1) // 2, p) == 1:
        x2 += 1
    not_on_curve = bytes([0x80 | (x2.to_bytes(48, "big")[0])]) + x2.to_bytes(48, "big")[1:]
    for bad in (off_subgroup, inf_payload, too_big, not_on_curve):
        assert pm.accepts(ov, bad) is pm.REJECT, bad.hex()
    assert pm.accepts(ov, ov.compress(None)) is None
    assert pm.accepts(ov, ov.compress(ov.mul(ov.g1, 12345))) == ov.mul(ov.g1, 12345)
    cb, ob = CURVES["bn254"]
    okb = ob.compress(ob.mul(ob.g1, 777))
    assert pm.accepts(ob, okb) == ob.mul(ob.g1, 777)
    assert pm.accepts(ob, bytes([okb[0] & 0x3F]) + okb[1:]) is pm.REJECT


def test_accepts_decodes_the_reference_known_answers():
    """setup/trusted_setup_test.go:172-288: every hex string decodes to a point of G1 that compresses back to it."""
    cv, ov = CURVES["bls12-381"]
    kat = json.load(open(os.path.join(G, "trusted_setup_kat.json")))
    hexes = kat["dusk_g1_first5"] + [kat["dusk_g1_32767"]] + kat["ethereum_g1_first5"] + [kat["ethereum_g1_32767"]]
    for h in hexes:
        P = pm.accepts(ov, bytes.fromhex(h))
        assert P not in (None, pm.REJECT) and ov.is_on_curve(P) and ov.compress(P).hex() == h
        assert P[0] == int(h, 16) & pm.payload_mask(ov)
    assert pm.accepts(ov, bytes.fromhex(kat["ethereum_g1_first5"][0])) == ov.g1


@pytest.mark.parametrize("cname", list(CURVES))
def test_flag_patterns_and_range(cname):
    cv, ov = CURVES[cname]
    x = ov.g1[0]
    ok = {f for f in pm.flag_patterns(ov) if pm.accepts(ov, pm.encode(ov, f, x)) is not pm.REJECT}
    assert ok == ({0b100, 0b101} if cname == "bls12-381" else {0b10, 0b11})
    assert {pm.accepts(ov, pm.encode(ov, f, x)) for f in ok} == {ov.g1, ov.neg(ov.g1)}
    inf = [f for f in pm.flag_patterns(ov) if pm.accepts(ov, pm.encode(ov, f, 0)) is None]
    assert inf == ([0b110] if cname == "bls12-381" else [0b01])
    assert pm.accepts(ov, pm.encode(ov, inf[0], 1)) is pm.REJECT
    assert pm.accepts(ov, pm.encode(ov, inf[0], (pm.payload_mask(ov) + 1) >> 1)) is pm.REJECT
    # [p, mask] is not empty on either curve, and nothing in it decodes
    small = min(ok)
    assert cv.p <= pm.payload_mask(ov)
    for xx in (cv.p, cv.p + 1, pm.payload_mask(ov)):
        assert pm.accepts(ov, pm.encode(ov, small, xx)) is pm.REJECT
    # x = p + 1 WOULD decode if it were reduced first (x = 1 is on BN254; on BLS12-381 the subgroup check refuses it anyway)
    if cname == "bn254":
        assert pm.accepts(ov, pm.encode(ov, small, 1)) not in (None, pm.REJECT)


@pytest.mark.parametrize("cname", list(CURVES))
def test_boundary_of_the_sign_compare(cname):
    cv, ov = CURVES[cname]
    p, h = cv.p, (cv.p - 1) // 2
    for a in (8, 27, 5, h):
        for x in pm.cube_roots(a, p):
            assert pow(x, 3, p) == a % p
    assert len(pm.cube_roots(8, p)) == 3 and 2 in pm.cube_roots(8, p)
    # no point has y = (p-1)/2 on either curve (point_model.boundary_point's docstring)
    assert pow((h * h - ov.b) % p, (p - 1) // 3, p) != 1
    assert pm.boundary_point(ov) is None
    below, above = pm.near_boundary(ov)
    assert ov.is_on_curve(below) and ov.is_on_curve(above)
    assert 0 <= h - below[1] < 1 << 12 and 0 < above[1] - h <= 1 << 12
    assert below[1] >> 32 == h >> 32 == above[1] >> 32            # they differ from the boundary in the lowest word only
    if cname == "bn254":
        assert pm.accepts(ov, ov.compress(below)) == below and pm.accepts(ov, ov.compress(above)) == above
        assert ov.compress(below)[0] >> 6 == 0b10 and ov.compress(above)[0] >> 6 == 0b11
        assert pm.accepts(ov, pm.wrong_sign(ov, below)) == ov.neg(below)
    else:
        assert pm.accepts(ov, ov.compress(below)) is pm.REJECT     # on the curve, outside G1


@pytest.mark.parametrize("cname", list(CURVES))
@pytest.mark.parametrize("n", [2, 8, 64])
def test_lagrange_of_powers_of_tau_is_the_closed_form(cname, n):
    """a_j = tau^j: c_i = L_i(tau) = omega^i (tau^n - 1) / (n (tau - omega^i)), as test_to_lagrange_matches_known_tau has it."""
    cv, ov = CURVES[cname]
    r, w = cv.r, ov.omega(n)
    tau = tau_from_seed(9, r)
    got = pm.lagrange_of([pow(tau, j, r) for j in range(n)], n, r, w)
    zn = (pow(tau, n, r) - 1) * pow(n, -1, r) % r
    for i in range(n):
        wi = pow(w, i, r)
        assert got[i] == wi * zn % r * pow(tau - wi, -1, r) % r


@pytest.mark.parametrize("cname", list(CURVES))
def test_lagrange_of_arbitrary_and_degenerate_inputs(cname):
    cv, ov = CURVES[cname]
    r, n = cv.r, 16
    w = ov.omega(n)
    g = SplitMix64(0x1A6)
    a = [g.fr(r) for _ in range(n)]
    c = pm.lagrange_of(a, n, r, w)
    for k in range(n):                            # evaluating the outputs at omega^k gives the inputs back
        assert sum(c[i] * pow(w, i * k, r) for i in range(n)) % r == a[k]
    assert pm.lagrange_of([1] + [0] * (n - 1), n, r, w) == [pow(n, -1, r)] * n
    assert pm.lagrange_of([1] * n, n, r, w) == [1] + [0] * (n - 1)
    for k in (1, n - 1):
        assert pm.lagrange_of([pow(w, k * j, r) for j in range(n)], n, r, w) == [int(i == k) for i in range(n)]
    assert pm.lagrange_of([0] * n, n, r, w) == [0] * n
    assert pm.lagrange_points(ov, [1] * 4, 4) == [ov.g1, None, None, None]

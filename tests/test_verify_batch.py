"""CPU tier: apk_verify_batch / apk_g1_lincomb_segments with device = -1 (the folds on the host, one pairing check per batch)
against apk_verify, the oracle's transcribed verifier and a plain-Python restatement of the batch statement
(tests/verify_batch_material.py).  Nothing here needs a GPU."""
import ctypes as C
import hashlib

import pytest

from algoplonk_amd import _lib, setup as ap_setup
from algoplonk_amd._lib import lib
from oracle import plonk as oplonk
from oracle.prng import SplitMix64, tau_from_seed

from helpers import CURVES
import verify_batch_material as vbm

OK, BAD = _lib.APK_OK, _lib.APK_ERR_VERIFY
CNAMES = ["bn254", "bls12-381"]
PLAIN = ["pyth", "id", "sq", "rnd"]


def _mutations(cv, opr, k):
    """tests/test_verify_host.py:115-129 (and :150-153 for the BSB22 circuits): name -> edit of (proof, public inputs)"""
    def first_g1(p, pub): C.memmove(p.lro[0], bytes(p.lro[1]), 96)
    def scalar(p, pub): C.memmove(p.claimed_values[2], cv.fr_to_mont_bytes((opr.claimed_values[2] + 1) % cv.r), 32)
    def opening(p, pub): C.memmove(p.zshift_h, bytes(p.batched_h), 96)
    def off_curve(p, pub): p.z[0] ^= 1
    def public(p, pub): pub[0] = (pub[0] + 1) % cv.r
    muts = {"first_g1": first_g1, "scalar": scalar, "opening": opening, "off_curve": off_curve, "public": public}
    if k:
        muts["bsb_point"] = lambda p, pub: C.memmove(p.bsb22[k - 1], bytes(p.lro[0]), 96)
        muts["qcp_value"] = lambda p, pub: C.memmove(p.claimed_values[6], cv.fr_to_mont_bytes(7), 32)
    return muts


def restate(m, oprs, pubs, unreadable=()):
    """The batch statement of include/apk.h restated from hashlib, oracle/curves.py arithmetic and the challenge code of
    oracle/plonk.py::verify (its trace gives zeta, gamma', [lin], lin(zeta) and the folded claim of every proof): D, rho_j and
    [lin]_j of the first four proofs, A and B, in the trace's encodings.  Proofs in `unreadable` (sizes that do not match the key)
    enter D as a marker byte 0 and nothing else, and take no part in the fold."""
    ov, q = m.ov, m.ov.r
    vk = m.ovk
    rb, fb = ov.raw_bytes, oplonk.fr_bytes
    N = len(oprs)
    h = hashlib.sha256()
    for P in [vk.ql, vk.qr, vk.qm, vk.qo, vk.qk, vk.s[0], vk.s[1], vk.s[2]] + list(vk.qcp) + [vk.g1]:
        h.update(rb(P))
    h.update(N.to_bytes(4, "big"))
    for j, (opr, pub) in enumerate(zip(oprs, pubs)):
        if j in unreadable:
            h.update(b"\x00")
            continue
        h.update(b"\x01")
        for P in list(opr.lro) + [opr.z] + list(opr.h) + [opr.batched_h, opr.zshift_h] + list(opr.bsb22_commitments):
            h.update(rb(P))
        for v in list(opr.claimed_values[1:]) + [opr.zshift_value] + list(pub):
            h.update(fb(v))
    D = h.digest()
    rho = [1] + [int.from_bytes(hashlib.sha256(b"apk-batch" + D + j.to_bytes(4, "big")).digest()[16:], "big") for j in range(1, N)]
    A, B, lins = None, None, []
    for j, (opr, pub) in enumerate(zip(oprs, pubs)):
        if j in unreadable:
            lins.append(bytes(2 * m.cv.fp_bytes))
            continue
        T = {}
        assert oplonk.verify(vk, oplonk.marshal_proof(ov, opr), oplonk.marshal_public_inputs(pub), trace_out=T)
        zeta, gk, c, lin_raw = T["zeta"], T["gamma_kzg"], T["folded_claims"], T["lin_poly_com"]
        lins.append(lin_raw)
        zw = opr.zshift_value
        rr = int.from_bytes(hashlib.sha256(b"random" + fb(gk) + rb(opr.z) + rb(opr.batched_h) + rb(opr.zshift_h) + fb(c) + fb(zw)).digest(), "big") % q
        Aj, g = ov.from_raw_bytes(lin_raw), gk
        for P in list(opr.lro) + [vk.s[0], vk.s[1]] + list(vk.qcp):
            Aj = ov.add(Aj, ov.mul(P, g))
            g = g * gk % q
        Aj = ov.add(Aj, ov.mul(opr.z, rr))
        Aj = ov.add(Aj, ov.neg(ov.mul(vk.g1, (c + rr * zw) % q)))
        Aj = ov.add(Aj, ov.mul(opr.batched_h, zeta))
        Aj = ov.add(Aj, ov.mul(opr.zshift_h, rr * zeta % q * vk.generator % q))
        Bj = ov.neg(ov.add(opr.batched_h, ov.mul(opr.zshift_h, rr)))
        A = ov.add(A, ov.mul(Aj, rho[j]))
        B = ov.add(B, ov.mul(Bj, rho[j]))
    pad = lambda x: vbm.pad_pt(m.cv, x)
    return (D, [fb(x) for x in rho[:4]], [pad(x) for x in lins[:4]], pad(oplonk.rb_ec(ov, A)), pad(oplonk.rb_ec(ov, B)))


def _single(vk, raw, pub):
    rv = vk.raw()
    return lib.apk_verify(C.byref(rv), C.byref(raw), vk.curve.fr_vector(pub))


@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("circuit", PLAIN + ["bsb1", "bsb2"])
def test_good_batches_take_one_fold_and_match_the_restatement(cname, circuit):
    """All good: APK_OK, every status APK_OK, one fold; D, rho_j, [lin]_j, A and B equal the Python restatement byte for byte."""
    m = vbm.material(cname, circuit)
    for n in (8, 3):
        raws, pubs, oprs = m.take(n)
        rc, status, tr = vbm.run_batch(m.vk, raws, pubs)
        assert rc == OK, lib.apk_last_error()
        assert status == [OK] * n and tr.folds == 1
        assert vbm.trace_bytes(tr, n) == restate(m, oprs, pubs)


@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("circuit", ["pyth", "bsb1"])
def test_a_proof_whose_sizes_do_not_match_enters_the_digest_as_a_marker(cname, circuit):
    """One proof with a wrong public-witness length: rejected alone, D takes its marker byte 0, the fold of the other five - with
    their own rho_j - is the restated one."""
    m = vbm.material(cname, circuit)
    raws, pubs, oprs = m.take(6)
    nb = [len(p) for p in pubs]
    nb[2] += 1
    rc, status, tr = vbm.run_batch(m.vk, raws, pubs, nb_public=nb)
    assert rc == BAD and status == [BAD if j == 2 else OK for j in range(6)] and tr.folds == 1
    assert vbm.trace_bytes(tr, 6) == restate(m, oprs, pubs, unreadable={2})


@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("circuit", PLAIN + ["bsb1", "bsb2"])
def test_one_mutated_proof_is_found_by_index(cname, circuit):
    """Each mutation on ONE proof of a batch of 8, at every position 0, 3, 7: exactly that status is APK_ERR_VERIFY."""
    m = vbm.material(cname, circuit)
    cv = m.cv
    k = len(m.ovk.qcp)
    for name in _mutations(cv, m.oprs[0], k):
        for pos in (0, 3, 7):
            raws, pubs, oprs = m.take(8)
            _mutations(cv, oprs[pos], k)[name](raws[pos], pubs[pos])
            rc, status, tr = vbm.run_batch(m.vk, raws, pubs)
            assert rc == BAD and status == [BAD if j == pos else OK for j in range(8)], (name, pos, status, lib.apk_last_error())
            assert tr.folds <= 1 + 2 * 3                      # 2 * bad * ceil(log2 8) extra folds at most
            assert ("proof %d rejected" % pos).encode() in lib.apk_last_error()


@pytest.mark.parametrize("cname", CNAMES)
def test_two_bad_all_bad_and_empty(cname):
    m = vbm.material(cname, "pyth")
    cv = m.cv
    raws, pubs, oprs = m.take(8)
    muts = _mutations(cv, oprs[2], 0)
    muts["scalar"](raws[2], pubs[2])
    _mutations(cv, oprs[5], 0)["opening"](raws[5], pubs[5])
    rc, status, tr = vbm.run_batch(m.vk, raws, pubs)
    assert rc == BAD and status == [BAD if j in (2, 5) else OK for j in range(8)]
    assert tr.folds <= 1 + 2 * 2 * 3
    raws, pubs, oprs = m.take(8)
    for j in range(8):
        _mutations(cv, oprs[j], 0)["scalar"](raws[j], pubs[j])
    rc, status, tr = vbm.run_batch(m.vk, raws, pubs)
    assert rc == BAD and status == [BAD] * 8
    rc, status, tr = vbm.run_batch(m.vk, [], [])
    assert rc == OK and tr.folds == 0


@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("circuit", PLAIN + ["bsb1", "bsb2"])
def test_a_batch_of_one_gives_apk_verify_s_verdict(cname, circuit):
    """count = 1 against apk_verify on the same inputs, for every case of tests/test_verify_host.py."""
    m = vbm.material(cname, circuit)
    cv = m.cv
    k = len(m.ovk.qcp)
    cases = [lambda p, pub: None, lambda p, pub: C.memmove(p.claimed_values[0], cv.fr_to_mont_bytes(12345), 32)]
    cases += list(_mutations(cv, m.oprs[0], k).values())
    for edit in cases:
        raws, pubs, _ = m.take(1)
        edit(raws[0], pubs[0])
        want = _single(m.vk, raws[0], pubs[0])
        rc, status, tr = vbm.run_batch(m.vk, raws, pubs)
        assert rc == want and status == [want]
    # a key for another tau rejects everything, one by one and together
    other = vbm.product_vk(cv, m.ovk, ap_setup.g2_from_tau(cv, m.tau + 1))
    raws, pubs, _ = m.take(1)
    assert _single(other, raws[0], pubs[0]) == BAD
    rc, status, _ = vbm.run_batch(other, raws, pubs)
    assert rc == BAD and status == [BAD]
    if k:
        wrong = vbm.product_vk(cv, m.ovk, m.g2)
        wrong.CommitmentConstraintIndexes[0] += 1
        assert _single(wrong, raws[0], pubs[0]) == BAD
        rc, status, _ = vbm.run_batch(wrong, raws, pubs)
        assert rc == BAD and status == [BAD]


@pytest.mark.parametrize("cname", CNAMES)
def test_opposite_openings_do_not_cancel(cname):
    """The attack the weights exist for: opening points of one proof replaced by the negated ones of another, so that they
    would cancel term by term in an unweighted sum of the B_j.  One tampered proof is found alone; a pair tampered against
    each other is rejected as a pair, the rest of the batch accepted."""
    m = vbm.material(cname, "pyth")
    cv, ov = m.cv, m.ov
    raws, pubs, oprs = m.take(4)
    for name in ("batched_h", "zshift_h"):                     # Wz_1 := -Wz_0, Wzw_1 := -Wzw_0
        b = cv.g1_to_bytes(ov.neg(getattr(oprs[0], name)))
        C.memmove(getattr(raws[1], name), b, len(b))
    rc, status, _ = vbm.run_batch(m.vk, raws, pubs)
    assert rc == BAD and status == [OK, BAD, OK, OK]
    raws, pubs, oprs = m.take(4)
    for j, o in ((0, 1), (1, 0)):                              # swap and negate: both tampered
        for name in ("batched_h", "zshift_h"):
            b = cv.g1_to_bytes(ov.neg(getattr(oprs[o], name)))
            C.memmove(getattr(raws[j], name), b, len(b))
    rc, status, _ = vbm.run_batch(m.vk, raws, pubs)
    assert rc == BAD and status == [BAD, BAD, OK, OK]


@pytest.mark.parametrize("cname", CNAMES)
def test_lincomb_segments_on_the_host(cname):
    """apk_g1_lincomb_segments(device = -1) against ov.mul / ov.add: empty segment, P and -P, the same point twice, zero scalars,
    scalar r - 1, an infinity input."""
    cv, ov = CURVES[cname]
    g = SplitMix64(0x11C)
    G = ov.mul(cv.g1, 1)
    P, Q = ov.mul(G, g.fr(cv.r)), ov.mul(G, g.fr(cv.r))
    a, b = g.fr(cv.r), g.fr(cv.r)
    points = [P, ov.neg(P), P, P, Q, Q, P, None, Q, P]
    scalars = [a, a, a, a, 0, 0, cv.r - 1, b, b, 1]
    seg = [0, 0, 2, 4, 6, 7, 9, 10, 10]
    rc, got = vbm.lincomb(cv, -1, points, scalars, seg)
    assert rc == OK, lib.apk_last_error()
    want = vbm.lincomb_reference(ov, points, scalars, seg)
    assert got == want
    assert got[0] is None and got[1] is None and got[3] is None and got[-1] is None and got[4] == ov.neg(P)
    pts = [ov.mul(G, g.fr(cv.r)) for _ in range(23)]
    sc = [g.fr(cv.r) for _ in range(23)]
    seg = [0, 11, 12, 23]
    rc, got = vbm.lincomb(cv, -1, pts, sc, seg)
    assert rc == OK and got == vbm.lincomb_reference(ov, pts, sc, seg)
    assert vbm.lincomb(cv, -1, pts, sc, [0, 5, 3])[0] == _lib.APK_ERR_ARG
    assert vbm.lincomb(cv, -1, pts, sc, [1, 5])[0] == _lib.APK_ERR_ARG


@pytest.mark.parametrize("cname", CNAMES)
def test_wrong_witness_size_other_tau_and_bad_key(cname):
    m = vbm.material(cname, "pyth")
    cv = m.cv
    raws, pubs, _ = m.take(8)
    nb = [len(p) for p in pubs]
    nb[4] -= 1                                                  # as apk_verify_ex: a length that is not vk.nb_public rejects
    rc, status, _ = vbm.run_batch(m.vk, raws, pubs, nb_public=nb)
    assert rc == BAD and status == [BAD if j == 4 else OK for j in range(8)]
    assert b"invalid witness size, got 1, expected 2 (public)" in lib.apk_last_error()
    other = vbm.product_vk(cv, m.ovk, ap_setup.g2_from_tau(cv, tau_from_seed(vbm.TAU_SEED, cv.r) + 1))
    rc, status, _ = vbm.run_batch(other, raws, pubs)
    assert rc == BAD and status == [BAD] * 8
    bad_key = vbm.product_vk(cv, m.ovk, m.g2)
    bad_key.Size = 12                                           # not a power of two
    assert vbm.run_batch(bad_key, raws, pubs)[0] == _lib.APK_ERR_ARG
    bad_key = vbm.product_vk(cv, m.ovk, m.g2)
    bad_key.KzgG1 = (bad_key.KzgG1[0], (bad_key.KzgG1[1] + 1) % cv.p)     # not a curve point
    rv = bad_key.raw()
    assert vbm.run_batch(bad_key, raws, pubs)[0] == _lib.APK_ERR_ARG
    assert lib.apk_verify(C.byref(rv), C.byref(raws[0]), cv.fr_vector(pubs[0])) in (_lib.APK_ERR_ARG,)


def test_python_api_on_the_host():
    """plonk.VerifyBatch on raw proofs, host mode"""
    from algoplonk_amd import plonk as ap_plonk
    m = vbm.material("bn254", "pyth")
    raws, pubs, oprs = m.take(4)
    C.memmove(raws[2].zshift_h, bytes(raws[2].batched_h), 96)
    proofs = [ap_plonk.Proof(m.cv, r) for r in raws]
    assert ap_plonk.VerifyBatch(proofs, m.vk, pubs, device=-1) == [True, True, False, True]

"""CPU tier: apk_verify_batch_keys / apk_verify_blobs with device = -1 (include/apk.h; csrc/verify_keys.h): proofs of several
circuits in one call, one pairing check per SRS, against apk_verify_batch per circuit, the oracle and a plain-Python restatement
of the statement (tests/verify_keys_material.py).  Proofs: oracle proofs of the pythagorean circuit (k = 0, n = 8) and the BSB22
circuits with one (n = 8) and two (n = 16) commitments.  Nothing here needs a GPU."""
import ctypes as C

import pytest

from algoplonk_amd import _lib, ecc, plonk as ap_plonk, ImportProofAndPublicInputs, MarshalProof, VerifyBatchKeys, VerifyBlob
from algoplonk_amd._lib import lib

import verify_batch_material as vbm
import verify_keys_material as vkm

OK, ARG, BAD = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_VERIFY
CNAMES = ["bn254", "bls12-381"]


three, bump_scalar, blobs_of = vkm.three, vkm.bump_scalar, vkm.blobs_of


@pytest.mark.parametrize("cname", CNAMES)
def test_three_circuits_under_one_tau_take_one_fold(cname):
    """Nine proofs of three circuits, interleaved: one group, one fold, the verdicts of three apk_verify_batch calls, and the trace
    is the restated statement byte for byte - [lin]_j of the first four proofs and A, B from the oracle's big-integer sums, which
    pins the per-key accumulation of the scalars of S1, S2 and Qcp_i."""
    mats = three(cname)
    assert [(len(m.ovk.qcp), m.ovk.size) for m in mats] == [(0, 8), (1, 8), (2, 16)]
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    rc, status, tr = vkm.run_keys([m.vk for m in mats], key_of, raws, pubs)
    assert rc == OK, lib.apk_last_error()
    assert status == [OK] * 9 and tr.groups == 1 and tr.folds == 1
    for i, m in enumerate(mats):
        sel = [j for j in range(9) if key_of[j] == i]
        rc1, st1, _ = vbm.run_batch(m.vk, [raws[j] for j in sel], [pubs[j] for j in sel])
        assert rc1 == OK and st1 == [status[j] for j in sel]
    assert vkm.trace_bytes(tr) == vkm.restate(mats, key_of, oprs, pubs) + (1,)


@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("pos", range(9))
def test_one_mutated_proof_is_found_at_every_position(cname, pos):
    mats = three(cname)
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    bump_scalar(mats[key_of[pos]], raws[pos], oprs[pos])
    rc, status, tr = vkm.run_keys([m.vk for m in mats], key_of, raws, pubs)
    assert rc == BAD and status == [BAD if j == pos else OK for j in range(9)], (pos, status, lib.apk_last_error())
    assert tr.groups == 1 and tr.folds <= 1 + 2 * 1 * 4                        # 1 + 2 * bad * ceil(log2 9)
    assert ("proof %d rejected" % pos).encode() in lib.apk_last_error()


@pytest.mark.parametrize("cname", CNAMES)
def test_two_bad_proofs_under_two_keys_and_sizes_that_do_not_match(cname):
    mats = three(cname)
    vks = [m.vk for m in mats]
    # two bad proofs under two different keys, the second one failing its OWN checks (a point off the curve)
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    assert key_of[1] != key_of[6]
    bump_scalar(mats[key_of[1]], raws[1], oprs[1])
    C.memmove(raws[6].zshift_h, bytes(raws[6].batched_h), 96)
    rc, status, tr = vkm.run_keys(vks, key_of, raws, pubs)
    assert rc == BAD and status == [BAD if j in (1, 6) else OK for j in range(9)]
    assert tr.folds <= 1 + 2 * 2 * 4
    # a proof whose sizes do not match its key enters the digest as a marker and is rejected alone
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    key_of[4] = 2                                                             # a k = 1 proof handed the k = 2 key
    nb = [len(p) for p in pubs]
    nb[8] += 1
    rc, status, tr = vkm.run_keys(vks, key_of, raws, pubs, nb_public=nb)
    assert rc == BAD and status == [BAD if j in (4, 8) else OK for j in range(9)] and tr.folds == 1
    assert vkm.trace_bytes(tr) == vkm.restate(mats, key_of, oprs, pubs, unreadable={4, 8}) + (1,)


@pytest.mark.parametrize("cname", CNAMES)
def test_a_second_tau_is_a_second_group(cname):
    a, b, other = vbm.material(cname, "pyth"), vbm.material(cname, "bsb1"), vkm.other_tau(cname)
    mats = [a, other, b]
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    rc, status, tr = vkm.run_keys([m.vk for m in mats], key_of, raws, pubs)
    assert rc == OK and status == [OK] * 9 and tr.groups == 2 and tr.folds == 2, lib.apk_last_error()
    assert vkm.trace_bytes(tr) == vkm.restate(mats, key_of, oprs, pubs) + (2,)
    # a proof handed the other group's key (the same circuit, so every size matches): rejected alone
    key_of[3] = 1
    rc, status, tr = vkm.run_keys([m.vk for m in mats], key_of, raws, pubs)
    assert rc == BAD and status == [BAD if j == 3 else OK for j in range(9)] and tr.groups == 2


def test_both_curves_in_one_call_are_two_groups():
    mats = [vbm.material("bn254", "pyth"), vbm.material("bls12-381", "bsb1"), vbm.material("bn254", "bsb2")]
    key_of, raws, pubs, oprs = vkm.interleave(mats, 2)
    vks = [m.vk for m in mats]
    rc, status, tr = vkm.run_keys(vks, key_of, raws, pubs)
    assert rc == OK and status == [OK] * 6 and tr.groups == 2 and tr.folds == 2, lib.apk_last_error()
    assert vkm.trace_bytes(tr) == vkm.restate(mats, key_of, oprs, pubs) + (2,)
    bump_scalar(mats[1], raws[4], oprs[4])
    rc, status, tr = vkm.run_keys(vks, key_of, raws, pubs)
    assert rc == BAD and status == [OK, OK, OK, OK, BAD, OK] and tr.folds == 2 + 1       # (the left half verifies: the right one is not folded again)
    key_of[0] = 1                                                             # a BN254 proof under the BLS12-381 key
    rc, status, tr = vkm.run_keys(vks, key_of, raws, pubs)
    assert rc == BAD and status == [BAD, OK, OK, OK, BAD, OK]


@pytest.mark.parametrize("cname", CNAMES)
def test_opposite_openings_under_two_keys_do_not_cancel(cname):
    """The cross-key form of test_verify_batch.py::test_opposite_openings_do_not_cancel: W_zeta of proof a (key A) moved by +P,
    W_zeta of proof b (key B) by -P - in an unweighted sum of the B_j the two would cancel.  Both are rejected, nothing else is."""
    mats = three(cname)
    ov, cv = mats[0].ov, mats[0].cv
    key_of, raws, pubs, oprs = vkm.interleave(mats, 2)
    P = ov.mul(cv.g1, 0xC0FFEE)
    assert key_of[0] != key_of[1]
    for j, Q in ((0, P), (1, ov.neg(P))):
        moved = cv.g1_to_bytes(ov.add(oprs[j].batched_h, Q))
        C.memmove(raws[j].batched_h, moved, len(moved))
    rc, status, _ = vkm.run_keys([m.vk for m in mats], key_of, raws, pubs)
    assert rc == BAD and status == [BAD, BAD, OK, OK, OK, OK]


@pytest.mark.parametrize("cname", CNAMES)
def test_one_key_gives_apk_verify_batch_s_statuses(cname):
    for circuit in ("pyth", "bsb2"):
        m = vbm.material(cname, circuit)
        raws, pubs, oprs = m.take(6)
        bump_scalar(m, raws[1], oprs[1])
        raws[4].z[0] ^= 1                                                     # off the curve
        nb = [len(p) for p in pubs]
        nb[5] += 1
        want = vbm.run_batch(m.vk, raws, pubs, nb_public=nb)
        rc, status, tr = vkm.run_keys([m.vk], [0] * 6, raws, pubs, nb_public=nb)
        assert (rc, status) == (want[0], want[1]) and status == [OK, BAD, OK, OK, BAD, BAD] and tr.groups == 1
        raws, pubs, _ = m.take(5)
        assert vkm.run_keys([m.vk], [0] * 5, raws, pubs)[:2] == vbm.run_batch(m.vk, raws, pubs)[:2] == (OK, [OK] * 5)


@pytest.mark.parametrize("cname", CNAMES)
def test_empty_calls_and_argument_errors(cname):
    mats = three(cname)
    vks = [m.vk for m in mats]
    cv = mats[0].cv
    rc, status, tr = vkm.run_keys(vks, [], [], [])
    assert rc == OK and tr.groups == 1 and tr.folds == 0                       # count = 0: the keys are checked
    assert lib.apk_verify_batch_keys(-1, None, 0, None, None, None, None, 0, None, None) == OK
    bad_g1 = vbm.product_vk(cv, mats[0].ovk, mats[0].g2)
    bad_g1.KzgG1 = (bad_g1.KzgG1[0], (bad_g1.KzgG1[1] + 1) % cv.p)              # not a curve point
    assert vkm.run_keys(vks + [bad_g1], [], [], [])[0] == ARG
    key_of, raws, pubs, _ = vkm.interleave(mats, 1)
    assert vkm.run_keys(vks + [bad_g1], key_of, raws, pubs)[0] == OK           # ... as apk_verify reports it: where a proof uses the key
    assert vkm.run_keys(vks + [bad_g1], [0, 1, 3], raws, pubs)[0] == BAD       # (sizes of proof 2 do not match key 3: the key is not looked at)
    assert vkm.run_keys(vks + [bad_g1], [3, 1, 2], raws, pubs)[0] == ARG
    bad_n = vbm.product_vk(cv, mats[0].ovk, mats[0].g2)
    bad_n.Size = 12                                                            # not a power of two
    assert vkm.run_keys(vks + [bad_n], key_of, raws, pubs)[0] == ARG
    keys = vkm.key_array(vks)
    keys[1].curve = 4
    assert vkm.run_keys(vks, key_of, raws, pubs, keys=keys)[0] == ARG and b"unsupported curve" in lib.apk_last_error()
    assert vkm.run_keys(vks, [0, 1, 3], raws, pubs)[0] == ARG and b"key_of" in lib.apk_last_error()
    assert vkm.run_keys([], key_of, raws, pubs)[0] == ARG                      # nb_keys = 0 with count > 0
    # null pointers
    arr = (_lib.Proof * 3)(*raws)
    kof, nbs, st = (C.c_uint32 * 3)(*key_of), (C.c_uint32 * 3)(*[len(p) for p in pubs]), (C.c_int * 3)()
    bufs = [cv.fr_vector(p) for p in pubs]
    ptrs = (C.c_void_p * 3)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bufs])
    keys = vkm.key_array(vks)
    assert lib.apk_verify_batch_keys(-1, keys, 3, kof, arr, ptrs, nbs, 3, st, None) == OK
    assert lib.apk_verify_batch_keys(-1, None, 3, kof, arr, ptrs, nbs, 3, st, None) == ARG
    assert lib.apk_verify_batch_keys(-1, keys, 3, None, arr, ptrs, nbs, 3, st, None) == ARG
    assert lib.apk_verify_batch_keys(-1, keys, 3, kof, None, ptrs, nbs, 3, st, None) == ARG
    assert lib.apk_verify_batch_keys(-1, keys, 3, kof, arr, None, nbs, 3, st, None) == ARG
    assert lib.apk_verify_batch_keys(-1, keys, 3, kof, arr, ptrs, None, 3, st, None) == ARG
    assert lib.apk_verify_batch_keys(-1, keys, 3, kof, arr, ptrs, nbs, 3, None, None) == ARG
    assert lib.apk_verify_batch_keys(-2, keys, 3, kof, arr, ptrs, nbs, 3, st, None) == ARG


@pytest.mark.parametrize("cname", CNAMES)
def test_blobs_are_unmarshal_then_batch_keys(cname):
    mats = three(cname)
    vks = [m.vk for m in mats]
    cv = mats[0].cv
    key_of, raws, pubs, oprs = vkm.interleave(mats, 2)
    blobs, pibs = blobs_of(mats, key_of, oprs, pubs)
    assert [ap_plonk.UnmarshalPublicInputs(cv, b) for b in pibs] == pubs
    unmarshalled = [ap_plonk.UnmarshalProof(cv, b).raw for b in blobs]
    assert [vbm.run_batch(mats[key_of[j]].vk, [unmarshalled[j]], [pubs[j]])[0] for j in range(6)] == [OK] * 6
    want = vkm.run_keys(vks, key_of, unmarshalled, pubs)
    rc, status, tr = vkm.run_blobs(vks, key_of, blobs, pibs)
    assert (rc, status) == (OK, [OK] * 6) == want[:2] and vkm.trace_bytes(tr) == vkm.trace_bytes(want[2])
    # a truncated blob in the middle, a scalar equal to r, public inputs one byte short: each rejected alone, by index
    off = 6 * 2 * cv.fp_bytes
    broken = list(blobs)
    broken[2] = broken[2][:-32]
    broken[3] = broken[3][:off] + cv.r.to_bytes(32, "big") + broken[3][off + 32:]
    short = list(pibs)
    short[5] = short[5][:-1]
    rc, status, tr = vkm.run_blobs(vks, key_of, broken, short)
    assert rc == BAD and status == [OK, OK, BAD, BAD, OK, BAD] and tr.folds == 1
    assert b"proof 2 rejected: proof blob: %d bytes" % len(broken[2]) in lib.apk_last_error()
    assert vkm.trace_bytes(tr) == vkm.restate(mats, key_of, oprs, pubs, unreadable={2, 3, 5}) + (1,)
    # argument errors of the call stay argument errors
    assert vkm.run_blobs(vks, [0, 1, 2, 0, 1, 3], blobs, pibs)[0] == ARG
    assert vkm.run_blobs([], key_of, blobs, pibs)[0] == ARG
    assert lib.apk_verify_blobs(-1, vkm.key_array(vks), 3, None, None, None, None, None, 6, None, None) == ARG


def test_python_api_on_files(tmp_path):
    """VerifyBatchKeys on bytes, on Proof objects and on a mix; VerifyBlob and ImportProofAndPublicInputs on exported files"""
    mats = three("bn254")
    cv = ecc.BN254
    key_of, raws, pubs, oprs = vkm.interleave(mats, 2)
    blobs, pibs = blobs_of(mats, key_of, oprs, pubs)
    paths = []
    for j in range(6):
        paths.append((str(tmp_path / ("proof%d.bin" % j)), str(tmp_path / ("public%d.bin" % j))))
        open(paths[j][0], "wb").write(blobs[j]); open(paths[j][1], "wb").write(pibs[j])
    read = [ImportProofAndPublicInputs(cv, *p) for p in paths]
    assert [MarshalProof(p) for p, _ in read] == blobs and [pub for _, pub in read] == pubs
    vk = lambda j: mats[key_of[j]].vk
    assert VerifyBatchKeys([(vk(j), blobs[j], pibs[j]) for j in range(6)], device=-1) == [True] * 6
    assert VerifyBatchKeys([(vk(j), read[j][0], read[j][1]) for j in range(6)], device=-1) == [True] * 6
    mixed = [(vk(j), blobs[j] if j % 2 else read[j][0], pibs[j] if j < 3 else pubs[j]) for j in range(6)]
    mixed[1] = (vk(1), blobs[1][:-1], pibs[1])
    mixed[4] = (vk(4), read[5][0], pubs[4])
    assert VerifyBatchKeys(mixed, device=-1) == [True, False, True, True, False, True]
    flipped = bytearray(blobs[3]); flipped[-1] ^= 1
    assert VerifyBatchKeys([(vk(j), bytes(flipped) if j == 3 else blobs[j], pibs[j]) for j in range(6)], device=-1) == [j != 3 for j in range(6)]
    assert VerifyBatchKeys([], device=-1) == []
    VerifyBlob(vk(0), blobs[0], pibs[0])
    with pytest.raises(ap_plonk.VerificationError, match="pairing check"):
        VerifyBlob(vk(0), blobs[0], pibs[3])
    with pytest.raises(ap_plonk.VerificationError, match="proof blob: 767 bytes"):
        VerifyBlob(vk(0), blobs[0][:-1], pibs[0])
    with pytest.raises(ap_plonk.VerificationError, match="proof blob"):
        open(paths[0][0], "wb").write(blobs[0][:-5])
        ImportProofAndPublicInputs(cv, *paths[0])

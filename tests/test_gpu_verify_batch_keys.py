"""-m gpu: apk_verify_batch_keys / apk_verify_blobs on the device (the sums and the point check through kernels_lincomb.h) against
host mode - status arrays and every byte of the trace - on the cases of tests/test_verify_batch_keys.py; then on proofs the HIP
prover makes in three contexts on one GPU, exported to files and read back; and on a BLS12-381 point outside the prime-order
subgroup that arrives in a blob."""
import ctypes as C

import pytest

from algoplonk_amd import _lib, plonk as ap_plonk, setup as ap_setup, ImportProofAndPublicInputs, MarshalProof, VerifiedProof
from algoplonk_amd._lib import lib
from oracle import plonk as oplonk
from oracle.prng import SplitMix64, tau_from_seed

from helpers import CURVES
from test_template_pin import _ccs_from_oracle_circuit
import verify_batch_material as vbm
import verify_keys_material as vkm
from verify_keys_material import blobs_of, bump_scalar, three

pytestmark = pytest.mark.gpu
OK, BAD = _lib.APK_OK, _lib.APK_ERR_VERIFY
CNAMES = ["bn254", "bls12-381"]


def both_modes(gpu, vks, key_of, raws, pubs):
    """the call on the device and on the host: the same return code, statuses and trace bytes; -> (rc, statuses, trace)"""
    rc_d, st_d, tr_d = vkm.run_keys(vks, key_of, raws, pubs, device=gpu)
    assert rc_d in (OK, BAD), lib.apk_last_error()
    err_d = lib.apk_last_error()
    rc_h, st_h, tr_h = vkm.run_keys(vks, key_of, raws, pubs, device=-1)
    assert (rc_d, st_d) == (rc_h, st_h), (st_d, st_h, err_d, lib.apk_last_error())
    assert vkm.trace_bytes(tr_d) == vkm.trace_bytes(tr_h) and bytes(tr_d) == bytes(tr_h)
    return rc_d, st_d, tr_d


@pytest.mark.parametrize("cname", CNAMES)
def test_three_circuits_under_one_tau_on_the_device(gpu, cname):
    mats = three(cname)
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    rc, status, tr = both_modes(gpu, [m.vk for m in mats], key_of, raws, pubs)
    assert rc == OK and status == [OK] * 9 and tr.groups == 1 and tr.folds == 1
    assert vkm.trace_bytes(tr) == vkm.restate(mats, key_of, oprs, pubs) + (1,)


@pytest.mark.parametrize("cname", CNAMES)
@pytest.mark.parametrize("pos", range(9))
def test_one_mutated_proof_at_every_position_on_the_device(gpu, cname, pos):
    mats = three(cname)
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    bump_scalar(mats[key_of[pos]], raws[pos], oprs[pos])
    rc, status, tr = both_modes(gpu, [m.vk for m in mats], key_of, raws, pubs)
    assert rc == BAD and status == [BAD if j == pos else OK for j in range(9)] and tr.folds <= 1 + 2 * 1 * 4


@pytest.mark.parametrize("cname", CNAMES)
def test_two_bad_proofs_under_two_keys_on_the_device(gpu, cname):
    mats = three(cname)
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    bump_scalar(mats[key_of[1]], raws[1], oprs[1])
    C.memmove(raws[6].zshift_h, bytes(raws[6].batched_h), 96)
    rc, status, tr = both_modes(gpu, [m.vk for m in mats], key_of, raws, pubs)
    assert rc == BAD and status == [BAD if j in (1, 6) else OK for j in range(9)] and tr.folds <= 1 + 2 * 2 * 4


@pytest.mark.parametrize("cname", CNAMES)
def test_a_second_tau_on_the_device(gpu, cname):
    mats = [vbm.material(cname, "pyth"), vkm.other_tau(cname), vbm.material(cname, "bsb1")]
    vks = [m.vk for m in mats]
    key_of, raws, pubs, oprs = vkm.interleave(mats, 3)
    rc, status, tr = both_modes(gpu, vks, key_of, raws, pubs)
    assert rc == OK and status == [OK] * 9 and tr.groups == 2 and tr.folds == 2
    key_of[3] = 1                                              # a proof handed the other group's key
    rc, status, tr = both_modes(gpu, vks, key_of, raws, pubs)
    assert rc == BAD and status == [BAD if j == 3 else OK for j in range(9)]


def test_both_curves_in_one_call_on_the_device(gpu):
    mats = [vbm.material("bn254", "pyth"), vbm.material("bls12-381", "bsb1"), vbm.material("bn254", "bsb2")]
    key_of, raws, pubs, oprs = vkm.interleave(mats, 2)
    rc, status, tr = both_modes(gpu, [m.vk for m in mats], key_of, raws, pubs)
    assert rc == OK and status == [OK] * 6 and tr.groups == 2 and tr.folds == 2
    assert vkm.trace_bytes(tr) == vkm.restate(mats, key_of, oprs, pubs) + (2,)


@pytest.mark.parametrize("cname", CNAMES)
def test_opposite_openings_under_two_keys_on_the_device(gpu, cname):
    mats = three(cname)
    ov, cv = mats[0].ov, mats[0].cv
    key_of, raws, pubs, oprs = vkm.interleave(mats, 2)
    P = ov.mul(cv.g1, 0xC0FFEE)
    for j, Q in ((0, P), (1, ov.neg(P))):
        moved = cv.g1_to_bytes(ov.add(oprs[j].batched_h, Q))
        C.memmove(raws[j].batched_h, moved, len(moved))
    rc, status, _ = both_modes(gpu, [m.vk for m in mats], key_of, raws, pubs)
    assert rc == BAD and status == [BAD, BAD, OK, OK, OK, OK]


def test_exported_proofs_of_three_contexts_verify_in_one_call(gpu, tmp_path):
    """Pythagorean and the one-commitment circuit at n = 8 under one BN254 SRS, the pythagorean circuit on BLS12-381 as a second
    group: three contexts on one GPU, four apk_prove proofs each (fresh blinding every time), written with
    ExportProofAndPublicInputs, read back, verified by ONE apk_verify_blobs call on the device.  One flipped byte in one file is
    found by index."""
    rigs = []
    for cname, circuit in (("bn254", "pythagorean"), ("bn254", "bsb22_square_k1"), ("bls12-381", "pythagorean")):
        cv, _ = CURVES[cname]
        ccs, w = _ccs_from_oracle_circuit(cv, circuit)
        k = len(ccs.commitments)
        tau = tau_from_seed(0x7E59, cv.r)
        assert ccs.domain_size() == 8
        srs = ap_setup.unsafe_srs(cv, 8, tau, device=gpu, lagrange=k > 0)
        pk, vk = ap_plonk.Setup(ccs, srs, device=gpu)
        vk.KzgG2 = ap_setup.g2_from_tau(cv, tau)
        rigs.append((cv, ccs, w, pk, vk))
    vks, key_of, paths = [r[4] for r in rigs], [], []
    for j in range(4):
        for i, (cv, ccs, w, pk, vk) in enumerate(rigs):
            proof = ap_plonk.Prove(ccs, pk, w)
            paths.append((str(tmp_path / ("proof_%d_%d.bin" % (i, j))), str(tmp_path / ("public_%d_%d.bin" % (i, j)))))
            VerifiedProof(proof, w).ExportProofAndPublicInputs(*paths[-1])
            read, pub = ImportProofAndPublicInputs(cv, *paths[-1])
            assert MarshalProof(read) == MarshalProof(proof) and pub == list(w.Public().public)
            key_of.append(i)
    blobs = [open(p, "rb").read() for p, _ in paths]
    pibs = [open(p, "rb").read() for _, p in paths]
    assert len(set(blobs)) == 12
    rc, status, tr = vkm.run_blobs(vks, key_of, blobs, pibs, device=gpu)
    assert rc == OK and status == [OK] * 12 and tr.groups == 2 and tr.folds == 2, lib.apk_last_error()
    rc_h, st_h, tr_h = vkm.run_blobs(vks, key_of, blobs, pibs, device=-1)
    assert (rc_h, st_h) == (rc, status) and bytes(tr_h) == bytes(tr)
    assert ap_plonk.VerifyBatchKeys([(vks[key_of[j]], blobs[j], pibs[j]) for j in range(12)], device=gpu) == [True] * 12
    # one flipped byte in one file (the last byte of r(zeta): the value stays below r)
    cv = rigs[key_of[7]][0]
    damaged = bytearray(blobs[7])
    damaged[6 * 2 * cv.fp_bytes + 2 * 32 - 1] ^= 0x01
    open(paths[7][0], "wb").write(bytes(damaged))
    blobs[7] = open(paths[7][0], "rb").read()
    rc, status, tr = vkm.run_blobs(vks, key_of, blobs, pibs, device=gpu)
    assert rc == BAD and status == [BAD if j == 7 else OK for j in range(12)] and b"proof 7 rejected" in lib.apk_last_error()
    for r in rigs:
        r[3].close()


def test_a_point_outside_the_subgroup_in_a_blob_is_rejected_on_the_device(gpu):
    """BLS12-381: Z replaced by a point of the curve that is not in the order-r subgroup (any on-curve point from a random x: the
    cofactor is ~2^126).  The reader takes it - it checks ranges only - and the device-side check rejects it, alone."""
    mats = three("bls12-381")
    cv, ov = mats[0].cv, mats[0].ov
    g = SplitMix64(0x50B)
    while True:
        x = g.fr(cv.r)
        rhs = (x * x * x + 4) % cv.p
        y = pow(rhs, (cv.p + 1) // 4, cv.p)
        if y * y % cv.p == rhs and ov.mul((x, y), cv.r - 1) != ov.neg((x, y)):
            break
    key_of, raws, pubs, oprs = vkm.interleave(mats, 2)
    blobs, pibs = blobs_of(mats, key_of, oprs, pubs)
    z_off = 6 * 96 + 5 * 32
    assert blobs[4][z_off: z_off + 96] == oplonk.marshal_proof(ov, oprs[4])[z_off: z_off + 96] == ov.raw_bytes(oprs[4].z)
    blobs[4] = blobs[4][:z_off] + x.to_bytes(48, "big") + y.to_bytes(48, "big") + blobs[4][z_off + 96:]
    assert ap_plonk.UnmarshalProof(cv, blobs[4]).Z == (x, y)
    rc, status, _ = vkm.run_blobs([m.vk for m in mats], key_of, blobs, pibs, device=gpu)
    assert rc == BAD and status == [BAD if j == 4 else OK for j in range(6)]
    assert b"proof 4 rejected" in lib.apk_last_error() and b"prime-order subgroup (device check)" in lib.apk_last_error()
    assert vkm.run_blobs([m.vk for m in mats], key_of, blobs, pibs, device=-1)[1] == status

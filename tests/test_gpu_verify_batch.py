"""-m gpu: apk_verify_batch / apk_g1_lincomb_segments on the device (kernels_lincomb.h) against host mode - statuses and trace
bytes - on the material of tests/test_verify_batch.py, then on proofs the HIP prover makes while other callers keep proving on
the same GPU, through CompiledCircuit.VerifyMany, and on a BLS12-381 point outside the prime-order subgroup."""
import ctypes as C
import threading

import pytest

from algoplonk_amd import _lib, batch, frontend, plonk as ap_plonk, setup as ap_setup, workloads
from algoplonk_amd import Compile
from algoplonk_amd._lib import lib, check
from bench_cpu import oracle_blobs
from oracle.prng import SplitMix64

from helpers import CURVES, oracle_threads
import verify_batch_material as vbm

pytestmark = pytest.mark.gpu
OK, BAD = _lib.APK_OK, _lib.APK_ERR_VERIFY


def _marshal(pr) -> bytes:
    out = C.create_string_buffer(2048)
    ln = C.c_size_t(0)
    check(lib.apk_marshal_proof(C.byref(pr), out, 2048, C.byref(ln)))
    return out.raw[: ln.value]


@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
@pytest.mark.parametrize("circuit", ["pyth", "rnd", "bsb1", "bsb2"])
def test_device_mode_equals_host_mode(gpu, cname, circuit):
    """N in {1, 2, 7, 64, 257}, k in {0, 1, 2}: statuses and trace bytes (D, rho, [lin]_j, A, B, folds) equal host mode's; at
    N = 7 also with one mutated proof.  (The random chain, a second k = 0 circuit, stops at N = 7: host mode is the slow side.)"""
    m = vbm.material(cname, circuit)
    full = circuit != "rnd"
    sizes = (1, 2, 7, 64, 257) if full else (1, 2, 7)
    for n in sizes:
        raws, pubs, _ = m.take(n)
        rc_d, st_d, tr_d = vbm.run_batch(m.vk, raws, pubs, device=gpu)
        assert rc_d == OK and st_d == [OK] * n and tr_d.folds == 1, (n, lib.apk_last_error())
        rc_h, st_h, tr_h = vbm.run_batch(m.vk, raws, pubs, device=-1)
        assert (rc_h, st_h) == (rc_d, st_d)
        assert vbm.trace_bytes(tr_d, n) == vbm.trace_bytes(tr_h, n), n
    raws, pubs, _ = m.take(7)
    C.memmove(raws[4].zshift_h, bytes(raws[4].batched_h), 96)
    rc_d, st_d, tr_d = vbm.run_batch(m.vk, raws, pubs, device=gpu)
    rc_h, st_h, tr_h = vbm.run_batch(m.vk, raws, pubs, device=-1)
    assert rc_d == rc_h == BAD and st_d == st_h == [BAD if j == 4 else OK for j in range(7)]
    assert vbm.trace_bytes(tr_d, 7) == vbm.trace_bytes(tr_h, 7) and tr_d.folds == tr_h.folds


@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_lincomb_segments_on_the_device(gpu, cname):
    """random and degenerate inputs, segment shapes {1 x 1, 300 x 11, 1 x 5000, mixed lengths including empty}"""
    cv, ov = CURVES[cname]
    g = SplitMix64(0x5E6)
    G = ov.mul(cv.g1, 1)
    base = [ov.mul(G, g.fr(cv.r)) for _ in range(40)]

    def both(points, scalars, seg):
        rc_h, host = vbm.lincomb(cv, -1, points, scalars, seg)
        rc_d, dev = vbm.lincomb(cv, gpu, points, scalars, seg)
        assert rc_h == OK and rc_d == OK, lib.apk_last_error()
        assert dev == host
        return dev

    P, Q = base[0], base[1]
    a, b = g.fr(cv.r), g.fr(cv.r)
    points = [P, ov.neg(P), P, P, Q, Q, P, None, Q, P]
    scalars = [a, a, a, a, 0, 0, cv.r - 1, b, b, 1]
    got = both(points, scalars, [0, 0, 2, 4, 6, 7, 9, 10, 10])
    assert got == vbm.lincomb_reference(ov, points, scalars, [0, 0, 2, 4, 6, 7, 9, 10, 10])
    both([P], [a], [0, 1])
    n = 300 * 11
    both([base[g.below(40)] for _ in range(n)], [g.fr(cv.r) for _ in range(n)], [11 * i for i in range(301)])
    both([base[g.below(40)] for _ in range(5000)], [g.fr(cv.r) for _ in range(5000)], [0, 5000])
    seg = [0, 0, 1, 1, 70, 71, 200, 200, 333]
    both([base[g.below(40)] for _ in range(333)], [g.fr(cv.r) for _ in range(333)], seg)
    both([P] * 130 + [ov.neg(P)] * 130, [a] * 260, [0, 260])          # equal and opposite operands all through the tree


@pytest.mark.parametrize("cname,log_n", [("bn254", 13), ("bls12-381", 12)])
def test_proofs_of_the_hip_prover_verified_beside_running_provers(gpu, cname, log_n):
    """32 distinct witnesses of a circuit with one BSB22 commitment, proved by apk_prove_device, verified in one device batch
    while 8 callers keep proving on the same GPU: all accepted, one corrupted proof found by index, and the provers' blobs are
    still the oracle's."""
    cv, ov = CURVES[cname]
    seed = 0xA193
    ccs, w, bl, tau = workloads.random_circuit_bsb22(cv, log_n, seed, nb_commitments=1)
    n = ccs.domain_size()
    srs = ap_setup.unsafe_srs(cv, n, tau, device=gpu, lagrange=True)
    T, K = 8, 32
    pk, vk = ap_plonk.Setup(ccs, srs, device=gpu, slots=T)
    vs = [workloads.Variant(w, bl, None, [(0xA193, 0x3910A)])] + workloads.variant_inputs(ccs, K - 1, seed)
    ws = batch.WitnessSet(pk, ccs, vs).to_device()
    want = oracle_blobs(cv, ccs, srs, ws.items, threads=oracle_threads())
    assert len(set(want)) == K
    proofs = []
    for a in range(K):
        pr = _lib.Proof()
        check(ws.prove(a, pr, "device"))
        assert _marshal(pr) == want[a]
        proofs.append(pr)
    stop, errors, made = threading.Event(), [], []

    def prover(i):
        pr = _lib.Proof()
        r = 0
        while not stop.is_set() or r < 2:
            a = (i + 5 * r) % K
            rc = ws.prove(a, pr, "device")
            if rc != 0:
                errors.append((rc, lib.apk_last_error()))
                return
            made.append((a, _marshal(pr)))
            r += 1

    th = [threading.Thread(target=prover, args=(i,)) for i in range(T)]
    [t.start() for t in th]
    try:
        assert ws.verify_all(proofs, vk, gpu) == [True] * K
        bad = [vbm.clone(p) for p in proofs]
        bad[17].zshift_value[3] ^= 0x10
        assert ws.verify_all(bad, vk, gpu) == [j != 17 for j in range(K)]
        assert ws.verify_all(proofs, vk, -1) == [True] * K
    finally:
        stop.set()
        [t.join() for t in th]
    assert not errors, errors[0]
    assert len(made) >= 2 * T and all(blob == want[a] for a, blob in made)
    ws.close()
    pk.close()


def test_verify_many_names_the_wrong_assignment(gpu, monkeypatch):
    class Pyth(frontend.Circuit):
        A = frontend.Public(); B = frontend.Public(); C = frontend.Secret()

        def define(self, api):
            api.AssertIsEqual(api.Add(api.Mul(self.A, self.A), api.Mul(self.B, self.B)), api.Mul(self.C, self.C))

    cv, _ = CURVES["bn254"]
    cc = Compile(Pyth(), cv, ap_setup.Name.TestOnlyBN254, device=gpu, seed=0x9A7)
    good = []
    for t in ((3, 4, 5), (5, 12, 13), (8, 15, 17)):
        a = Pyth(); a.A, a.B, a.C = t
        good.append(a)
    for dev in (gpu, -1):
        out = cc.VerifyMany(good, device=dev)
        assert len(out) == 3 and [vp.Witness.public for vp in out] == [[3, 4], [5, 12], [8, 15]]
    wrong = Pyth(); wrong.A, wrong.B, wrong.C = 5, 12, 14
    with pytest.raises(RuntimeError, match=r"error creating Plonk proof: .*\(assignment 1\)"):
        cc.VerifyMany([good[0], wrong, good[2]], device=gpu)
    # a proof that is well-formed but not of its public inputs is the verifier's to find: by index
    proofs = [vp.Proof for vp in out]
    pubs = [[3, 4], [5, 13], [8, 15]]
    assert ap_plonk.VerifyBatch(proofs, cc.Vk, pubs, device=gpu) == [True, False, True]
    # ... and VerifyMany's own rejection: a prover that hands back a damaged proof for the third assignment
    real_prove, calls = ap_plonk.Prove, []

    def damaged(ccs, pk, witness, blinding=None, hiding=None):
        pr = real_prove(ccs, pk, witness, blinding, hiding)
        calls.append(1)
        if len(calls) % 3 == 0:
            pr.raw.zshift_value[5] ^= 1
        return pr

    monkeypatch.setattr(ap_plonk, "Prove", damaged)
    for dev in (gpu, -1):
        with pytest.raises(RuntimeError, match=r"error verifying Plonk proof: rejected by the batch verifier \(assignment 2\)"):
            cc.VerifyMany(good, device=dev)
    monkeypatch.undo()
    cc.Pk.close()


def test_a_point_outside_the_subgroup_is_rejected_on_the_device(gpu):
    """BLS12-381: Z replaced by a point of the curve that is not in the order-r subgroup (any on-curve point from a random x: the
    cofactor is ~2^126) - rejected by the device-side check, the rest of the batch accepted."""
    m = vbm.material("bls12-381", "pyth")
    cv, ov = m.cv, m.ov
    g = SplitMix64(0x50B)
    while True:
        x = g.fr(cv.r)
        rhs = (x * x * x + 4) % cv.p
        y = pow(rhs, (cv.p + 1) // 4, cv.p)
        if y * y % cv.p == rhs and ov.mul((x, y), cv.r - 1) != ov.neg((x, y)):
            break
    raws, pubs, _ = m.take(8)
    b = cv.g1_to_bytes((x, y))
    C.memmove(raws[5].z, b, len(b))
    rc, status, _ = vbm.run_batch(m.vk, raws, pubs, device=gpu)
    assert rc == BAD and status == [BAD if j == 5 else OK for j in range(8)]
    assert b"proof 5 rejected" in lib.apk_last_error() and b"prime-order subgroup (device check)" in lib.apk_last_error()
    assert vbm.run_batch(m.vk, raws, pubs, device=-1)[1] == status

"""Helpers of the cross-circuit batch-verifier tests (test_verify_batch_keys.py, test_gpu_verify_batch_keys.py): the calls
apk_verify_batch_keys / apk_verify_blobs on product keys, proofs under a second tau, and a plain-Python restatement of the
statement include/apk.h gives for them.  The proofs themselves come from verify_batch_material.py.
"""
import ctypes as C
import functools
import hashlib

from algoplonk_amd import _lib, ecc, setup as ap_setup
from algoplonk_amd._lib import lib
from oracle import circuits as ocircuits, plonk as oplonk
from oracle.prng import SplitMix64, tau_from_seed

from helpers import CURVES
import verify_batch_material as vbm

TAU2_SEED = 0x7E58


CIRCUITS = ["pyth", "bsb1", "bsb2"]          # k = 0 (n = 8), k = 1 (n = 8), k = 2 (n = 16)


def three(cname):
    """the three circuits of the cross-circuit tests, eight proofs each, under one tau"""
    return [vbm.material(cname, c) for c in CIRCUITS]


def bump_scalar(m, raw, opr):
    """r(zeta) + 1: every own check of the proof passes, its pairing equation does not hold"""
    C.memmove(raw.claimed_values[2], m.cv.fr_to_mont_bytes((opr.claimed_values[2] + 1) % m.cv.r), 32)


def blobs_of(mats, key_of, oprs, pubs):
    return ([oplonk.marshal_proof(mats[key_of[j]].ov, oprs[j]) for j in range(len(oprs))], [oplonk.marshal_public_inputs(p) for p in pubs])


class OtherTau:
    """pythagorean proofs under a second SRS: the fields of vbm.Material the tests use"""

    def __init__(self, cname, count=3):
        cv, ov = CURVES[cname]
        self.cv, self.ov, self.cname, self.circuit = cv, ov, cname, "pyth"
        self.tau = tau_from_seed(TAU2_SEED, cv.r)
        g = SplitMix64(0x0707)
        c, _ = ocircuits.pythagorean(ov)
        opk = oplonk.setup(c, oplonk.synthetic_srs(ov, c.domain_size(), self.tau, materialize=False))
        self.raws, self.pubs, self.oprs = [], [], []
        for j in range(count):
            sol = ocircuits.pythagorean(ov, *vbm.PYTH[j])[1]
            L, R, O = oplonk.solve_lro(c, sol)
            opr = oplonk.prove(opk, L, R, O, sol[: c.nb_public], [g.fr(cv.r) for _ in range(9)])
            self.oprs.append(opr); self.pubs.append(list(sol[: c.nb_public])); self.raws.append(vbm.raw_proof(cv, opr))
        self.ovk = opk.vk
        self.g2 = ap_setup.g2_from_tau(cv, self.tau)
        self.vk = vbm.product_vk(cv, opk.vk, self.g2)

    def take(self, n):
        return [vbm.clone(p) for p in self.raws[:n]], [list(p) for p in self.pubs[:n]], list(self.oprs[:n])


@functools.lru_cache(maxsize=None)
def other_tau(cname) -> OtherTau:
    return OtherTau(cname)


def key_array(vks):
    arr = (_lib.VerifyingKey * max(len(vks), 1))()
    for i, vk in enumerate(vks):
        r = vk.raw()
        C.memmove(C.byref(arr, i * C.sizeof(_lib.VerifyingKey)), C.byref(r), C.sizeof(_lib.VerifyingKey))
    return arr


def run_keys(vks, key_of, raws, pubs, device=-1, nb_public=None, keys=None):
    """apk_verify_batch_keys -> (return code, statuses, trace); vks = product keys (keys = a prepared array instead)"""
    n = len(raws)
    arr = (_lib.Proof * max(n, 1))()
    for j, p in enumerate(raws):
        C.memmove(C.byref(arr, j * C.sizeof(_lib.Proof)), C.byref(p), C.sizeof(_lib.Proof))
    bufs = [(ecc.BN254 if raws[j].curve == _lib.APK_BN254 else ecc.BLS12_381).fr_vector(list(pubs[j])) for j in range(n)]
    ptrs = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bufs])
    nbs = (C.c_uint32 * max(n, 1))(*(nb_public if nb_public is not None else [len(p) for p in pubs]))
    kof = (C.c_uint32 * max(n, 1))(*key_of)
    status = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    tr = _lib.VerifyKeysTrace()
    rc = lib.apk_verify_batch_keys(device, keys if keys is not None else key_array(vks), len(vks), kof, arr, ptrs, nbs, n, status, C.byref(tr))
    return rc, [status[j] for j in range(n)], tr


def run_blobs(vks, key_of, blobs, pibs, device=-1):
    """apk_verify_blobs -> (return code, statuses, trace)"""
    n = len(blobs)
    pptr = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(b), C.c_void_p) for b in blobs])
    iptr = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(b), C.c_void_p) for b in pibs])
    plen = (C.c_size_t * max(n, 1))(*[len(b) for b in blobs])
    ilen = (C.c_size_t * max(n, 1))(*[len(b) for b in pibs])
    kof = (C.c_uint32 * max(n, 1))(*key_of)
    status = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    tr = _lib.VerifyKeysTrace()
    rc = lib.apk_verify_blobs(device, key_array(vks), len(vks), kof, pptr, plen, iptr, ilen, n, status, C.byref(tr))
    return rc, [status[j] for j in range(n)], tr


def trace_bytes(tr):
    """every byte of the trace, field by field"""
    return (bytes(tr.d), [bytes(x) for x in tr.rho], [bytes(x) for x in tr.lin_commitment], bytes(tr.a), bytes(tr.b), tr.groups, tr.folds)


def interleave(mats, per):
    """`per` proofs of each material, interleaved (proof j under key j % len(mats)): -> (key_of, raws, pubs, oprs)"""
    taken = [m.take(per) for m in mats]
    key_of, raws, pubs, oprs = [], [], [], []
    for j in range(per):
        for i, (r, p, o) in enumerate(taken):
            key_of.append(i); raws.append(r[j]); pubs.append(p[j]); oprs.append(o[j])
    return key_of, raws, pubs, oprs


def restate(mats, key_of, oprs, pubs, unreadable=()):
    """The statement of include/apk.h for apk_verify_batch_keys restated from hashlib, oracle/curves.py big-integer arithmetic and the
    challenge code of oracle/plonk.py::verify: (D, rho_j and [lin]_j of the first four proofs, A and B of the first group's fold, the
    number of groups).  mats[i] = the material of key i (.cv, .ov, .ovk, .g2)."""
    fb = oplonk.fr_bytes
    h = hashlib.sha256()
    h.update(len(mats).to_bytes(4, "big"))
    groups = []
    for m in mats:
        vk, rb = m.ovk, m.ov.raw_bytes
        h.update(m.cv.abi.to_bytes(4, "big"))
        for P in [vk.ql, vk.qr, vk.qm, vk.qo, vk.qk, vk.s[0], vk.s[1], vk.s[2]] + list(vk.qcp) + [vk.g1]:
            h.update(rb(P))
        h.update(vk.size.to_bytes(8, "big") + vk.nb_public.to_bytes(4, "big") + len(vk.qcp).to_bytes(4, "big"))
        for idx in vk.commitment_constraint_indexes:
            h.update(idx.to_bytes(4, "big"))
        h.update(m.g2)
        if (m.cv.abi, rb(vk.g1), m.g2) not in groups:
            groups.append((m.cv.abi, rb(vk.g1), m.g2))
    N = len(oprs)
    h.update(N.to_bytes(4, "big"))
    for j, (opr, pub) in enumerate(zip(oprs, pubs)):
        m = mats[key_of[j]]
        h.update((b"\x00" if j in unreadable else b"\x01") + key_of[j].to_bytes(4, "big"))
        if j in unreadable:
            continue
        for P in list(opr.lro) + [opr.z] + list(opr.h) + [opr.batched_h, opr.zshift_h] + list(opr.bsb22_commitments):
            h.update(m.ov.raw_bytes(P))
        for v in list(opr.claimed_values[1:]) + [opr.zshift_value] + list(pub):
            h.update(fb(v))
    D = h.digest()
    rho = [int.from_bytes(hashlib.sha256(b"apk-batch-keys" + D + j.to_bytes(4, "big")).digest()[16:], "big") for j in range(N)]
    gid_of = lambda m: (m.cv.abi, m.ov.raw_bytes(m.ovk.g1), m.g2)
    with_proofs = [gid_of(mats[key_of[j]]) for j in range(N) if j not in unreadable]
    first = next((g for g in groups if g in with_proofs), None)      # the first group with a proof to fold
    A, B, lins, fold_ov = None, None, [], None
    for j, (opr, pub) in enumerate(zip(oprs, pubs)):
        m = mats[key_of[j]]
        ov, q, vk, rb = m.ov, m.ov.r, m.ovk, m.ov.raw_bytes
        if j in unreadable:
            lins.append(bytes(_lib.G1_MAX))
            continue
        T = {}
        assert oplonk.verify(vk, oplonk.marshal_proof(ov, opr), oplonk.marshal_public_inputs(pub), trace_out=T)
        zeta, gk, c, lin_raw = T["zeta"], T["gamma_kzg"], T["folded_claims"], T["lin_poly_com"]
        lins.append(vbm.pad_pt(m.cv, lin_raw))
        if gid_of(m) != first:
            continue
        fold_ov = ov
        zw = opr.zshift_value
        rr = int.from_bytes(hashlib.sha256(b"random" + fb(gk) + rb(opr.z) + rb(opr.batched_h) + rb(opr.zshift_h) + fb(c) + fb(zw)).digest(), "big") % q
        Aj, g = ov.from_raw_bytes(lin_raw), gk
        for P in list(opr.lro) + [vk.s[0], vk.s[1]] + list(vk.qcp):     # the key's own S1, S2, Qcp_i: proof by proof here, per key in the library
            Aj = ov.add(Aj, ov.mul(P, g))
            g = g * gk % q
        Aj = ov.add(Aj, ov.mul(opr.z, rr))
        Aj = ov.add(Aj, ov.neg(ov.mul(vk.g1, (c + rr * zw) % q)))
        Aj = ov.add(Aj, ov.mul(opr.batched_h, zeta))
        Aj = ov.add(Aj, ov.mul(opr.zshift_h, rr * zeta % q * vk.generator % q))
        Bj = ov.neg(ov.add(opr.batched_h, ov.mul(opr.zshift_h, rr)))
        A = ov.add(A, ov.mul(Aj, rho[j]))
        B = ov.add(B, ov.mul(Bj, rho[j]))
    pad4 = lambda xs, zero: (xs + [zero] * 4)[:4]
    ab = lambda P: bytes(_lib.G1_MAX) if fold_ov is None else vbm.pad_pt(None, oplonk.rb_ec(fold_ov, P))
    return (D, pad4([fb(x) for x in rho], bytes(32)), pad4(lins, bytes(_lib.G1_MAX)), ab(A), ab(B), len(groups))

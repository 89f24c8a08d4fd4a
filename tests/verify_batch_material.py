"""Proof material for the batch-verifier tests (test_verify_batch.py, test_gpu_verify_batch.py) and tools/verify_batch_bench.py.

Material: oracle proofs of the circuits tests/test_verify_host.py uses (pythagorean / identity / square / random chain and the
k = 1, 2 BSB22 circuits), several per circuit with distinct witnesses and blinding, as apk_proof structs.
"""
import ctypes as C
import functools

from algoplonk_amd import _lib, plonk as ap_plonk, setup as ap_setup
from algoplonk_amd._lib import lib
from oracle import circuits as ocircuits, plonk as oplonk
from oracle.prng import SplitMix64, tau_from_seed

from helpers import CURVES

TAU_SEED = 0x7E57
PYTH = [(3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29), (9, 40, 41), (12, 35, 37), (11, 60, 61)]


def product_vk(cv, ovk, g2_bytes) -> ap_plonk.VerifyingKey:
    return ap_plonk.VerifyingKey(curve=cv, Size=ovk.size, SizeInv=ovk.size_inv, Generator=ovk.generator, CosetShift=ovk.coset_shift,
                                 NbPublicVariables=ovk.nb_public, Ql=ovk.ql, Qr=ovk.qr, Qm=ovk.qm, Qo=ovk.qo, Qk=ovk.qk, S=list(ovk.s),
                                 Qcp=list(ovk.qcp), CommitmentConstraintIndexes=list(ovk.commitment_constraint_indexes), KzgG1=ovk.g1,
                                 tau=None, KzgG2=g2_bytes)


def raw_proof(cv, opr) -> _lib.Proof:
    p = _lib.Proof()
    p.curve, p.nb_commitments = cv.abi, len(opr.bsb22_commitments)

    def pt(slot, P):
        b = cv.g1_to_bytes(P)
        C.memmove(slot, b, len(b))

    def fr(slot, x):
        C.memmove(slot, cv.fr_to_mont_bytes(x), 32)

    for j in range(3):
        pt(p.lro[j], opr.lro[j]); pt(p.h[j], opr.h[j])
    pt(p.z, opr.z); pt(p.batched_h, opr.batched_h); pt(p.zshift_h, opr.zshift_h)
    for k, P in enumerate(opr.bsb22_commitments):
        pt(p.bsb22[k], P)
    for i, v in enumerate(opr.claimed_values):
        fr(p.claimed_values[i], v)
    fr(p.zshift_value, opr.zshift_value)
    return p


def clone(p: _lib.Proof) -> _lib.Proof:
    q = _lib.Proof()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(_lib.Proof))
    return q


def _resolve_chain(c, seeds):
    """another solution of a random-chain circuit: new publics / secret seeds, every gate's output recomputed"""
    r = c.curve.r
    sol = list(seeds)
    for (ql, qr, qm, qo, qk, xa, xb, xc) in c.constraints:
        assert xc == len(sol) and qo == r - 1
        sol.append((ql * sol[xa] + qr * sol[xb] + qm * sol[xa] % r * sol[xb] + qk) % r)
    return sol


class Material:
    """`count` proofs of one circuit: .vk (product key), .ovk, .raws (apk_proof), .pubs (ints), .oprs (oracle proofs)"""

    def __init__(self, cname, circuit, count):
        cv, ov = CURVES[cname]
        self.cv, self.ov, self.cname, self.circuit = cv, ov, cname, circuit
        self.tau = tau_from_seed(TAU_SEED, cv.r)
        g = SplitMix64(0xBA7C4 + count)
        self.raws, self.pubs, self.oprs = [], [], []
        if circuit in ("bsb1", "bsb2"):
            k = int(circuit[-1])
            opk = None
            for j in range(count):
                y = 3 + j
                c, sol, plan = ocircuits.bsb22_square(ov, k, x=y * y, y=y)
                n = c.domain_size()
                osrs = oplonk.synthetic_srs(ov, n, self.tau, materialize=False)
                if opk is None:
                    opk = oplonk.setup(c, osrs)
                wn = ov.omega(n)
                sol, pi2 = ocircuits.solve_bsb22(c, sol, plan, lambda col: osrs.commit(oplonk.intt(col, wn, cv.r)),
                                                 [(g.fr(cv.r), g.fr(cv.r)) for _ in range(k)])
                L, R, O = oplonk.solve_lro(c, sol)
                self._add(opk, L, R, O, sol[:1], [g.fr(cv.r) for _ in range(9)], pi2)
        else:
            if circuit == "pyth":
                c, _ = ocircuits.pythagorean(ov)
                sols = [ocircuits.pythagorean(ov, *PYTH[j % len(PYTH)])[1] for j in range(count)]
            elif circuit == "id":
                c, _ = ocircuits.identity(ov)
                sols = [ocircuits.identity(ov, 7 + j)[1] for j in range(count)]
            elif circuit == "sq":
                c, _ = ocircuits.square(ov)
                sols = [ocircuits.square(ov, (3 + j) ** 2, 3 + j)[1] for j in range(count)]
            else:
                c, sol0 = ocircuits.random_chain(ov, 4, 0xA190)
                sols = [sol0] + [_resolve_chain(c, [g.fr(cv.r) for _ in range(c.nb_public + 2)]) for _ in range(count - 1)]
            opk = oplonk.setup(c, oplonk.synthetic_srs(ov, c.domain_size(), self.tau, materialize=False))
            for sol in sols:
                L, R, O = oplonk.solve_lro(c, sol)
                self._add(opk, L, R, O, sol[: c.nb_public], [g.fr(cv.r) for _ in range(9)], None)
        self.ovk = opk.vk
        self.g2 = ap_setup.g2_from_tau(cv, self.tau)
        self.vk = product_vk(cv, opk.vk, self.g2)

    def _add(self, opk, L, R, O, pub, bl, pi2):
        opr = oplonk.prove(opk, L, R, O, pub, bl, pi2=pi2) if pi2 is not None else oplonk.prove(opk, L, R, O, pub, bl)
        self.oprs.append(opr); self.pubs.append(list(pub)); self.raws.append(raw_proof(self.cv, opr))

    def take(self, n):
        """n proofs (cycling through the distinct ones when n is larger): raws (fresh copies), pubs, oprs"""
        idx = [j % len(self.raws) for j in range(n)]
        return [clone(self.raws[i]) for i in idx], [list(self.pubs[i]) for i in idx], [self.oprs[i] for i in idx]


@functools.lru_cache(maxsize=None)
def material(cname, circuit, count=8) -> Material:
    return Material(cname, circuit, count)


def run_batch(vk, raws, pubs, device=-1, nb_public=None):
    """apk_verify_batch -> (return code, statuses, trace)"""
    cv = vk.curve
    n = len(raws)
    arr = (_lib.Proof * max(n, 1))()
    for j, p in enumerate(raws):
        C.memmove(C.byref(arr, j * C.sizeof(_lib.Proof)), C.byref(p), C.sizeof(_lib.Proof))
    bufs = [cv.fr_vector(list(p)) for p in pubs]
    ptrs = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bufs])
    nbs = (C.c_uint32 * max(n, 1))(*(nb_public if nb_public is not None else [len(p) for p in pubs]))
    status = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    tr = _lib.VerifyBatchTrace()
    rv = vk.raw()
    rc = lib.apk_verify_batch(device, C.byref(rv), arr, ptrs, nbs, n, status, C.byref(tr))
    return rc, [status[j] for j in range(n)], tr


def trace_bytes(tr, count):
    m = min(count, 4)
    return (bytes(tr.d), [bytes(tr.rho[j]) for j in range(m)], [bytes(tr.lin_commitment[j]) for j in range(m)], bytes(tr.a), bytes(tr.b))


def pad_pt(cv, raw: bytes) -> bytes:
    return raw + bytes(_lib.G1_MAX - len(raw))


def lincomb(cv, device, points, scalars, seg):
    """apk_g1_lincomb_segments -> (return code, list of points)"""
    nseg = len(seg) - 1
    out = C.create_string_buffer(max(nseg, 1) * 2 * cv.fp_bytes)
    segs = (C.c_uint64 * len(seg))(*seg)
    rc = lib.apk_g1_lincomb_segments(cv.abi, device, cv.g1_vector(points), cv.fr_vector(scalars), segs, nseg, out)
    w = 2 * cv.fp_bytes
    return rc, [cv.g1_from_bytes(out.raw[i * w: (i + 1) * w]) for i in range(nseg)]


def lincomb_reference(ov, points, scalars, seg):
    out = []
    for s in range(len(seg) - 1):
        acc = None
        for i in range(seg[s], seg[s + 1]):
            acc = ov.add(acc, ov.mul(points[i], scalars[i]))
        out.append(acc)
    return out

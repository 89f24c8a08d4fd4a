"""The carry-save forms of ffu.h (sums and differences left unswept where a product absorbs the carries), the quotient-estimate
reduction reduce_2p, and the kernels that use them (tests/carry_save_model.py states each contract).

CPU tier: the host seam against the big-integer model, limb for limb, at the edges each call site allows; products on operands
at the stated limb bounds against the products of the swept operands; the reduction at every multiple of p and at the rounding
boundaries of its estimate; long madd_lazy chains with the lazy class checked after every step.
GPU tier: device == host for the same records; the transforms (radix 4 on and off, semi-canonical hand-off), the MSM and whole
proofs against the C oracle, with the lone and the loaded forms."""
from __future__ import annotations

import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from algoplonk_amd._lib import check, lib

import carry_save_model as cs
import limb_model as lm
from helpers import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [(c, f) for c in ("bn254", "bls12-381") for f in (0, 1)]
FIELD_IDS = ["%s-%s" % (c, "fp" if f else "fr") for c, f in FIELDS]


def _field(cname, fld):
    return lm.field(CURVES[cname][0], fld)


def _shapes(f, bound, factor=1):
    """limb vectors for a value class [0, bound): 0, 1, p - 1 and the class maximum as normalised values, every limb at the
    maximum of the limb factor, and every limb zero except the top"""
    lower = cs.value(f, cs.all_max(f, factor, 0))
    out = [cs.normalised(f, v) for v in (0, 1, f.p - 1, bound - 1) if v < bound]
    if lower < bound:
        out.append(cs.all_max(f, factor, cs.top_below(f, bound, lower)))
    out.append(cs.top_only(f, cs.top_below(f, bound, 0)))
    return out


def _mont2(f, a, b, c=0, d=0):
    """(a b + c d + m p) / R' with m = -(a b + c d) / p mod R': what mul_nr / mul2_nr compute, as a value"""
    t = a * b + c * d
    m = (-t * pow(f.p, -1, f.Rp)) % f.Rp
    return (t + m * f.p) // f.Rp


# ---- the cases: (seam code, rows of operand limb vectors, expected limb vectors) ---------------------------------------------------
def _form_cases(f):
    """add_s / sub_s<2> / neg_s<2> / sub_n<2> at what their call sites allow (kernels_ntt.h: x0 below 64p, x1 below 1.91p;
    ec.h: X3 below 5.1p, Q below 1.1p, q.y canonical)"""
    p = f.p
    wide = _shapes(f, 64 * p)
    prod = _shapes(f, 191 * p // 100)
    cases = []
    rows = [(a, b) for a in wide for b in prod]
    cases.append((cs.OP_ADD_S, rows, [cs.add_s(f, a, b) for a, b in rows]))
    # a - b + 2p at least 0.09p: far above what the top limb needs (carry_save_model.min_value_for_top)
    assert 2 * p - 191 * p // 100 > cs.min_value_for_top(f, cs.sub_s_factor(1, 1))
    cases.append((cs.OP_SUB_S2, rows, [cs.sub_s(f, 2, a, b) for a, b in rows]))
    rows1 = [(a,) for a in _shapes(f, p + 1)]
    cases.append((cs.OP_NEG_S2, rows1, [cs.neg_s(f, 2, a) for (a,) in rows1]))
    # the second stage of the radix-4 step: y1 of limb factor 3 (value at least 0.09p) minus a product
    y1 = [cs.sub_s(f, 2, a, b) for a, b in rows] + [cs.all_max(f, 3, cs.top_below(f, 66 * p, cs.value(f, cs.all_max(f, 3, 0))))]
    rows3 = [(a, b) for a in y1 for b in prod]
    cases.append((cs.OP_SUB_N2, rows3, [cs.sub_n(f, 2, a, b) for a, b in rows3]))
    return cases


def _product_cases(f):
    """mul_nr / mul2_nr with one operand of each pair at a limb factor the budget accepts, every limb maximal: the result is the
    product of the VALUES - what the swept operand gives - limb for limb"""
    p = f.p
    cases = []
    gmax = max(g for g in range(1, 1 << (32 - f.B)) if cs.mul_takes(f, 1, g))
    g2max = max(g for g in range(1, 1 << (32 - f.B)) if cs.mul2_takes(f, 1, g, 1, g))
    assert cs.mul_takes(f, 1, 3) and cs.mul2_takes(f, 1, 3, 1, 1) and gmax >= 3 and g2max >= 2
    R = cs.all_max(f, 1, cs.top_below(f, 31 * p // 10, cs.value(f, cs.all_max(f, 1, 0))))      # R below 3.1p
    Y = cs.all_max(f, 1, cs.top_below(f, 4 * p, cs.value(f, cs.all_max(f, 1, 0))))             # Y up to 4p
    PPP = cs.all_max(f, 1, cs.top_below(f, 11 * p // 10, cs.value(f, cs.all_max(f, 1, 0))))
    rows, rows2 = [], []
    for g in sorted({2, 3, gmax}):
        T = cs.all_max(f, g, cs.top_below(f, 71 * p // 10, cs.value(f, cs.all_max(f, g, 0))))   # T below 7.1p
        rows += [(R, T), (T, R), (cs.top_only(f, R[-1]), T)]
    for g in sorted({2, 3, g2max}):
        if not cs.mul2_takes(f, 1, g, 1, 1):
            continue
        T = cs.all_max(f, g, cs.top_below(f, 71 * p // 10, cs.value(f, cs.all_max(f, g, 0))))
        rows2.append((R, T, Y, PPP))
        if cs.mul2_takes(f, 1, g, 1, g):     # both pairs at the bound: the case that proves the column budget
            rows2.append((R, T, PPP, cs.all_max(f, g, cs.top_below(f, 4 * p, cs.value(f, cs.all_max(f, g, 0))))))
    v = lambda x: cs.value(f, x)
    cases.append((cs.OP_MUL_NR, rows, [cs.normalised(f, _mont2(f, v(a), v(b))) for a, b in rows]))
    cases.append((cs.OP_MUL2_NR, rows2, [cs.normalised(f, _mont2(f, v(a), v(b), v(c), v(d))) for a, b, c, d in rows2]))
    return cases


def _reduce_inputs(f, K):
    p, lo_bits = f.p, f.B * (f.L - 1)
    vals = {2 * K * p - 1}
    for k in range(2 * K + 1):
        vals.update({k * p - 1, k * p, k * p + 1})
    for t in cs.estimate_boundaries(f, K):
        vals.update({t << lo_bits, (t << lo_bits) | ((1 << lo_bits) - 1)})
    return sorted(v for v in vals if 0 <= v < 2 * K * p)


def _check(f, code, rows, want, device=None):
    out = cs.run(f, code, cs.records(f, rows), device=device)
    for ops, w, got in zip(rows, want, out):
        assert [int(x) for x in got] == list(w), ("%s op %d" % (f, code), [[hex(x) for x in o] for o in ops])
    return out


# ---- CPU tier -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,fld", FIELDS, ids=FIELD_IDS)
def test_column_budgets_follow_from_the_limb_shape(cname, fld):
    """mul_takes / mul2_takes / sqr_takes are what L and B give (no field's numbers written down), and they accept what the call
    sites use: a twiddle times a sum (2) or a difference (3), mul2_nr with T unswept; the squares keep swept inputs where the
    doubled operand would not fit its word."""
    f = _field(cname, fld)
    rows = [([fa, fb, fc, fd] + [0] * (f.L - 4),) for fa in range(1, 9) for fb in range(1, 9) for fc in (1, 2, 3) for fd in (1, 3)]
    out = cs.run(f, cs.OP_TAKES, cs.records(f, rows))
    for (r,), got in zip(rows, out):
        fa, fb, fc, fd = r[:4]
        assert [int(x) for x in got[:4]] == [int(cs.mul_takes(f, fa, fb)), int(cs.mul2_takes(f, fa, fb, fc, fd)),
                                             int(cs.sqr_takes(f, fa)), cs.column_room(f)], (str(f), fa, fb, fc, fd)
    assert cs.mul_takes(f, 1, cs.add_s_factor(1, 1)) and cs.mul_takes(f, 1, cs.sub_s_factor(1, 1)) and cs.mul_takes(f, cs.neg_s_factor(1), 1)
    assert cs.mul2_takes(f, 1, cs.sub_s_factor(1, 1), 1, 1)
    assert 3 * f.L + 1 <= cs.column_room(f)           # the assertion ffu.h had before: mul2_nr on normalised limbs


@pytest.mark.parametrize("cname,fld", FIELDS, ids=FIELD_IDS)
def test_carry_save_forms_match_the_model_limb_for_limb(cname, fld):
    f = _field(cname, fld)
    for code, rows, want in _form_cases(f):
        out = _check(f, code, rows, want)
        if code == cs.OP_SUB_N2:
            assert (out[:, : f.L - 1] <= f.mask).all()


@pytest.mark.parametrize("cname,fld", FIELDS, ids=FIELD_IDS)
def test_products_absorb_the_carries_of_their_operands(cname, fld):
    """A product of an operand at its limb bound, every limb maximal, is bit for bit the product of the swept operand."""
    f = _field(cname, fld)
    for code, rows, want in _product_cases(f):
        out = _check(f, code, rows, want)
        swept = [tuple(cs.normalised(f, cs.value(f, x)) for x in ops) for ops in rows]
        assert (cs.run(f, code, cs.records(f, swept)) == out).all()
        assert (out[:, : f.L - 1] <= f.mask).all()


@pytest.mark.parametrize("K", [4, 8, 32])
@pytest.mark.parametrize("cname,fld", FIELDS, ids=FIELD_IDS)
def test_quotient_estimate_reduction(cname, fld, K):
    """reduce_2p<K> on k p - 1, k p, k p + 1 for every k up to 2K, on 2K p - 1 and on values whose top limb sits where the estimate
    steps: the result is congruent, in [0, 2p), normalised (the top limb included), the model's limbs; canon<1> of it is
    canon<K> of the input."""
    f = _field(cname, fld)
    vals = _reduce_inputs(f, K)
    rows = [(cs.normalised(f, v),) for v in vals]
    want = [cs.reduce_2p(f, a) for (a,) in rows]
    out = _check(f, cs.OP_REDUCE_2P[K], rows, want)
    assert (out <= f.mask).all()
    for v, got in zip(vals, out):
        g = cs.value(f, got)
        assert 0 <= g < 2 * f.p and (g - v) % f.p == 0, (str(f), K, hex(v))
    canon_k = cs.run(f, cs.OP_CANON[K], cs.records(f, rows))
    assert (cs.run(f, cs.OP_CANON[1], cs.records(f, [(list(map(int, r)),) for r in out])) == canon_k).all()
    assert [cs.value(f, r) for r in canon_k] == [v % f.p for v in vals]
    if K == 32:
        assert (cs.run(f, cs.OP_REDUCE_CANON32, cs.records(f, rows)) == canon_k).all()


def test_new_ops_leave_the_gaps_rejected():
    cv, _ = CURVES["bn254"]
    rec, out = np.zeros((1, 36), dtype=np.uint32), np.zeros((1, 9), dtype=np.uint32)
    for op in (30, 39, 49):
        assert lib.apk_host_feu_op(cv.abi, 0, op, 1, rec.ctypes.data, out.ctypes.data) != 0
        assert lib.apk_device_feu_op(cv.abi, 0, op, 0, 1, rec.ctypes.data, out.ctypes.data) != 0      # checked before any launch
    buf = C.create_string_buffer(128)
    assert lib.apk_host_g1_op(cv.abi, 16, buf, buf, buf) != 0


CHAIN_STEPS = 320


def _chain_reference(ov, a, b):
    """g1 op 15's script (selftest_ops.h) on the oracle's group law"""
    state, cur = None, a
    for i in range(CHAIN_STEPS):
        pt, negate = cur, bool(i & 1) if i < 160 else bool((i >> 4) & 1)
        if i < 4:
            pt, negate = a, i == 1
        if i in (200, 260) and state is not None:
            pt, negate = state, i == 200
        state = ov.add(state, ov.neg(pt) if negate else pt)
        cur = ov.add(cur, b)
    return state


@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_madd_lazy_chains_stay_in_the_lazy_class(cname):
    """320 signed mixed additions through madd_lazy per pair - alternating signs, then runs of sixteen - with a cancellation and
    a doubling under unit_z at the start and again with ZZ != 1 later (state == -q at step 200, state == q at step 260).  The op
    checks the documented class (X < 5.1p, Y <= 4p, ZZ, ZZZ < 1.4p, limbs normalised, infinity <=> the plain chain's) after every
    step and reports a violation as an all-ones record; the final point must be the group's."""
    cv, ov = CURVES[cname]
    rnd = random.Random(23)
    out = C.create_string_buffer(2 * cv.fp_bytes)
    for _ in range(3):
        a, b = ov.mul(ov.g1, rnd.randrange(1, cv.r)), ov.mul(ov.g1, rnd.randrange(1, cv.r))
        check(lib.apk_host_g1_op(cv.abi, 15, cv.g1_to_bytes(a), cv.g1_to_bytes(b), out))
        assert out.raw != b"\xff" * len(out.raw), "a state left the lazy class"
        assert cv.g1_from_bytes(out.raw) == _chain_reference(ov, a, b)


# ---- GPU tier -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cname,fld", FIELDS, ids=FIELD_IDS)
def test_carry_save_ops_device_equal_host(gpu, cname, fld):
    """The same records on the device (whose BN254 base-field products are the generated chains of ffu_asm.h): the model's limbs
    for the forms and the products, the host's for the reductions."""
    f = _field(cname, fld)
    for code, rows, want in _form_cases(f) + _product_cases(f):
        _check(f, code, rows, want, device=gpu)
    for K in (4, 8, 32):
        rows = [(cs.normalised(f, v),) for v in _reduce_inputs(f, K)]
        _check(f, cs.OP_REDUCE_2P[K], rows, [cs.reduce_2p(f, a) for (a,) in rows], device=gpu)
    rows = [(cs.normalised(f, v),) for v in _reduce_inputs(f, 32)]
    recs = cs.records(f, rows)
    assert (cs.run(f, cs.OP_REDUCE_CANON32, recs, device=gpu) == cs.run(f, cs.OP_CANON[32], recs)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_madd_lazy_chains_on_the_device(gpu, cname):
    cv, ov = CURVES[cname]
    rnd = random.Random(29)
    g1b = 2 * cv.fp_bytes
    pairs = [(ov.mul(ov.g1, rnd.randrange(1, cv.r)), ov.mul(ov.g1, rnd.randrange(1, cv.r))) for _ in range(3)]
    out = C.create_string_buffer(len(pairs) * g1b)
    check(lib.apk_device_g1_op(cv.abi, 15, gpu, len(pairs), b"".join(cv.g1_to_bytes(a) for a, _ in pairs),
                               b"".join(cv.g1_to_bytes(b) for _, b in pairs), out))
    for i, (a, b) in enumerate(pairs):
        raw = out.raw[i * g1b:(i + 1) * g1b]
        assert raw != b"\xff" * g1b, "a state left the lazy class"
        assert cv.g1_from_bytes(raw) == _chain_reference(ov, a, b)


# One process per form (the knobs are read once): the transforms at 2^10 and 2^12 (4n of n = 2^8 and 2^10: two passes of 512-element
# tiles each), an MSM over 2^10 bases and whole proofs, all against the C oracle.
_KERNEL_SCRIPT = r"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from algoplonk_amd import MarshalProof, frontend, plonk, setup
from algoplonk_amd._lib import lib, check
from oracle import c_oracle
from oracle.prng import SplitMix64, tau_from_seed
from helpers import CURVES, blinding, oracle_threads, random_chain_ccs
import limb_model as lm
import msm_model as mm
form = sys.argv[1]
clib = c_oracle.load()
fails = []

def oracle_proof(cv, ccs, srs, sol, w, bl):
    tr = frontend.build_trace(ccs)
    L, R, O = frontend.wire_columns(ccs, sol)
    rc, want, _ = c_oracle.prove(clib, cv.abi, ccs.domain_size(), ccs.GetNbPublicVariables(), srs.g1,
                                 [cv.fr_vector(x) for x in (tr.ql, tr.qr, tr.qm, tr.qo, tr.qk)], tr.perm, cv.fr_vector(L),
                                 cv.fr_vector(R), cv.fr_vector(O), cv.fr_vector(w.public), cv.fr_vector(bl), threads=oracle_threads())
    assert rc == 0
    return want

for cname in ("bn254", "bls12-381"):
    cv, ov = CURVES[cname]
    r, u = cv.r, ov.coset_shift
    for log_n in (8, 10):
        ccs, w, sol = random_chain_ccs(cv, log_n, 0xC5 + log_n)
        n = ccs.domain_size()
        srs = setup.unsafe_srs(cv, n, tau_from_seed(0xC5, r), device=0)
        pk, vk = plonk.Setup(ccs, srs, device=0)
        size, log_size = 4 * n, log_n + 2
        g = SplitMix64(log_n)
        ui = pow(u, -1, r)
        for inverse, coset in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1)):
            top = lm.ntt_top_growth_input(ov, log_size, bool(inverse))
            if coset and not inverse:          # divided by the coset powers, so the pre-multiplied data are the plain case's
                top = [v * pow(ui, i, r) % r for i, v in enumerate(top)]
            for name, vals in (("top growth", top), ("all p-1", [r - 1] * size), ("random", [g.fr(r) for _ in range(size)])):
                data = b"".join(v.to_bytes(32, "little") for v in vals)
                a_buf, b_buf = C.create_string_buffer(data, len(data)), C.create_string_buffer(data, len(data))
                assert clib.orc_ntt(cv.abi, a_buf, size, inverse, 1 if coset else 0) == 0
                check(lib.apk_ntt(pk.ctx, 1, inverse, coset, b_buf))
                if coset == 2:                 # semi-canonical: below 2r, the oracle's residues
                    got = [int.from_bytes(b_buf.raw[32 * i: 32 * i + 32], "little") for i in range(size)]
                    want = [int.from_bytes(a_buf.raw[32 * i: 32 * i + 32], "little") for i in range(size)]
                    ok = all(x < 2 * r and x % r == y for x, y in zip(got, want))
                else:
                    ok = b_buf.raw == a_buf.raw
                if not ok:
                    fails.append("ntt %s 2^%d %s inverse=%d coset=%d" % (cname, log_size, name, inverse, coset))
        if log_n == 10:
            # MSM over the 2^10 canonical bases: raw words as the kernels split them (basis 0)
            c = pk.msm_window
            lay = mm.plan(mm.curve_bits(cname), mm.CURVE_PARAMS[cname][1], c, log_n, n + 3).lay
            edges = mm.edge_scalars(r, lay, "raw", seed=c).values
            for name, words in (("all r-1", [r - 1] * n), ("digit edges", [edges[i % len(edges)] for i in range(n)]),
                                ("random", [g.fr(r) for _ in range(n)])):
                buf = b"".join(m.to_bytes(32, "little") for m in words)
                out, want = C.create_string_buffer(2 * cv.fp_bytes), C.create_string_buffer(2 * cv.fp_bytes)
                assert clib.orc_msm(cv.abi, srs.g1, buf, n, oracle_threads(), want) == 0
                check(lib.apk_msm_g1(pk.ctx, 0, buf, n, out))
                if out.raw != want.raw:
                    fails.append("msm %s %s" % (cname, name))
            bl = blinding(cv, 3)
            if MarshalProof(plonk.Prove(ccs, pk, w, bl)) != oracle_proof(cv, ccs, srs, sol, w, bl):
                fails.append("proof %s 2^%d" % (cname, log_n))
        pk.close()
if form == "loaded":
    cv, ov = CURVES["bn254"]
    ccs, w, sol = random_chain_ccs(cv, 12, 0xC5 + 12)
    srs = setup.unsafe_srs(cv, ccs.domain_size(), tau_from_seed(0xC5, cv.r), device=0)
    pk, vk = plonk.Setup(ccs, srs, device=0, msm_window=16, slots=3)
    bl = blinding(cv, 4)
    if MarshalProof(plonk.Prove(ccs, pk, w, bl)) != oracle_proof(cv, ccs, srs, sol, w, bl):
        fails.append("proof bn254 2^12, loaded forms")
    paths = pk.paths(reset=True)
    if not (paths["ntt_radix4"] and paths["msm_lean_tail"]):
        fails.append("the loaded forms did not run: %s" % paths)
    pk.close()
for f in fails[:40]:
    print("FAIL", f)
print("KERNELS_DONE %d failures" % len(fails))
sys.exit(1 if fails else 0)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lone", "loaded"])
def test_transforms_msm_and_proofs_against_the_c_oracle(gpu, form):
    """Both curves.  Transforms of 2^10 and 2^12 points - plain, on the coset, on the coset in the prover's semi-canonical form
    (apk_ntt coset = 2: every word below 2r and congruent to the oracle's), inverse, inverse from the coset - on the input that
    drives the last output to the top of the lazy range (limb_model.ntt_top_growth_input), on all p - 1 and on random words.  An
    MSM over 2^10 bases on all r - 1, on the signed-digit edge words of the context's window and on random words.  One proof at
    2^10 per curve, bytes equal to the C oracle's.  `loaded` forces the forms the library takes with other proofs in flight
    (radix-4 steps, lean tail kernels, no tail-filling side stream) and adds a BN254 proof at 2^12 with 16-bit windows, where the
    lean merge is really taken."""
    env = dict(os.environ)
    env.pop("APK_MSM_WINDOW", None)
    if form == "loaded":
        env.update({"APK_NTT_RADIX4": "1", "APK_MSM_LEAN_TAIL": "1", "APK_TAIL_FILL": "0"})
    else:
        env.update({"APK_NTT_RADIX4": "0"})
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _KERNEL_SCRIPT, form], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "KERNELS_DONE 0 failures" in out.stdout, (out.stdout[-4000:], out.stderr[-2000:])

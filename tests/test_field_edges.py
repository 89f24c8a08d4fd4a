"""Field and curve primitives at their limb and lazy-bound edges (tests/limb_model.py states each op's contract).

CPU tier: every raw unsaturated-limb op (ffu.h FeU) on the host seam, all four fields, against the big-integer model, on edge
operands (0, 1, k p +- 1 for every multiple the input class allows, the class maximum, all-MASK lower limbs, powers of the
limb radix) and a random bulk; the host curve templates at extreme points.
GPU tier: the same seams on the device, whose compile takes other branches (the MacChain product of ff.h, the generated
ffu_asm.h chains, the four-lane DPP point forms): device bytes == host bytes bit for bit, and the model / oracle on top; and
the NTT on adversarial inputs at one-pass, two-pass, >= 2^14 and forced radix-4 sizes."""
import ctypes as C
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

from algoplonk_amd import _lib
from algoplonk_amd._lib import lib, check
from oracle.curves import sqrt_mod

import limb_model as lm
from helpers import CURVES

FIELDS = [(c, f) for c in ("bn254", "bls12-381") for f in (0, 1)]
FIELD_IDS = ["%s-%s" % (c, "fp" if f else "fr") for c, f in FIELDS]
N_RANDOM_HOST = 2048          # model-checked random operands per op (CPU tier)
N_RANDOM_DEVICE = 1 << 16     # random operands per op compared bit for bit host vs device (GPU tier)


def _field(cname, fld):
    return lm.field(CURVES[cname][0], fld)


# ---- CPU tier: the contracts themselves ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,fld", FIELDS, ids=FIELD_IDS)
def test_headroom_is_what_the_lazy_forms_assume(cname, fld):
    """HEADROOM <= R'/p (a product of operands below A p and C p with A C <= HEADROOM stays below 2p), and at least what the
    users assert: the lazy point class (ec.h, Fp) needs 160, the NTT (kernels_ntt.h, Fr) 64."""
    f = _field(cname, fld)
    assert f.H * f.p <= f.Rp < (f.H + 1) * f.p * 2
    assert f.H >= (160 if fld else 64)
    assert f.N * 32 <= f.B * f.L and (3 * f.L + 1) <= 1 << (64 - 2 * f.B)   # packing fits; mul2_nr's column sums fit 64 bits
    # the top limb of p leaves room for the widest lazy value any op takes (H p below R', so below 2^B in the top limb)
    assert (f.H * f.p) >> (f.B * (f.L - 1)) < 1 << f.B


@pytest.mark.parametrize("op", [o.name for o in lm.OPS])
@pytest.mark.parametrize("cname,fld", FIELDS, ids=FIELD_IDS)
def test_unsaturated_ops_host_match_model(cname, fld, op):
    f, o = _field(cname, fld), lm.OPS_BY_NAME[op]
    xs = lm.operands(f, o, N_RANDOM_HOST, seed=zlib.crc32(("%s/%d/%s" % (cname, fld, op)).encode()))
    out = lm.run(f, o, lm.pack_records(f, o, xs))
    bad = lm.violations(f, o, xs, out)
    assert not bad, "\n".join(bad)


def _extreme_points(cv, ov):
    """points with extreme coordinates: the smallest x (as a value and as gnark's Montgomery word) for which x^3 + b is a square,
    the largest such x below p, each with the small root and its negation (y close to p)"""
    p, R = ov.p, cv.fp_R

    def lift(x):
        y = sqrt_mod((x * x * x + ov.b) % p, p)
        if y is None:
            return None
        y = min(y, p - y)
        return [(x, y), (x, p - y)]

    pts = []
    for xs in (range(0, 1000), (k * pow(R, -1, p) % p for k in range(1, 1000)), range(p - 1, p - 1000, -1)):
        for x in xs:
            got = lift(x)
            if got:
                pts += got
                break
    for P in pts:
        assert ov.is_on_curve(P)
    return pts


def _g1_cases(cv, ov, rnd):
    """(op, P, q, expected) over the special cases: equal / opposite operands, infinity, extreme coordinates"""
    ext = _extreme_points(cv, ov)
    gen = [ov.mul(ov.g1, rnd.randrange(1, cv.r)) for _ in range(2)]
    pts = ext + gen
    cases = []
    for P in pts:
        for Q in (P, ov.neg(P), None, gen[0], ext[0], ext[-1]):
            for op in (0, 1, 10, 11):
                cases.append((op, P, Q, ov.add(P, Q)))
            for op in (12, 13):
                cases.append((op, P, Q, ov.add(P, ov.mul(Q, 3)) if Q is not None else P))
            cases.append((14, P, Q, ov.add(ov.mul(P, 4), ov.mul(Q, 6)) if Q is not None else None))
        cases.append((2, P, None, ov.add(P, P)))
        for k in (0, 1, 2, cv.r - 1, cv.r - 2, rnd.randrange(cv.r)):
            cases.append((3, P, k, ov.mul(P, k)))
    cases.append((0, None, gen[0], gen[0]))
    cases.append((2, None, None, None))
    return cases


def _q_bytes(cv, op, q):
    return cv.fr_to_mont_bytes(q) if op == 3 else cv.g1_to_bytes(q)


@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_host_curve_ops_at_extreme_points(cname):
    cv, ov = CURVES[cname]
    out = C.create_string_buffer(2 * cv.fp_bytes)
    for op, P, q, want in _g1_cases(cv, ov, random.Random(3)):
        if op == 14 and q is None:
            continue            # op 14 takes two finite points (its chain doubles both)
        check(lib.apk_host_g1_op(cv.abi, op, cv.g1_to_bytes(P), None if op == 2 else _q_bytes(cv, op, q), out))
        assert cv.g1_from_bytes(out.raw) == want, (cname, op, P, q)


@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_host_lazy_point_chains_over_many_points(cname):
    """The lazy mixed addition (ops 12) and the lazy full addition / doubling (14) over many random pairs: the lazy class's
    bounds (X < 5.1p, Y <= 4p, ...) are reached only by some points, and a multiple of p too small in one difference
    (ec.h sub_k<K>) shows only there."""
    cv, ov = CURVES[cname]
    rnd = random.Random(11)
    out = C.create_string_buffer(2 * cv.fp_bytes)
    for _ in range(48):
        P, Q = ov.mul(ov.g1, rnd.randrange(1, cv.r)), ov.mul(ov.g1, rnd.randrange(1, cv.r))
        check(lib.apk_host_g1_op(cv.abi, 12, cv.g1_to_bytes(P), cv.g1_to_bytes(Q), out))
        assert cv.g1_from_bytes(out.raw) == ov.add(P, ov.mul(Q, 3))
        check(lib.apk_host_g1_op(cv.abi, 14, cv.g1_to_bytes(P), cv.g1_to_bytes(Q), out))
        assert cv.g1_from_bytes(out.raw) == ov.add(ov.mul(P, 4), ov.mul(Q, 6))


@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_ntt_top_growth_input_reaches_the_canon_limit(cname):
    """The NTT's adversarial input (used by the GPU test below) really takes the lazy butterflies where canon<32> is needed: the
    last output of a 2^17 forward transform ends between 32p and the stated (4 + 2 log2 N) p, while a plain all-(p - 1) input
    stays near (1 + log2 N) p.  Values only (limb_model.lazy_ntt), so this runs without a GPU."""
    _, ov = CURVES[cname]
    p, log_n = ov.r, 17
    a = lm.lazy_ntt(ov, log_n, lm.ntt_top_growth_input(ov, log_n))
    assert 32 * p <= a[-1] < (4 + 2 * log_n) * p < 64 * p
    assert max(a) == a[-1]
    plain = lm.lazy_ntt(ov, 12, [p - 1] * (1 << 12))
    assert max(plain) < 16 * p


def test_seams_reject_unknown_ops():
    cv, _ = CURVES["bn254"]
    rec = np.zeros((1, 4 * 9), dtype=np.uint32)
    out = np.zeros((1, 9), dtype=np.uint32)
    assert lib.apk_host_feu_op(cv.abi, 0, 30, 1, rec.ctypes.data, out.ctypes.data) == _lib.APK_ERR_ARG
    buf = C.create_string_buffer(64)
    assert lib.apk_device_fe_op(cv.abi, 0, 5, 0, 1, buf, buf, buf) == _lib.APK_ERR_ARG      # checked before any launch
    assert lib.apk_device_g1_op(cv.abi, 22, 0, 1, buf, buf, buf) == _lib.APK_ERR_ARG
    assert lib.apk_device_feu_op(7, 0, 0, 0, 1, rec.ctypes.data, out.ctypes.data) == _lib.APK_ERR_ARG


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cname,fld", FIELDS, ids=FIELD_IDS)
def test_unsaturated_ops_device_equal_host(gpu, cname, fld):
    """Every raw-limb op: the device (ffu_asm.h chains for mul / sqr) gives the host's bytes on the edge operands and on a
    random bulk of 2^16 per op, and its edge results satisfy the model."""
    f = _field(cname, fld)
    rng = np.random.default_rng(fld * 2 + (cname == "bls12-381"))
    for o in lm.OPS:
        xs = lm.operands(f, o, 0, seed=5)
        edge = lm.pack_records(f, o, xs)
        bulk = np.zeros((N_RANDOM_DEVICE, 4, f.L), dtype=np.uint32)
        per = N_RANDOM_DEVICE // len(o.classes(f)) + 1
        for ci, cls in enumerate(o.classes(f)):
            rows = slice(ci * per, min((ci + 1) * per, N_RANDOM_DEVICE))
            n = rows.stop - rows.start
            for i in range(o.arity):
                if o.io == "words_in" and i == 0:
                    w = rng.integers(0, 1 << 32, size=(n, f.N), dtype=np.uint64).astype(np.uint32)
                    if o.name == "from_fe":      # canonical input: the top word below p's
                        w[:, f.N - 1] %= np.uint32(f.p >> (32 * (f.N - 1)))
                    bulk[rows, i, : f.N] = w
                else:
                    bulk[rows, i, :] = lm.random_limbs(f, cls[i], n, rng)
        recs = np.concatenate([edge, bulk.reshape(N_RANDOM_DEVICE, 4 * f.L)])
        host = lm.run(f, o, recs)
        dev = lm.run(f, o, recs, device=gpu)
        diff = np.nonzero((host != dev).any(axis=1))[0]
        assert diff.size == 0, "%s %s: device != host on %d records, first: %s" % (f, o.name, diff.size, recs[diff[0]].tolist())
        bad = lm.violations(f, o, xs, dev[: len(xs)])
        assert not bad, "\n".join(bad)


def _fe_edges(mod, rnd):
    vals = [0, 1, 2, mod - 1, mod - 2, (mod - 1) // 2, (mod + 1) // 2, (1 << 32) - 1, 1 << 32] + [rnd.randrange(mod) for _ in range(6)]
    return [v % mod for v in vals]


@pytest.mark.gpu
@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_saturated_field_ops_device_at_edges(gpu, cname):
    """ff.h Fe ops 0-4 (the device's MacChain product) and 10-14 (the unsaturated forms, converted) on the device against big
    integers, on edge representations (p - 1 x p - 1 and so on, as gnark's Montgomery words), and device bytes == host bytes."""
    cv, _ = CURVES[cname]
    rnd = random.Random(7)
    for fld, mod, nb in ((0, cv.r, 32), (1, cv.p, cv.fp_bytes)):
        R = 1 << (8 * nb)
        rinv = pow(R, -1, mod)
        e = _fe_edges(mod, rnd)
        pairs = [(a, b) for a in e for b in e]          # raw Montgomery words: a stands for a / R
        A = b"".join(a.to_bytes(nb, "little") for a, _ in pairs)
        Bv = b"".join(b.to_bytes(nb, "little") for _, b in pairs)
        for op in (0, 1, 2, 3, 4, 10, 11, 12, 13, 14):
            dev, host = C.create_string_buffer(len(A)), C.create_string_buffer(nb)
            check(lib.apk_device_fe_op(cv.abi, fld, op, gpu, len(pairs), A, Bv, dev))
            for i, (a, b) in enumerate(pairs):
                got = int.from_bytes(dev.raw[i * nb:(i + 1) * nb], "little")
                check(lib.apk_host_fe_op(cv.abi, fld, op, A[i * nb:(i + 1) * nb], Bv[i * nb:(i + 1) * nb], host))
                assert dev.raw[i * nb:(i + 1) * nb] == host.raw, (cname, fld, op, a, b)
                x, y = a * rinv % mod, b * rinv % mod            # the values
                if op in (0, 11):
                    want = (x + y) % mod
                elif op in (1, 12):
                    want = (x - y) % mod
                elif op in (2, 10):
                    want = x * y % mod
                elif op == 3:
                    want = pow(x, -1, mod) if x else 0
                elif op in (4, 13):
                    want = -x % mod
                else:
                    u, v = x, y
                    for _ in range(10):
                        u, v = (u + y * v) % mod, (u - y * v) % mod
                    want = u
                assert got < mod and got * rinv % mod == want, (cname, fld, op, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_curve_ops_device_at_extreme_points(gpu, cname):
    """ec.h ops 0-3 and 10-14 on the device against the oracle (P + P, P + (-P), infinity, extreme coordinates), and the
    four-lane forms lane by lane: add_quad_general (20) and dbl_quad_general (21) on lazy-class operands."""
    cv, ov = CURVES[cname]
    g1b = 2 * cv.fp_bytes
    cases = [c for c in _g1_cases(cv, ov, random.Random(3)) if not (c[0] == 14 and c[2] is None)]
    for op in sorted({c[0] for c in cases}):
        sel = [c for c in cases if c[0] == op]
        P = b"".join(cv.g1_to_bytes(c[1]) for c in sel)
        Q = None if op == 2 else b"".join(_q_bytes(cv, op, c[2]) for c in sel)
        out = C.create_string_buffer(len(sel) * g1b)
        check(lib.apk_device_g1_op(cv.abi, op, gpu, len(sel), P, Q, out))
        for i, (_, a, q, want) in enumerate(sel):
            assert cv.g1_from_bytes(out.raw[i * g1b:(i + 1) * g1b]) == want, (cname, op, a, q)
    # the quad forms: generic pairs, extreme points, infinity (a copy), equal and opposite operands (reported as degenerate)
    rnd = random.Random(9)
    ext = _extreme_points(cv, ov)
    gen = [ov.mul(ov.g1, rnd.randrange(1, cv.r)) for _ in range(6)]
    pts = ext + gen
    pairs = [(P, Q) for P in pts for Q in pts if P != Q and P != ov.neg(Q)]
    special = [(P, P) for P in pts[:3]] + [(P, ov.neg(P)) for P in pts[:3]]
    inf = [(pts[0], None), (None, pts[1])]
    allp = pairs + special + inf
    out = C.create_string_buffer(4 * len(allp) * g1b)
    check(lib.apk_device_g1_op(cv.abi, 20, gpu, len(allp), b"".join(cv.g1_to_bytes(P) for P, _ in allp),
                               b"".join(cv.g1_to_bytes(Q) for _, Q in allp), out))
    for i, (P, Q) in enumerate(allp):
        for lane in range(4):
            raw = out.raw[(4 * i + lane) * g1b:(4 * i + lane + 1) * g1b]
            if (P, Q) in special:
                assert raw == b"\xff" * g1b, ("degenerate pair not reported", cname, lane, P, Q)
            else:
                assert cv.g1_from_bytes(raw) == ov.add(P, Q), (cname, "add_quad", lane, P, Q)
    dp = pts + [None]
    out = C.create_string_buffer(4 * len(dp) * g1b)
    check(lib.apk_device_g1_op(cv.abi, 21, gpu, len(dp), b"".join(cv.g1_to_bytes(P) for P in dp), None, out))
    for i, P in enumerate(dp):
        for lane in range(4):
            raw = out.raw[(4 * i + lane) * g1b:(4 * i + lane + 1) * g1b]
            assert cv.g1_from_bytes(raw) == ov.add(P, P), (cname, "dbl_quad", lane, P)


_NTT_SCRIPT = r"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from algoplonk_amd import setup, plonk
from algoplonk_amd._lib import lib, check
from oracle import c_oracle, plonk as oplonk
from oracle.prng import tau_from_seed
from helpers import CURVES, random_chain_ccs
import limb_model as lm
clib = c_oracle.load()
for cname in ("bn254", "bls12-381"):
    cv, ov = CURVES[cname]
    r = cv.r
    for log_n in (8, 10, 12):
        ccs, _, _ = random_chain_ccs(cv, log_n, 31)
        n = ccs.domain_size()
        srs = setup.unsafe_srs(cv, n, tau_from_seed(5, r), device=0)
        pk, _ = plonk.Setup(ccs, srs, device=0)
        for which, size in ((0, n), (1, 4 * n)):
            for name, vals in (("all p-1", [r - 1] * size), ("alternating 0, p-1", [0, r - 1] * (size // 2)),
                               ("p-1 impulse", [0] * (size - 1) + [r - 1]), ("p-1 at 0", [r - 1] + [0] * (size - 1))):
                for inverse, coset in ((0, 0), (1, 0)) + (((0, 1), (1, 1)) if which else ()):
                    data = cv.fr_vector(vals)
                    if size <= 1024 and not coset:
                        w = ov.omega(size)
                        want = cv.fr_vector((oplonk.intt if inverse else oplonk.ntt)(vals, w, r))
                    else:
                        a_buf = C.create_string_buffer(data, len(data))
                        assert clib.orc_ntt(cv.abi, a_buf, size, inverse, coset) == 0
                        want = a_buf.raw
                    b_buf = C.create_string_buffer(data, len(data))
                    check(lib.apk_ntt(pk.ctx, which, inverse, coset, b_buf))
                    if b_buf.raw != want:
                        print("MISMATCH", cname, size, name, "inverse" if inverse else "forward", "coset" if coset else "")
        pk.close()
    # 2^17 (4n, n = 2^15): inputs that drive the last output above 32p (limb_model.ntt_top_growth_input), forward and on the
    # coset (the same words divided by the coset powers, so the pre-multiplied data are the forward case's) and inverse
    ccs, _, _ = random_chain_ccs(cv, 15, 31)
    n = ccs.domain_size()
    srs = setup.unsafe_srs(cv, n, tau_from_seed(5, r), device=0)
    pk, _ = plonk.Setup(ccs, srs, device=0)
    size, log_size, u = 4 * n, (4 * n).bit_length() - 1, ov.coset_shift
    for inverse, coset in ((0, 0), (0, 1), (1, 0)):
        x = lm.ntt_top_growth_input(ov, log_size, bool(inverse))
        if coset:
            ui = pow(u, -1, r)
            x = [v * pow(ui, i, r) % r for i, v in enumerate(x)]
        data = b"".join(v.to_bytes(32, "little") for v in x)
        a_buf, b_buf = C.create_string_buffer(data, len(data)), C.create_string_buffer(data, len(data))
        assert clib.orc_ntt(cv.abi, a_buf, size, inverse, coset) == 0
        check(lib.apk_ntt(pk.ctx, 1, inverse, coset, b_buf))
        if b_buf.raw != a_buf.raw:
            print("MISMATCH", cname, size, "top-growth input", "inverse" if inverse else "forward", "coset" if coset else "")
    pk.close()
print("DONE")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("radix4", ["default", "radix4"])
def test_ntt_adversarial_inputs(gpu, radix4):
    """The lazy butterflies (kernels_ntt.h: values grow by up to 2p a stage, canon<32> at the end) on inputs that sit at the
    top of the class - all p - 1, alternating 0 and p - 1, a single p - 1 impulse - forward, inverse and on the coset, at 2^8 ..
    2^14 (two passes each: ntt_plan.h, tests/test_ntt_model.py lists the stages), and at 2^17 (three passes) an input whose last
    output reaches past 32p before the final canon<32>; in a process of its own with APK_NTT_RADIX4=1 (read once per process)."""
    env = dict(os.environ)
    if radix4 == "radix4":
        env["APK_NTT_RADIX4"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", _NTT_SCRIPT], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "DONE" in out.stdout and "MISMATCH" not in out.stdout, out.stdout[-3000:]

"""The polynomial-stage kernels (algoplonk_amd/csrc/kernels_poly.h) one stage at a time, outside a proof, through
apk_device_poly_op (include/apk.h), against the big-integer references of tests/poly_model.py.

CPU tier: the value-level models of the lazy kernels (GpTermsK, QuotientK, subcoset_merge_kernel, EvalPartialK, LincombK,
DerivePowersK) over the edge classes below - every intermediate below the bound its comment states, every comment's figure
following from its operands' figures, every precondition of a subtraction or reduction met, the model's result equal to the
plain reference - and the seam's argument checking, which answers before any device is touched.
GPU tier: the device output equals the plain reference, word for word (the kernels end in canon<1>: no tolerance).

Input classes (stored words): per-proof vectors l, r, o, z, zs, pi2 from {0, 1, r-1, r, r+1, 2r-2, 2r-1, random below 2r};
per-circuit tables and challenges from {0, 1, r-1, r-2, random}, every challenge at r-1 at once, and a vector of all 2r-1
against tables of all r-1.  Shapes are the smallest at which each launch path exists."""
from __future__ import annotations

import ctypes as C
import random

import pytest

from algoplonk_amd import _lib
from algoplonk_amd._lib import lib

import poly_model as pm
from helpers import CURVES

CURVE_NAMES = ["bn254", "bls12-381"]
BIG = pm.SCAN_BLOCK * pm.POLY_THREADS + 1      # 2048 * 256 + 1: the first size with more than POLY_THREADS blocks


def _cv(name):
    return CURVES[name][0]


def _F(name) -> pm.PolyField:
    return pm.PolyField(_cv(name).r)


def semi_class(r, rnd):      # per-proof vectors: semi-canonical words
    return [0, 1, r - 1, r, r + 1, 2 * r - 2, 2 * r - 1, rnd.randrange(2 * r)]


def canon_class(r, rnd):     # per-circuit tables and challenges: canonical words
    return [0, 1, r - 1, r - 2, rnd.randrange(r)]


def draw(cls, r, rnd, n):
    """n words: the class's edges in turn, every fourth word random"""
    top, edges = 2 * r if cls is semi_class else r, cls(r, rnd)[:-1]
    return [rnd.randrange(top) if i % 4 == 3 else edges[(i - i // 4) % len(edges)] for i in range(n)]


# ---- the seam ---------------------------------------------------------------------------------------------------------------------
def pack(words) -> bytes:
    return b"".join(w.to_bytes(32, "little") for w in words)


def unpack(buf: bytes):
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def poly_op(cv, op, vec=None, fr=None, iv=(), out=None, elem=32, out_elem=32, device=0):
    """one apk_device_poly_op call: vec {slot: words | bytes}, fr {slot: word}, iv [ints], out {slot: elements} ->
    (return code, {slot: words | bytes})"""
    a, keep = _lib.PolyArgs(), []
    for i, words in (vec or {}).items():
        raw = bytes(words) if isinstance(words, (bytes, bytearray)) else pack(words)
        buf = C.create_string_buffer(raw, max(len(raw), 1))
        keep.append(buf)
        a.vec[i], a.len[i] = C.addressof(buf), len(raw) // elem
    for i, w in (fr or {}).items():
        a.fr[i][:] = list(w.to_bytes(32, "little"))
    for i, v in enumerate(iv):
        a.iv[i] = v
    bufs = {}
    for i, count in (out or {}).items():
        bufs[i] = C.create_string_buffer(max(count * out_elem, 1))
        a.out[i], a.out_len[i] = C.addressof(bufs[i]), count
    rc = lib.apk_device_poly_op(cv.abi, op, device, C.byref(a))
    return rc, {i: (unpack(b.raw) if out_elem == 32 else b.raw[:out_elem * (out or {})[i]]) for i, b in bufs.items()}


def run(cv, op, **kw):
    rc, outs = poly_op(cv, op, **kw)
    _lib.check(rc)
    return outs


def same(got, want, what):
    assert len(got) == len(want), what
    if got != want:
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        raise AssertionError("%s: %d of %d words differ, first at %d: got %#x, want %#x" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


# ---- quotient inputs: the whole coset as words under QuotientArgs' names -------------------------------------------------------
def quotient_inputs(F, pattern, nb_commit, nb_inject, n4, seed):
    r, rnd = F.r, random.Random(seed)
    q = {"nb_commit": nb_commit, "nb_inject": nb_inject}
    tables = ("qk", "ql", "qr", "qm", "qo", "s1", "s2", "s3", "x", "l0")
    consts = ("alpha", "beta", "gamma", "beta_u", "beta_u2", "alpha2")
    if pattern == "extreme":       # all 2r-1 against tables of all r-1, every challenge at r-1 at once
        for k in ("l", "r", "o", "z"):
            q[k] = [2 * r - 1] * n4
        for k in tables:
            q[k] = [r - 1] * n4
        q["pi2"] = [[2 * r - 1] * n4 for _ in range(nb_commit)]
        q["qcp"] = [[r - 1] * n4 for _ in range(nb_commit)]
        q["inj_tab"] = [[r - 1] * n4 for _ in range(nb_inject)]
        q["inj_delta"] = [r - 1] * nb_inject
        for k in consts:
            q[k] = r - 1
        q["zh_inv"] = [r - 1] * 4
    else:                          # the classes' edges against each other, a quarter random
        for k in ("l", "r", "o", "z"):
            q[k] = draw(semi_class, r, rnd, n4)
            rnd.shuffle(q[k])
        for k in tables:
            q[k] = draw(canon_class, r, rnd, n4)
            rnd.shuffle(q[k])
        q["pi2"] = [draw(semi_class, r, rnd, n4) for _ in range(nb_commit)]
        q["qcp"] = [draw(canon_class, r, rnd, n4) for _ in range(nb_commit)]
        q["inj_tab"] = [draw(canon_class, r, rnd, n4) for _ in range(nb_inject)]
        q["inj_delta"] = [canon_class(r, rnd)[(j + 2) % 5] for j in range(nb_inject)]
        for j, k in enumerate(consts):
            q[k] = canon_class(r, rnd)[(j + 2) % 5] if pattern == "edges" else rnd.randrange(r)
        q["zh_inv"] = [r - 1, r - 2, 1, rnd.randrange(r)]
    return q


def quotient_point(q, i):
    """the words point i of the whole coset sees"""
    n4 = len(q["l"])
    p = {k: q[k][i] for k in ("l", "r", "o", "z", "qk", "ql", "qr", "qm", "qo", "s1", "s2", "s3", "x", "l0")}
    p["zs"] = q["z"][(i + 4) % n4]
    p.update({k: q[k] for k in ("alpha", "beta", "gamma", "beta_u", "beta_u2", "alpha2", "inj_delta")})
    p["zh_inv"] = q["zh_inv"][i & 3]
    for k in ("qcp", "pi2", "inj_tab"):
        p[k] = [v[i] for v in q[k]]
    return p


def quotient_call(cv, q, glog, k):
    """class k of 2^glog: the per-proof vectors hold the points k + G j at index j, the tables the whole coset"""
    G, n4 = 1 << glog, len(q["l"])
    cls = lambda v, kk=k: v[kk::G]
    vec = {0: cls(q["l"]), 1: cls(q["r"]), 2: cls(q["o"]), 3: cls(q["z"])}
    if glog == 3:
        vec[4] = cls(q["z"], (k + 4) % 8)        # Z(omega X) lives in class (k + 4) mod 8
    for c in range(q["nb_commit"]):
        vec[5 + c], vec[17 + c] = cls(q["pi2"][c]), q["qcp"][c]
    for j, name in enumerate(("qk", "ql", "qr", "qm", "qo", "s1", "s2", "s3", "x", "l0")):
        vec[7 + j] = q[name]
    for j in range(q["nb_inject"]):
        vec[19 + j] = q["inj_tab"][j]
    fr = {j: q[name] for j, name in enumerate(("alpha", "beta", "gamma", "beta_u", "beta_u2", "alpha2"))}
    fr.update({6 + j: w for j, w in enumerate(q["zh_inv"])})
    fr.update({10 + j: w for j, w in enumerate(q["inj_delta"])})
    return run(cv, _lib.POLY_QUOTIENT, vec=vec, fr=fr, iv=[n4 >> glog, q["nb_commit"], q["nb_inject"], k, glog], out={0: n4 >> glog})[0]


# =====================================================================================================================
# CPU tier
# =====================================================================================================================
def _clean(trace, what=""):
    assert not trace.bad, "%s%s" % (what, "\n".join(trace.bad[:5]))


@pytest.mark.parametrize("cname", CURVE_NAMES)
@pytest.mark.parametrize("pattern", ["extreme", "edges", "random"])
def test_quotient_model_stays_inside_the_stated_bounds(cname, pattern):
    """QuotientK's chain of comments with the full complement (2 commitments, 6 injections): classes, figures, values,
    preconditions; the model's result is the plain reference's; the largest gate / num / res seen are printed."""
    F = _F(cname)
    q = quotient_inputs(F, pattern, 2, 6, 256, 0x51A0 + len(pattern))
    want = pm.ref_quotient(F, q)
    peak = {"gate": 0.0, "num": 0.0, "res": 0.0}
    for i in range(256):
        got, t = pm.lazy_quotient(F, quotient_point(q, i))
        _clean(t, "point %d: " % i)
        assert got == want[i], "point %d: the value-level model and the plain reference disagree" % i
        for k in peak:
            peak[k] = max(peak[k], t.named[k][0] / F.r)
    print("%s %s: gate <= %.3f r (stated 14.4), num <= %.3f r (stated 17), res <= %.4f r (limit 2)" % (cname, pattern, peak["gate"], peak["num"], peak["res"]))
    assert peak["gate"] < 14.4 and peak["num"] < 17 and peak["res"] < 2


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_quotient_model_names_the_line_of_a_wide_operand(cname):
    """an operand one class wider than the comment says is refused, with the kernel's line: a table at r (the comment takes
    tables below r), a per-proof word at 2 r"""
    F = _F(cname)
    q = quotient_inputs(F, "random", 2, 6, 8, 1)
    p = quotient_point(q, 3)
    _clean(pm.lazy_quotient(F, p)[1])
    for name, word, line in (("ql", F.r, "ld(a.ql, i), l)"), ("l", 2 * F.r, "ld(a.l, jj)"), ("s2", F.r + 5, "U pa = "), ("alpha", F.r, "const U perm")):
        t = pm.lazy_quotient(F, dict(p, **{name: word}))[1]
        assert t.bad and any(line in b and name in b for b in t.bad), (name, t.bad)
    # and a comment whose figure does not follow from its operands: a semi-canonical TABLE makes "1 x 2: < 1.04" a 2 x 2 product
    t = pm.Trace(F, "QuotientK")
    x = t.stated("ql*l", t.mul_nr(pm.LV(F.r - 1, pm.Fraction(2)), pm.LV(F.r - 1, pm.Fraction(2)), "g1"), "1.04", "g1")
    assert x and any("the comment states 1.0400 r" in b for b in t.bad)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_gp_terms_model(cname):
    """GpTermsK: sums below 4 r, products below 2 r, canon<1> below 2 r; result = the reference's row terms (exact / 1024)"""
    F, rnd = _F(cname), random.Random(7)
    r = F.r
    rows = [[r - 1] * 11] + [[canon_class(r, rnd)[(i + j) % 5] for j in range(11)] for i in range(10)] + [[rnd.randrange(r) for _ in range(11)] for _ in range(40)]
    for row in rows:
        L, R, O, S1, S2, S3, w, b, gm, bu, bu2 = row
        nu, de, t = pm.lazy_gp_terms(F, L, R, O, S1, S2, S3, w, b, gm, bu, bu2)
        _clean(t)
        # (a one-row "domain": tw = [w], row 0)
        num, den, _ = pm.ref_gp(F, [L], [R], [O], [S1], [S2], [S3], [w], b, gm, bu, bu2) if de else (None, None, None)
        if de:
            assert [nu] == num and [de] == den
    t = pm.lazy_gp_terms(F, r, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)[2]      # a wire at r: `// < 2` no longer follows
    assert any("L enters at" in b for b in t.bad)


@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_sum_kernels_models(cname):
    """subcoset_merge_kernel (8 products), EvalPartialK (8 products, reduce_2p<8>), LincombK (LC_MAX products, reduce_2p<32>),
    DerivePowersK: all operands at r-1, edges, random; the result is the reference's"""
    F, rnd = _F(cname), random.Random(11)
    r = F.r
    for words in ([r - 1] * 64, [canon_class(r, rnd)[i % 5] for i in range(64)], [rnd.randrange(r) for _ in range(64)]):
        for G in (2, 4, 8):
            out, t = pm.lazy_merge(F, words[:G], words[8:16], words[16:16 + G], G)
            _clean(t)
            assert out == pm.ref_merge(F, words[:G], words[16:16 + G], words[8:16], 1, G)
        got, t = pm.lazy_eval_lane(F, words[:8], words[8:16])
        _clean(t)
        assert got == pm.ref_eval(F, words[:8], words[8:16])
        got, t = pm.lazy_lincomb(F, words[:pm.LC_MAX], words[20:20 + pm.LC_MAX])
        _clean(t)
        assert [got] == pm.ref_lincomb(F, [[w] for w in words[20:20 + pm.LC_MAX]], words[:pm.LC_MAX], 1)
        got, t = pm.lazy_derive(F, words[0], words[1])
        _clean(t)
        assert [got] == pm.ref_derive(F, [words[1]], [words[0], 0], 4, 0)
    # one term more than LC_MAX would still fit 64 r - but 33 would not, and the model says so
    t = pm.Trace(F, "LincombK")
    acc = pm.LV(0, pm.Fraction(0))
    for _ in range(33):
        acc = t.add_n(acc, pm.LV(r, pm.Fraction(2)))
    t.reduce_2p(32, acc, "reduce_2p<32>(acc)")
    assert t.bad


def test_seam_refuses_bad_arguments_before_any_device():
    """unknown op, counts above EVAL_MAX / LC_MAX / QK_INJECT_MAX, sub_glog > 3, zero lengths, a stray vector: APK_ERR_ARG with
    a message, whether or not a GPU is there (device 99 is never opened)"""
    assert hasattr(lib, "apk_device_poly_op") and "apk_device_poly_op" in _lib.SYMBOLS
    cv = _cv("bn254")
    one = [1]
    bad = [
        (99, {}), (-1, {}),
        (_lib.POLY_EVAL, dict(vec={i: one for i in range(13)}, iv=[13], out={0: 13})),
        (_lib.POLY_EVAL, dict(vec={0: one}, iv=[1], out={0: 1})),                                  # no table of powers
        (_lib.POLY_EVAL, dict(vec={0: [1, 1], 24: one}, iv=[1], out={0: 1})),                      # ... or a short one
        (_lib.POLY_LINCOMB, dict(vec={i: one for i in range(21)}, iv=[21, 1], out={0: 1})),
        (_lib.POLY_LINCOMB, dict(vec={0: one}, iv=[1, 0], out={0: 0})),
        (_lib.POLY_LINCOMB, dict(vec={0: []}, iv=[1, 1], out={0: 1})),
        (_lib.POLY_SCAN, dict(vec={0: []}, iv=[0, 0, 0], out={0: 0})),
        (_lib.POLY_SCAN, dict(vec={0: one}, iv=[0, 1, 1], out={0: 1})),                            # shift with rev
        (_lib.POLY_SCAN, dict(vec={0: one, 5: one}, iv=[0, 0, 0], out={0: 1})),                    # a vector outside the layout
        (_lib.POLY_SCAN, dict(vec={0: one}, iv=[0, 0, 0], out={0: 2})),
        (_lib.POLY_MERGE, dict(vec={0: one * 16, 1: one * 16}, iv=[1, 4], out={0: 16})),
        (_lib.POLY_DERIVE_POWERS, dict(vec={0: one, 1: one, 2: one}, iv=[3, 1, 0, 0], out={0: 1, 1: 1})),
        (_lib.POLY_KZG_QUOTIENT, dict(vec={0: one, 1: one, 2: one}, iv=[1, 0], out={0: 0})),
        (_lib.POLY_BLIND, dict(vec={0: one * 8}, iv=[4, 4], out={0: 8})),
        (_lib.POLY_TAIL, dict(vec={0: b""}, iv=[1, 0], out={0: 1}, elem=16, out_elem=4)),
        (_lib.POLY_GRAND_PRODUCT, dict(vec={i: one * 6 for i in range(6)}, iv=[6], out={0: 6, 1: 6, 2: 6})),
    ]
    q = quotient_inputs(_F("bn254"), "random", 2, 6, 8, 3)
    base = dict(vec={**{i: q["l"] for i in range(4)}, 5: q["l"], 6: q["l"], **{i: q["ql"] for i in range(7, 25)}}, out={0: 8})
    bad += [(_lib.POLY_QUOTIENT, dict(base, iv=iv)) for iv in ([8, 2, 7, 0, 0], [8, 3, 6, 0, 0], [8, 2, 6, 0, 4], [8, 2, 6, 1, 0], [2, 2, 6, 0, 0], [8, 2, 5, 0, 0])]
    for op, kw in bad:
        rc, _ = poly_op(cv, op, device=99, **kw)
        assert rc == _lib.APK_ERR_ARG and b"polynomial-stage op" in lib.apk_last_error(), (op, kw.get("iv"))
    rc, _ = poly_op(cv, _lib.POLY_QUOTIENT, device=99, **dict(base, iv=[8, 2, 6, 0, 0]))     # the same block, in order: past the checks,
    assert rc != _lib.APK_OK and b"polynomial-stage op" not in lib.apk_last_error()          # refused for the device alone
    assert lib.apk_device_poly_op(7, 0, 0, C.byref(_lib.PolyArgs())) == _lib.APK_ERR_ARG and lib.apk_device_poly_op(0, 0, 0, None) == _lib.APK_ERR_ARG
    assert _lib.ABI_VERSION == 5 and lib.apk_abi_version() == 5          # additive


# =====================================================================================================================
# GPU tier
# =====================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
@pytest.mark.parametrize("shape", [(0, 0), (2, 1), (0, 6), (2, 6)], ids=lambda s: "commit%d-inject%d" % s)
@pytest.mark.parametrize("pattern", ["extreme", "edges", "random"])
def test_gpu_quotient_whole_and_in_every_subcoset_class(gpu, cname, shape, pattern):
    """n4 = 512 arbitrary words (the kernel is pointwise), Z(omega X) at point i = z[(i + 4) mod n4].  The whole coset equals the
    reference; so does the union of the classes for G = 2, 4, 8 with every sub_k (m = 256, 128, 64): the wrap at is >= n4 in every
    class, the G = 8 j / j+1 rule, zh_inv[i & 3]."""
    cv, F = _cv(cname), _F(cname)
    q = quotient_inputs(F, pattern, shape[0], shape[1], 512, 0xC05E7 + 16 * shape[0] + shape[1])
    want = pm.ref_quotient(F, q)
    same(quotient_call(cv, q, 0, 0), want, "whole coset")
    for glog in (1, 2, 3):
        G, got = 1 << glog, [None] * 512
        for k in range(G):
            got[k::G] = quotient_call(cv, q, glog, k)
        same(got, want, "the union of %d classes" % G)


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
@pytest.mark.parametrize("n", [2048, 4096])
@pytest.mark.parametrize("pattern", ["edges", "random"])
def test_gpu_grand_product(gpu, cname, n, pattern):
    """n = 2048 (one scan block) and 4096, the domain points from the size-n twiddle table.  Z equals the reference product, the
    rows' num and den equal exact / 1024.  Rows whose denominator is zero are excluded (the prover's formula inverts the product
    of all denominators; gnark's own Z is undefined there too): such a row's L is drawn again."""
    cv, F = _cv(cname), _F(cname)
    r, g, rnd = F.r, F.gnark, random.Random(n + len(pattern))
    cols = [draw(canon_class, r, rnd, n) if pattern == "edges" else [rnd.randrange(r) for _ in range(n)] for _ in range(6)]
    om = cv.omega(n)
    tw, x = [], 1
    for _ in range(n // 2):
        tw.append(g.enc(x))
        x = x * om % r
    ch = [r - 1, r - 1, r - 1, r - 1] if pattern == "edges" else [rnd.randrange(r) for _ in range(4)]   # 32 beta, gamma, 32 beta u, 32 beta u^2
    for _ in range(4):
        _, den, _ = pm.ref_gp(F, *cols, tw, *ch)
        zero = [i for i, d in enumerate(den) if d == 0]
        if not zero:
            break
        for i in zero:
            cols[0][i] = rnd.randrange(r)
    assert not zero
    num, den, z = pm.ref_gp(F, *cols, tw, *ch)
    out = run(cv, _lib.POLY_GRAND_PRODUCT, vec={**{i: c for i, c in enumerate(cols)}, 6: tw}, fr=dict(enumerate(ch)), iv=[n], out={0: n, 1: n, 2: n})
    same(out[0], num, "num")
    same(out[1], den, "den")
    same(out[2], z, "Z")


def _scan_data(F, mul, count, rnd):
    r = F.r
    if not mul:
        return [r - 1] * count
    data = [rnd.randrange(1, r) for _ in range(count)]
    one = F.gnark.enc(1)
    lo = count // 3
    data[lo:lo + min(300, count // 4)] = [one] * len(data[lo:lo + min(300, count // 4)])      # a block of ones
    if count > 2:
        data[(2 * count) // 3] = 0                                                               # a single zero
    return data


SCAN_CASES = [(c, rev, shift) for c in (1, 2047, 2048, 2049, 4099) for rev, shift in ((0, 0), (1, 0), (0, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
@pytest.mark.parametrize("mul", [1, 0], ids=["mul", "add"])
def test_gpu_scan(gpu, cname, mul):
    """counts 1, 2047, 2048, 2049, 4099; forward / reverse, shift 0 / 1 (forward).  multiply: random with a block of ones and a
    single zero; add: all r-1."""
    cv, F = _cv(cname), _F(cname)
    rnd = random.Random(5)
    for count, rev, shift in SCAN_CASES:
        data = _scan_data(F, mul, count, rnd)
        got = run(cv, _lib.POLY_SCAN, vec={0: data}, iv=[0 if mul else 1, rev, shift], out={0: count})[0]
        same(got, pm.ref_scan(F, data, bool(mul), bool(rev), shift), "count %d rev %d shift %d" % (count, rev, shift))


@pytest.mark.gpu
@pytest.mark.parametrize("mul", [1, 0], ids=["mul", "add"])
def test_gpu_scan_more_blocks_than_threads(gpu, mul):
    """2048 * 256 + 1 elements: 257 blocks, the first size where a lane of scan_totals_body takes more than one block total"""
    cv, F = _cv("bls12-381"), _F("bls12-381")
    data = _scan_data(F, mul, BIG, random.Random(9))
    got = run(cv, _lib.POLY_SCAN, vec={0: data}, iv=[0 if mul else 1, 1 - mul, 0], out={0: BIG})[0]
    same(got, pm.ref_scan(F, data, bool(mul), not mul, 0), "count %d" % BIG)


def _powers(F, z, n):
    out, x = [], 1
    for _ in range(n):
        out.append(F.gnark.enc(x))
        x = x * z % F.r
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_gpu_eval_twelve_polynomials_of_unequal_length(gpu, cname):
    """EVAL_MAX polynomials of lengths 1 .. 4099 in one launch, shared and own tables of powers mixed, values r-1, edges, random"""
    cv, F = _cv(cname), _F(cname)
    r, rnd = F.r, random.Random(12)
    lens = [1, 255, 2048, 2049, 4099, 256, 257, 2047, 4096, 4097, 3, 1]
    shared = _powers(F, rnd.randrange(r), 4099)
    shared[7] = r - 1
    vec, want = {24: shared}, []
    for i, n in enumerate(lens):
        f = [r - 1] * n if i % 3 == 0 else draw(canon_class, r, rnd, n) if i % 3 == 1 else [rnd.randrange(r) for _ in range(n)]
        vec[i] = f
        own = None
        if i % 2:
            own = [r - 1] * n if i % 3 == 0 else _powers(F, r - 1 if i == 1 else rnd.randrange(r), n)
            vec[12 + i] = own
        want.append(pm.ref_eval(F, f, own or shared))
    same(run(cv, _lib.POLY_EVAL, vec=vec, iv=[12], out={0: 12})[0], want, "evaluations / 32")


@pytest.mark.gpu
def test_gpu_eval_more_partials_than_threads(gpu):
    """one polynomial of 2048 * 256 + 1 coefficients beside a short one: 257 partials, EvalFinalK's strided loop"""
    cv, F = _cv("bn254"), _F("bn254")
    r, rnd = F.r, random.Random(13)
    f = [rnd.randrange(r) for _ in range(BIG)]
    f[-1] = f[0] = r - 1
    pw = _powers(F, rnd.randrange(r), BIG)
    got = run(cv, _lib.POLY_EVAL, vec={0: f, 1: f[:5], 24: pw}, iv=[2], out={0: 2})[0]
    same(got, [pm.ref_eval(F, f, pw), pm.ref_eval(F, f[:5], pw)], "evaluations / 32")


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_gpu_lincomb(gpu, cname):
    """LC_MAX terms with lengths on both sides of out_len: coefficient words r-1 against value words r-1; coefficients 32 (r-1)
    and edges against edges and random; one term"""
    cv, F = _cv(cname), _F(cname)
    r, rnd = F.r, random.Random(14)
    out_len = 300
    lens = [1, 255, 256, 257, 299, 300, 301, 600, 2, 300, 150, 300, 298, 512, 300, 7, 300, 64, 300, 300]
    for pattern in ("extreme", "mixed"):
        if pattern == "extreme":
            fs, coef = [[r - 1] * n for n in lens], [r - 1] * 20
        else:
            fs = [draw(canon_class, r, rnd, n) if i % 2 else [rnd.randrange(r) for _ in range(n)] for i, n in enumerate(lens)]
            coef = [F.prod.enc(r - 1) if i % 3 == 0 else canon_class(r, rnd)[i % 5] for i in range(20)]
        got = run(cv, _lib.POLY_LINCOMB, vec=dict(enumerate(fs)), fr=dict(enumerate(coef)), iv=[20, out_len], out={0: out_len})[0]
        same(got, pm.ref_lincomb(F, fs, coef, out_len), "20 terms, " + pattern)
    for n in (299, 301):
        f = [r - 1] * n
        got = run(cv, _lib.POLY_LINCOMB, vec={0: f}, fr={0: F.prod.enc(r - 1)}, iv=[1, out_len], out={0: out_len})[0]
        same(got, pm.ref_lincomb(F, [f], [F.prod.enc(r - 1)], out_len), "one term of %d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
@pytest.mark.parametrize("G", [2, 4, 8])
def test_gpu_subcoset_merge(gpu, cname, G):
    """m = 64: parts all r-1 and random, rho a primitive G-th root of unity"""
    cv, F = _cv(cname), _F(cname)
    r, rnd, m = F.r, random.Random(15 + G), 64
    rho_inv = pow(cv.omega(G), -1, r)
    rho = [F.prod.enc(pow(rho_inv, e, r)) for e in range(8)]
    for pattern in ("extreme", "random"):
        part = [r - 1] * (G * m) if pattern == "extreme" else [rnd.randrange(r) for _ in range(G * m)]
        post = [r - 1] * (G * m) if pattern == "extreme" else draw(canon_class, r, rnd, G * m)
        got = run(cv, _lib.POLY_MERGE, vec={0: part, 1: post}, fr=dict(enumerate(rho)), iv=[m, G.bit_length() - 1], out={0: G * m})[0]
        same(got, pm.ref_merge(F, part, post, rho, m, G), pattern)


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
@pytest.mark.parametrize("n", [8, 2048])
def test_gpu_derive_powers(gpu, cname, n):
    """count n + 3, both directions in one launch: the exponents 0, n/2, n-1 and the wrap past n"""
    cv, F = _cv(cname), _F(cname)
    r, rnd = F.r, random.Random(16)
    om = cv.omega(n)
    twu = [F.prod.enc(pow(om, j, r)) for j in range(n // 2)]
    a = _powers(F, rnd.randrange(r), n + 3)
    b = [r - 1] * (n + 3)
    b[1::3] = [rnd.randrange(r) for _ in b[1::3]]
    for inv in ((0, 1), (1, 0)):
        out = run(cv, _lib.POLY_DERIVE_POWERS, vec={0: a, 1: b, 2: twu}, iv=[n, n + 3, inv[0], inv[1]], out={0: n + 3, 1: n + 3})
        same(out[0], pm.ref_derive(F, a, twu, n, inv[0]), "first, inverse %d" % inv[0])
        same(out[1], pm.ref_derive(F, b, twu, n, inv[1]), "second, inverse %d" % inv[1])


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_gpu_kzg_quotient(gpu, cname):
    """(f - f(z)) / (X - z) for 2, 2049 and 4099 coefficients, z in {0, 1, r-1, random}"""
    cv, F = _cv(cname), _F(cname)
    r, rnd = F.r, random.Random(17)
    for n in (2, 2049, 4099):
        f = [rnd.randrange(r) for _ in range(n)]
        f[::5] = [r - 1] * len(f[::5])
        for z in (0, 1, r - 1, rnd.randrange(2, r)):
            vec = {0: f}
            if z:
                vec.update({1: _powers(F, z, n), 2: _powers(F, pow(z, -1, r), n)})
            got = run(cv, _lib.POLY_KZG_QUOTIENT, vec=vec, iv=[n, int(z == 0)], out={0: n - 1})[0]
            same(got, pm.ref_kzg_quotient(F, f, z), "len %d z %s" % (n, {0: "0", 1: "1", r - 1: "r-1"}.get(z, "random")))


@pytest.mark.gpu
@pytest.mark.parametrize("cname", CURVE_NAMES)
def test_gpu_blind(gpu, cname):
    """BlindK for d = 1, 2, 3; Blind3K with p and lag each null and non-null"""
    cv, F = _cv(cname), _F(cname)
    r, rnd, n = F.r, random.Random(18), 64
    for d in (1, 2, 3):
        p = [rnd.randrange(r) for _ in range(n)] + [0xBAD] * d
        p[0], p[1] = 0, r - 1
        b = [r - 1, 1, rnd.randrange(r)]
        got = run(cv, _lib.POLY_BLIND, vec={0: p}, fr=dict(enumerate(b)), iv=[n, d], out={0: n + d})[0]
        same(got, pm.ref_blind(F, p, n, b, d), "d = %d" % d)
        ps = [[rnd.randrange(r) for _ in range(n)] + [0xBAD] * d for _ in range(6)]
        bs = [[rnd.randrange(r), r - 1, 1][j:] + [0, 0, 0, 0] for j in range(3)]
        for have_p, have_lag in (((1, 1, 1), (1, 1, 1)), ((1, 0, 1), (0, 1, 0)), ((0, 0, 0), (1, 1, 1)), ((1, 1, 1), (0, 0, 0))):
            vec = {j: ps[j] for j in range(3) if have_p[j]}
            vec.update({3 + j: ps[3 + j] for j in range(3) if have_lag[j]})
            out = run(cv, _lib.POLY_BLIND3, vec=vec, fr={4 * j + i: bs[j][i] for j in range(3) for i in range(4)}, iv=[n, d], out={i: n + d for i in vec})
            for j in range(3):
                if have_p[j]:
                    same(out[j], pm.ref_blind(F, ps[j], n, bs[j], d), "wire %d" % j)
                if have_lag[j]:      # the scalars appended behind the n values, nothing else touched
                    same(out[3 + j], ps[3 + j][:n] + bs[j][:d], "lag %d" % j)


@pytest.mark.gpu
def test_gpu_tail_nonzero(gpu):
    """all zero: the flag is untouched; one non-zero word first, last, in the middle: the epoch; count4 no multiple of the grid
    (5000 records on 3 blocks; 2^20 + 2049 on the 512-block cap)"""
    cv = _cv("bn254")
    for count4 in (1, 5000, 512 * 2048 + 2049):
        spots = {None, 0, 16 * count4 - 4, (16 * count4 // 2) & ~3, 16 * (count4 - 1)}
        for spot in sorted(spots, key=lambda s: -1 if s is None else s):
            raw = bytearray(16 * count4)
            if spot is not None:
                raw[spot] = 0x80
            out = run(cv, _lib.POLY_TAIL, vec={0: raw}, iv=[7, 0xDEAD], out={0: 1}, elem=16, out_elem=4)[0]
            assert int.from_bytes(out, "little") == (0xDEAD if spot is None else 7), (count4, spot)

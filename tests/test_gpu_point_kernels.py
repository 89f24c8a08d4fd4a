"""-m gpu: the device code that handles group elements WITHOUT going through the MSM, held to big integers at its encoding and
group edges - g1_decompress_kernel and the lagrange_* kernels (kernels_setup.h), g1_mul_batch_kernel (kernels_msm.h),
lincomb_partial_kernel / lincomb_reduce_kernel / g1_check_kernel (kernels_lincomb.h) - through the C-ABI as it is
(apk_g1_decompress, apk_g1_to_lagrange, apk_g1_mul_batch, apk_g1_lincomb_segments, apk_verify_batch).

The references are tests/point_model.py (gnark's SetBytes rules, ToLagrangeG1 in the exponent), oracle/curves.py and
verify_batch_material.lincomb_reference; every comparison is exact.  Sizes are the smallest that reach the path: 255 / 256 / 257
around the 256-lane workgroups, 256 / 512 butterflies around the 128-lane one, 63 / 64 / 65 around LINCOMB_TREE."""
import ctypes as C
import functools

import pytest

from algoplonk_amd import _lib, setup as ap_setup
from algoplonk_amd._lib import lib, check
from oracle.prng import SplitMix64

import point_model as pm
import verify_batch_material as vbm
from helpers import CURVES

pytestmark = pytest.mark.gpu
OK, BAD, ARG = _lib.APK_OK, _lib.APK_ERR_VERIFY, _lib.APK_ERR_ARG
BOTH = ["bn254", "bls12-381"]


@functools.lru_cache(maxsize=None)
def _points(cname, count, seed=0x6E0):
    """`count` random points of G1 with the multiples of the generator they are: ([k_i], [k_i G]); computed once per curve"""
    cv, ov = CURVES[cname]
    g = SplitMix64(seed)
    ks = [g.fr(cv.r) or 1 for _ in range(count)]
    return ks, [ov.mul(ov.g1, k) for k in ks]


@functools.lru_cache(maxsize=None)
def _non_residue_x(cname):
    """an x below p with x^3 + b not a square: on no curve point"""
    _, ov = CURVES[cname]
    x = 5
    while pow((x ** 3 + ov.b) % ov.p, (ov.p - 1) // 2, ov.p) == 1:
        x += 1
    return x


def _decompress(cv, gpu, blob):
    """apk_g1_decompress -> (return code, points or None)"""
    count = len(blob) // cv.fp_bytes
    out = C.create_string_buffer(count * 2 * cv.fp_bytes)
    rc = lib.apk_g1_decompress(cv.abi, gpu, blob, count, out)
    return rc, (cv.g1_vector_decode(out.raw) if rc == OK else None)


# ---- 1. decompress: encodings ---------------------------------------------------------------------------------------------------
def _encoding_entries(cname):
    cv, ov = CURVES[cname]
    small = 0b100 if cname == "bls12-381" else 0b10
    infinity = 0b110 if cname == "bls12-381" else 0b01
    mask = pm.payload_mask(ov)
    e = [("x=0", pm.encode(ov, small, 0)), ("x=1", pm.encode(ov, small, 1)), ("x=p-1", pm.encode(ov, small, cv.p - 1)),
         ("x=p", pm.encode(ov, small, cv.p)), ("x=p+1", pm.encode(ov, small, cv.p + 1)), ("x=mask", pm.encode(ov, small, mask))]
    xv = _points(cname, 24)[1][20][0]
    for f in pm.flag_patterns(ov):
        e.append(("flags %s over a valid x" % bin(f), pm.encode(ov, f, xv)))
        e.append(("flags %s over zero" % bin(f), pm.encode(ov, f, 0)))
    e.append(("infinity, lowest payload bit", pm.encode(ov, infinity, 1)))
    e.append(("infinity, highest payload bit", pm.encode(ov, infinity, (mask + 1) >> 1)))
    below, above = pm.near_boundary(ov)
    for name, P in (("y just below the boundary", below), ("y just above the boundary", above)):
        e.append((name, ov.compress(P)))
        e.append((name + ", wrong sign", pm.wrong_sign(ov, P)))
    return e


@pytest.mark.parametrize("cname", BOTH)
def test_decompress_accepts_exactly_what_the_model_accepts(gpu, cname):
    """One entry per edge of SetBytes, each decoded beside a good point (the call gives one verdict): x at 0, 1, p-1, p, p+1 and
    the largest the mask leaves; every flag pattern over a valid x and over zero; the infinity flag with a payload bit at either
    end; the curve points whose y is closest to (p-1)/2 from either side, under both flags."""
    cv, ov = CURVES[cname]
    good_pt = ov.mul(ov.g1, 12345)
    good = ov.compress(good_pt)
    verdicts = set()
    for name, enc in _encoding_entries(cname):
        want = pm.accepts(ov, enc)
        rc, got = _decompress(cv, gpu, good + enc)
        verdicts.add(want is pm.REJECT)
        if want is pm.REJECT:
            assert rc == ARG, (name, enc.hex(), got)
            assert b"1 compressed point(s)" in lib.apk_last_error(), name
        else:
            assert rc == OK and got == [good_pt, want], (name, enc.hex(), lib.apk_last_error())
    assert verdicts == {True, False}


@pytest.mark.parametrize("cname", BOTH)
def test_decompress_wrong_sign_flag_gives_the_negated_point(gpu, cname):
    cv, ov = CURVES[cname]
    pts = _points(cname, 24)[1][:20]
    blob = b"".join(pm.wrong_sign(ov, P) for P in pts)
    assert [pm.accepts(ov, blob[i * cv.fp_bytes:(i + 1) * cv.fp_bytes]) for i in range(20)] == [ov.neg(P) for P in pts]
    rc, got = _decompress(cv, gpu, blob)
    assert rc == OK and got == [ov.neg(P) for P in pts], lib.apk_last_error()


@pytest.mark.parametrize("cname", BOTH)
def test_decompress_at_the_sign_boundary(gpu, cname):
    """y = (p-1)/2 is the largest "smallest" y, (p+1)/2 the smallest "largest": the point with that y under both flags."""
    cv, ov = CURVES[cname]
    bp = pm.boundary_point(ov)
    if bp is None:
        pytest.skip("%s has no point with y = (p-1)/2: ((p-1)/2)^2 - %d is not a cube mod p (point_model.boundary_point); the "
                    "nearest points on either side are in test_decompress_accepts_exactly_what_the_model_accepts" % (cname, ov.b))
    good = ov.compress(ov.g1)
    for P in bp:
        for enc in (ov.compress(P), pm.wrong_sign(ov, P)):
            want = pm.accepts(ov, enc)
            rc, got = _decompress(cv, gpu, good + enc)
            assert (rc, got) == ((ARG, None) if want is pm.REJECT else (OK, [ov.g1, want])), enc.hex()


# ---- 2. decompress: launch shape ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", BOTH)
def test_decompress_across_workgroups_and_the_error_count(gpu, cname):
    """255 / 256 / 257 / 513 points with infinity first and last: the whole vector.  Then one non-residue x at index 0, 255, 256,
    512 of 513 in turn, and three at once: APK_ERR_ARG and the count in the message."""
    cv, ov = CURVES[cname]
    rnd = _points(cname, 513)[1]
    nb = cv.fp_bytes
    for count in (255, 256, 257, 513):
        pts = [None] + rnd[1:count - 1] + [None]
        rc, got = _decompress(cv, gpu, b"".join(ov.compress(P) for P in pts))
        assert rc == OK and got == pts, (count, lib.apk_last_error())
    blob = b"".join(ov.compress(P) for P in rnd)
    bad = pm.encode(ov, 0b100 if cname == "bls12-381" else 0b10, _non_residue_x(cname))
    assert pm.accepts(ov, bad) is pm.REJECT
    for where in ([0], [255], [256], [512], [5, 300, 512]):
        b = bytearray(blob)
        for i in where:
            b[i * nb:(i + 1) * nb] = bad
        rc, _ = _decompress(cv, gpu, bytes(b))
        assert rc == ARG, where
        assert ("%d compressed point(s)" % len(where)).encode() in lib.apk_last_error(), (where, lib.apk_last_error())


# ---- 3, 4. ToLagrangeG1 ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g_times(cname, k):
    _, ov = CURVES[cname]
    return ov.mul(ov.g1, k)


def _lagrange_case(gpu, cname, a, src=None):
    """inputs a_j G -> every output against lagrange_of"""
    cv, ov = CURVES[cname]
    n = len(a)
    src = src if src is not None else [_g_times(cname, k % cv.r) for k in a]
    got = cv.g1_vector_decode(ap_setup.to_lagrange_g1(cv, cv.g1_vector(src), gpu))
    want = pm.lagrange_points(ov, a, n)
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (n, len(bad), bad[:8])


@pytest.mark.parametrize("cname", BOTH)
@pytest.mark.parametrize("n", [2, 4, 256, 512])
def test_to_lagrange_every_output_for_arbitrary_inputs(gpu, cname, n):
    """random a_j G that are not powers of anything.  n = 256: the butterflies are exactly one 128-lane workgroup; 512: four, and
    the twiddle index low << (log_n - 1 - t) is taken at every t"""
    ks, pts = _points(cname, 513)
    _lagrange_case(gpu, cname, ks[:n], pts[:n])


@pytest.mark.parametrize("cname", BOTH)
@pytest.mark.parametrize("n", [8, 256])
@pytest.mark.parametrize("kind", ["tau=0", "tau=1", "tau=omega", "tau=omega^(n-1)", "alternating", "zeros", "quarter zero"])
def test_to_lagrange_degenerate_inputs(gpu, cname, n, kind):
    """the complete-addition branches of the butterfly: infinity operands and scalar_mul_point of infinity (tau = 0, zeros, a
    quarter zero), equal operands then cancellation (tau = 1), tau on the domain (one output G, the rest infinity), opposite
    operands (alternating)"""
    cv, ov = CURVES[cname]
    r, w = cv.r, ov.omega(n)
    g = SplitMix64(0x7A6 + n)
    c = g.fr(r) or 1
    a = {"tau=0": [1] + [0] * (n - 1),
         "tau=1": [1] * n,
         "tau=omega": [pow(w, j, r) for j in range(n)],
         "tau=omega^(n-1)": [pow(w, (n - 1) * j, r) for j in range(n)],
         "alternating": [c if j % 2 == 0 else r - c for j in range(n)],
         "zeros": [0] * n,
         "quarter zero": [0 if j % 4 == 1 else g.fr(r) for j in range(n)]}[kind]
    want = pm.lagrange_of(a, n, r, w)
    known = {"tau=0": [pow(n, -1, r)] * n, "tau=1": [1] + [0] * (n - 1), "tau=omega": [int(i == 1) for i in range(n)],
             "tau=omega^(n-1)": [int(i == n - 1) for i in range(n)], "zeros": [0] * n}
    if kind in known:
        assert want == known[kind]
    _lagrange_case(gpu, cname, a)


# ---- 5. apk_g1_mul_batch --------------------------------------------------------------------------------------------------------
def _edge_scalars(r):
    s = [0, 1, 2, r - 1, r - 2]
    for k in (31, 32, 33, 63, 64, 65, 127, 128, 191, 192, 224):
        s += [1 << k, (1 << k) - 1]
    return s + [1 << (r.bit_length() - 1)]


@pytest.mark.parametrize("cname", BOTH)
@pytest.mark.parametrize("base", ["G", "-G", "random", "infinity"])
def test_g1_mul_batch_edge_scalars_bases_and_counts(gpu, cname, base):
    """0, 1, 2, r-1, r-2, single bits and runs of ones at the 32-bit word seams, r's top bit, random fill; on G, -G, a random
    point and infinity; counts 1, 255, 256, 257 (one prefix of the same list each, so every count ends on another scalar)"""
    cv, ov = CURVES[cname]
    g = SplitMix64(0xB45E)
    scalars = _edge_scalars(cv.r)
    scalars = scalars[3:] + scalars[:3]                           # count = 1 is r - 1, not 0
    scalars += [g.fr(cv.r) for _ in range(257 - len(scalars))]
    P = {"G": ov.g1, "-G": ov.neg(ov.g1), "random": _points(cname, 24)[1][21], "infinity": None}[base]
    want = [ov.mul(P, s) for s in scalars]
    for count in (1, 255, 256, 257):
        out = C.create_string_buffer(count * 2 * cv.fp_bytes)
        check(lib.apk_g1_mul_batch(cv.abi, gpu, cv.g1_to_bytes(P), cv.fr_vector(scalars[:count]), count, out))
        got = cv.g1_vector_decode(out.raw)
        bad = [i for i in range(count) if got[i] != want[i]]
        assert not bad, (count, bad[:8])


# ---- 6. segmented sums against the big-integer reference ------------------------------------------------------------------------
def _lincomb_case(gpu, cname, points, scalars, seg, want=None):
    cv, ov = CURVES[cname]
    if want is None:
        want = vbm.lincomb_reference(ov, points, scalars, seg)
    rc_d, dev = vbm.lincomb(cv, gpu, points, scalars, seg)
    assert rc_d == OK, lib.apk_last_error()
    rc_h, host = vbm.lincomb(cv, -1, points, scalars, seg)
    assert rc_h == OK, lib.apk_last_error()
    assert dev == want, [i for i in range(len(want)) if dev[i] != want[i]][:8]
    assert host == want, [i for i in range(len(want)) if host[i] != want[i]][:8]
    return want


@pytest.mark.parametrize("cname", BOTH)
def test_lincomb_scalars_at_the_window_seams(gpu, cname):
    """lincomb_partial_kernel cuts a scalar into four 64-bit windows across lanes: scalars that are one bit, or a run of ones,
    on either side of a seam - one term per segment, then all in one segment.  Then an input whose first and last segments
    are empty, and one of empty segments only."""
    cv, ov = CURVES[cname]
    scalars = [(1 << 64) - 1, 1 << 64, (1 << 64) + 1, (1 << 128) - 1, 1 << 128, 1 << 192, (1 << 192) - 1, cv.r - 1, 0, 1]
    pts = _points(cname, 24)[1][:len(scalars)]
    n = len(scalars)
    each = _lincomb_case(gpu, cname, pts, scalars, list(range(n + 1)))
    assert each[8] is None and each[9] == pts[9] and each[7] == ov.neg(pts[7])
    total = None
    for P in each:
        total = ov.add(total, P)
    assert _lincomb_case(gpu, cname, pts, scalars, [0, n]) == [total]
    assert _lincomb_case(gpu, cname, pts, scalars, [0, 0, 3, n, n])[0::3] == [None, None]
    _lincomb_case(gpu, cname, [], [], [0, 0, 0], want=[None, None])


@pytest.mark.parametrize("cname", BOTH)
@pytest.mark.parametrize("live", ["bottom window only", "top window only"])
def test_lincomb_segment_with_dead_windows(gpu, cname, live):
    """200 terms whose scalars are all below 2^64 (the window sums 1 to 3 are infinity: the Horner of lincomb_reduce_kernel
    doubles infinity 192 times) or all multiples of 2^192 (only the top window is live: three windows of infinity are added)"""
    cv, ov = CURVES[cname]
    g = SplitMix64(0xDEAD)
    pts = _points(cname, 513)[1]
    top = cv.r >> 192
    if live == "bottom window only":
        scalars = [g.next() or 1 for _ in range(200)]
        assert max(scalars) < 1 << 64
    else:
        scalars = [(1 + g.below(top - 1)) << 192 for _ in range(200)]
        assert all(s < cv.r and s % (1 << 192) == 0 for s in scalars)
    _lincomb_case(gpu, cname, pts[:200], scalars, [0, 200])


@pytest.mark.parametrize("cname", BOTH)
def test_lincomb_segment_lengths_around_the_tree(gpu, cname):
    """lengths 63, 64, 65, 128, 129 around LINCOMB_TREE = 64 with every third point at infinity; 64 copies of (a, P): a doubling
    at every level of the tree; 65 x (a, P) then 65 x (a, -P): equal operands up the tree and infinity at its root"""
    cv, ov = CURVES[cname]
    g = SplitMix64(0x7EE)
    pts = _points(cname, 513)[1]
    lens = [63, 64, 65, 128, 129]
    seg = [0]
    for ln in lens:
        seg.append(seg[-1] + ln)
    n = seg[-1]
    points = [None if i % 3 == 2 else pts[i] for i in range(n)]
    scalars = [g.fr(cv.r) for _ in range(n)]
    _lincomb_case(gpu, cname, points, scalars, seg)
    a, P = g.fr(cv.r), pts[7]
    aP = ov.mul(P, a)
    assert _lincomb_case(gpu, cname, [P] * 64, [a] * 64, [0, 64]) == [ov.mul(aP, 64)]
    assert _lincomb_case(gpu, cname, [P] * 65 + [ov.neg(P)] * 65, [a] * 130, [0, 130]) == [None]


# ---- 7. the point check on the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", BOTH)
@pytest.mark.parametrize("what", ["off the curve", "infinity"])
def test_point_check_on_the_device(gpu, cname, what):
    """8 proofs = 72 checked points = two 64-lane workgroups of g1_check_kernel.  One commitment of proof 1 (lane 9 of the first
    workgroup), then one of proof 7 (lane 66: the second), replaced by (x, y + 1) - on no curve - or by the point at infinity:
    statuses and the rejected index equal host mode's, the rest of the batch is accepted, and an off-curve point is refused by
    the DEVICE's check (its text), before the host's own."""
    m = vbm.material(cname, "pyth")
    cv, ov = m.cv, m.ov
    for j, slot in ((1, "lro"), (7, "z")):
        raws, pubs, oprs = m.take(8)
        P = oprs[j].lro[0] if slot == "lro" else oprs[j].z
        Q = None if what == "infinity" else (P[0], (P[1] + 1) % cv.p)
        assert P is not None and (Q is None or not ov.is_on_curve(Q))
        b = cv.g1_to_bytes(Q)
        C.memmove(raws[j].lro[0] if slot == "lro" else raws[j].z, b, len(b))
        rc_d, st_d, _ = vbm.run_batch(m.vk, raws, pubs, device=gpu)
        err_d = lib.apk_last_error()
        rc_h, st_h, _ = vbm.run_batch(m.vk, raws, pubs, device=-1)
        err_h = lib.apk_last_error()
        assert rc_d == rc_h == BAD and st_d == st_h == [BAD if i == j else OK for i in range(8)], (j, st_d, st_h, err_d)
        assert ("proof %d rejected" % j).encode() in err_d and ("proof %d rejected" % j).encode() in err_h
        if what == "off the curve":
            assert b"not on the curve (device check)" in err_d, err_d
            assert b"not on the curve" in err_h and b"device check" not in err_h, err_h
        else:
            assert b"pairing check" in err_d and b"pairing check" in err_h, (err_d, err_h)


def test_zero_counts_are_answered_before_any_launch(gpu):
    """count = 0 and zero segments return APK_OK from the C-ABI itself (no empty grid is ever launched); ToLagrangeG1 has no
    size below 2"""
    cv, ov = CURVES["bn254"]
    out = C.create_string_buffer(2 * cv.fp_bytes)
    assert lib.apk_g1_decompress(cv.abi, gpu, ov.compress(ov.g1), 0, out) == OK
    assert lib.apk_g1_mul_batch(cv.abi, gpu, cv.g1_to_bytes(ov.g1), cv.fr_vector([1]), 0, out) == OK
    assert lib.apk_g1_lincomb_segments(cv.abi, gpu, None, None, (C.c_uint64 * 1)(0), 0, out) == OK
    assert not any(out.raw)
    for n in (0, 1, 3):
        assert lib.apk_g1_to_lagrange(cv.abi, gpu, cv.g1_to_bytes(ov.g1) * max(n, 1), n, out) == ARG

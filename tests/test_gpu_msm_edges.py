"""GPU tier: the MSM at the edges of its signed-digit recoding and at the sizes where the window planner's limits bind, against
plain references (the known-tau rule and its closed forms, the C oracle).  The words, layouts and planner rules come from
tests/msm_model.py, which tests/test_msm_model.py holds to its definitions on the CPU."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
import time

import pytest

import msm_model as mm
from algoplonk_amd import _lib, frontend, plonk as ap_plonk, setup as ap_setup
from algoplonk_amd._lib import check, lib
from helpers import CURVES, oracle_threads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lagrange_coeffs(r: int, n: int, tau: int, omega: int):
    """L_i(tau) = omega^i (tau^n - 1) / (n (tau - omega^i)) for i < n, then tau^(n+k) - tau^k for the three blinding points of the
    extended Lagrange table: what the bases of a basis-1 MSM are worth in the exponent."""
    zn = (pow(tau, n, r) - 1) * pow(n, -1, r) % r
    out, wi = [], 1
    for _ in range(n):
        out.append(wi * zn % r * pow((tau - wi) % r, -1, r) % r)
        wi = wi * omega % r
    return out + [(pow(tau, n + k, r) - pow(tau, k, r)) % r for k in range(3)]


def _form(pc: dict) -> str:
    return "fused" if pc["msm_sort_fused"] else "four-launch" if pc["msm_sort_two_level"] else "one-level"


# ---- B: the digit-edge matrix -------------------------------------------------------------------------------------------------
# One process per (curve, sort form): the knobs are read once, into statics.  Inside it one SRS (n = 2^11, with its Lagrange form)
# serves every window c = 7..20 (one context per c), both bases and every length.
_EDGE_SCRIPT = r"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from algoplonk_amd import plonk, setup
from algoplonk_amd._lib import lib, check
from oracle.prng import tau_from_seed
from helpers import CURVES, random_chain_ccs
import msm_model as mm
from test_gpu_msm_edges import _form, _lagrange_coeffs
cname, form = sys.argv[1], sys.argv[2]
cv, ov = CURVES[cname]
r, n = cv.r, 1 << 11
nb = n + 3
bits, fp = mm.curve_bits(cname), mm.CURVE_PARAMS[cname][1]
sort2_env, fused_env = (-1, 1) if form == "default" else (1, 0 if form == "four-launch" else 1)
t0 = time.time()
ccs, _, _ = random_chain_ccs(cv, 11, 0xED6E)
tau = tau_from_seed(0xED6E, r)
srs = setup.unsafe_srs(cv, n, tau, device=0, lagrange=True)
coeffs = ([pow(tau, i, r) for i in range(nb)], _lagrange_coeffs(r, n, tau, cv.omega(n)))
rinv = pow(mm.R_MONT, -1, r)
fails, forms_seen = [], {}
for c in range(7, 21):
    pk, vk = plonk.Setup(ccs, srs, device=0, msm_window=c)
    if pk.msm_window != c:
        fails.append("c=%d: apk_ctx_msm_window = %d" % (c, pk.msm_window))
    p = mm.plan(bits, fp, c, 11, nb)
    for basis in (0, 1):
        # basis 0 splits the raw word it is given (value m R^-1), basis 1 the canonical value of its Montgomery word
        words = mm.edge_scalars(r, p.lay, "raw" if basis == 0 else "canonical", seed=c).values
        enc = (lambda m: m.to_bytes(32, "little")) if basis == 0 else cv.fr_to_mont_bytes
        val = (lambda m: m * rinv % r) if basis == 0 else (lambda m: m)
        coef = coeffs[basis]
        start = (97 * c + 31 * basis) % len(words)
        seq = [words[(start + i) % len(words)] for i in range(nb)]
        vals = [val(m) for m in seq]
        buf = b"".join(enc(m) for m in seq)
        out = C.create_string_buffer(2 * cv.fp_bytes)
        for L in (nb, 1, 2, 65, 2049, 2048):
            pk.paths(reset=True)
            rc = lib.apk_msm_g1(pk.ctx, basis, buf, L, out)
            pc = pk.paths(reset=True)
            if rc != 0:
                fails.append("c=%d basis=%d L=%d: rc %d %s" % (c, basis, L, rc, lib.apk_last_error())); continue
            want = ov.mul(ov.g1, sum(v * k for v, k in zip(vals[:L], coef)) % r)
            if cv.g1_from_bytes(out.raw) != want:
                fails.append("c=%d basis=%d L=%d: wrong group element" % (c, basis, L))
            got, exp = _form(pc), mm.sort_form(p, nb, L, sort2_env=sort2_env, fused_env=fused_env)
            forms_seen.setdefault(c, set()).add(got)
            if pc["msm_batches"] != 1 or got != exp:
                fails.append("c=%d basis=%d L=%d: sort %s, the model expects %s (%s)" % (c, basis, L, got, exp, pc))
        # one batch of four ranges of mixed lengths, the last ending at the last base
        segs = [(0, 1), (1, 66), (66, 68), (nb - 2049, nb)]
        d = C.c_void_p()
        check(lib.apk_device_alloc(pk.ctx, len(buf), C.byref(d)))
        check(lib.apk_device_upload(pk.ctx, d, buf, len(buf)))
        k = len(segs)
        ptrs, offs, ls = (C.c_void_p * k)(), (C.c_uint64 * k)(), (C.c_uint64 * k)()
        for i, (lo, hi) in enumerate(segs):
            ptrs[i], offs[i], ls[i] = d.value + 32 * lo, lo, hi - lo
        bout = C.create_string_buffer(k * 2 * cv.fp_bytes)
        pk.paths(reset=True)
        rc = lib.apk_msm_g1_batch_device(pk.ctx, basis, k, ptrs, offs, ls, bout)
        pc = pk.paths(reset=True)
        check(lib.apk_device_free(pk.ctx, d))
        if rc != 0:
            fails.append("c=%d basis=%d batch: rc %d %s" % (c, basis, rc, lib.apk_last_error())); continue
        for (lo, hi), P in zip(segs, cv.g1_vector_decode(bout.raw)):
            if P != ov.mul(ov.g1, sum(vals[i] * coef[i] for i in range(lo, hi)) % r):
                fails.append("c=%d basis=%d batch range [%d, %d): wrong group element" % (c, basis, lo, hi))
        got, exp = _form(pc), mm.sort_form(p, nb, 2049, batch=k, sort2_env=sort2_env, fused_env=fused_env)
        forms_seen.setdefault(c, set()).add(got)
        if pc["msm_batches"] != 1 or got != exp:
            fails.append("c=%d basis=%d batch: sort %s, the model expects %s (%s)" % (c, basis, got, exp, pc))
    pk.close()
print("FORMS", cname, form, {c: sorted(v) for c, v in forms_seen.items()})
for f in fails[:40]:
    print("FAIL", f)
print("EDGE_DONE %d failures %.1f s" % (len(fails), time.time() - t0))
sys.exit(1 if fails else 0)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "fused", "four-launch"])
@pytest.mark.parametrize("cname", ["bn254", "bls12-381"])
def test_signed_digit_edges_every_window_every_recoding(gpu, cname, form):
    """Every window width c = 7..20, on the canonical table (basis 0: the kernels split the raw Montgomery word) and on the plain
    Lagrange table (basis 1: the PLAIN kernels split the canonical value), with words whose digits sit on every edge of the
    recoding (msm_model.edge_scalars), through the three copies of the digit loop: the one-level sort (default; from c = 18 the
    sort is two levels only), the fused two-level sort (APK_MSM_SORT2=1) and its four-launch form (APK_MSM_SORT_FUSED=0).  Every
    call's path counters must show the form msm_model.sort_form predicts (at n = 2^11, c = 8..10 leave fewer than four
    partitions, so they sort in one level even when two are asked for; the fused form needs runs of 64 entries per partition,
    which c = 18..20 do not give)."""
    env = dict(os.environ)
    env.pop("APK_MSM_WINDOW", None)
    if form != "default":
        env["APK_MSM_SORT2"] = "1"
    if form == "four-launch":
        env["APK_MSM_SORT_FUSED"] = "0"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    t0 = time.time()
    out = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", _EDGE_SCRIPT, cname, form], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=660)
    print(out.stdout[-3000:], "%.1f s" % (time.time() - t0))
    assert out.returncode == 0 and "EDGE_DONE 0 failures" in out.stdout, (out.stdout[-4000:], out.stderr[-2000:])
    forms = [ln for ln in out.stdout.splitlines() if ln.startswith("FORMS")][0]
    assert {"default": "one-level", "fused": "fused", "four-launch": "four-launch"}[form] in forms, forms


# ---- C: the large-size plans --------------------------------------------------------------------------------------------------
# The bases repeat a 2^20-point known-tau SRS: base i = tau^(i mod 2^20) G.  Nothing in the kernels depends on the points being
# distinct, and the host SRS stays cheap.  Every scalar family repeats a block of B | 2^20 words, so the known-tau reference has a
# closed form (geometric sums over the block); up to 2^21 the uniform family is also held to the C oracle's MSM.
PERIOD = 1 << 20
_SRS_CACHE = {}


def _cyclic_srs(cname):
    if cname not in _SRS_CACHE:
        cv, _ = CURVES[cname]
        from oracle.prng import tau_from_seed
        tau = tau_from_seed(0xB16, cv.r)
        pw = [1] * PERIOD
        for i in range(1, PERIOD):
            pw[i] = pw[i - 1] * tau % cv.r
        _SRS_CACHE.clear()                      # one curve's at a time
        _SRS_CACHE[cname] = (tau, ap_setup._mul_base_batch(cv, pw, 0))
    return _SRS_CACHE[cname]


def _bases(cname, count):
    tau, g1 = _cyclic_srs(cname)
    pt = len(g1) // PERIOD
    reps = -(-count // PERIOD)
    return tau, (g1 * reps)[: count * pt] if reps > 1 else g1[: count * pt]


def _block_sum(r, tau, vals, x):
    """sum_{i < x} vals[i mod B] tau^i for x <= PERIOD, B = len(vals) dividing PERIOD: block entry b recurs with ratio tau^B."""
    B = len(vals)
    a = pow(tau, B, r)
    inv = pow(a - 1, -1, r)
    q, rem = divmod(x, B)
    g_lo, g_hi = (pow(a, q, r) - 1) * inv % r, (pow(a, q + 1, r) - 1) * inv % r
    s, t = 0, 1
    for b, v in enumerate(vals):
        if v:
            s += v * t * (g_hi if b < rem else g_lo)
        t = t * tau % r
    return s % r


def _periodic_sum(r, tau, vals, lo, hi):
    """sum_{lo <= i < hi} vals[i mod B] tau^(i mod PERIOD): the known-tau value of an MSM over [lo, hi) of the cyclic bases."""
    def S(L):
        q, rem = divmod(L, PERIOD)
        return (q * _block_sum(r, tau, vals, PERIOD) + _block_sum(r, tau, vals, rem)) % r
    return (S(hi) - S(lo)) % r


def _uniform_words(r, count, seed):
    import hashlib
    raw = hashlib.shake_256(b"apk msm plans %d" % seed).digest(32 * count * 2)
    out, i, mask = [], 0, (1 << r.bit_length()) - 1
    while len(out) < count:                      # rejection: uniform over all of [0, r), no clamp below a power of two
        m = int.from_bytes(raw[i: i + 32], "little") & mask
        i += 32
        if m < r:
            out.append(m)
    return out


LARGE = [("bn254", 1 << 18, 0), ("bn254", 1 << 20, 0), ("bn254", 1 << 21, 0), ("bn254", (1 << 21) + 3, 0), ("bn254", 1 << 22, 0),
         ("bn254", 1 << 23, 0), ("bn254", 1 << 24, 0), ("bn254", 786432, 17),
         ("bls12-381", 1 << 20, 0), ("bls12-381", 1 << 21, 0), ("bls12-381", (1 << 21) + 3, 0), ("bls12-381", 1 << 22, 0),
         ("bls12-381", 1 << 23, 0)]
ORC_MSM_MAX = 1 << 21          # the C oracle's MSM beside the closed form up to here


@pytest.mark.gpu
@pytest.mark.parametrize("cname,count,window", LARGE, ids=["%s-%d-c%d" % x for x in LARGE])
def test_large_size_plans_against_closed_forms(gpu, cname, count, window):
    """MSM-only contexts at the sizes where choose_window's limits bind: the window the library picks must be the model's
    (msm_model.default_window restates choose_window), and every scalar family - uniform raw words over [0, r), the recoding's
    edge words at that window, all-equal, every digit = half, zeros with every eighth entry uniform - must give the known-tau
    value at the full length and one less.  A four-range batch on an MSM-only context (its workspace holds one MSM) must give the
    right sums or a clean APK_ERR_ARG, never a wrong point."""
    cv, ov = CURVES[cname]
    r = cv.r
    t0 = time.time()
    tau, bases = _bases(cname, count)
    ctx = C.c_void_p()
    check(lib.apk_msm_ctx_create(cv.abi, gpu, bases, count, window, C.byref(ctx)))
    d = C.c_void_p()
    try:
        c = lib.apk_ctx_msm_window(ctx)
        lg = mm.msm_only_log_size(count)
        assert c == (window or mm.default_window(cname, lg, bases=count)), c
        p = mm.plan(mm.curve_bits(cname), mm.CURVE_PARAMS[cname][1], window, lg, count)
        rinv = pow(mm.R_MONT, -1, r)
        uni = _uniform_words(r, 1 << 12, count)
        edges = mm.edge_scalars(r, p.lay, "raw", seed=count).values
        families = {
            "uniform": _uniform_words(r, 1 << 16, count + 1),
            "edges": [edges[b % len(edges)] for b in range(1 << 12)],
            "all-equal": [uni[0]],
            "all-half": [mm.all_half(r, p.lay)],
            "sparse-uniform": [uni[b] if b % 8 == 0 else 0 for b in range(1 << 12)],
        }
        check(lib.apk_device_alloc(ctx, 32 * count, C.byref(d)))
        out = C.create_string_buffer(2 * cv.fp_bytes)
        report = {"c": c, "P": p.P, "pb_log": p.pb_log, "idx_bits": p.idx_bits}
        clib = None
        for name, blk in families.items():
            wb = b"".join(m.to_bytes(32, "little") for m in blk)
            buf = (wb * -(-count // len(blk)))[: 32 * count]
            check(lib.apk_device_upload(ctx, d, buf, len(buf)))
            vals = [m * rinv % r for m in blk]
            for L in (count, count - 1):
                pc = _lib.PathCounts()
                check(lib.apk_paths_read(ctx, C.byref(pc), 1))
                check(lib.apk_msm_g1_device(ctx, 0, d, L, out))
                check(lib.apk_paths_read(ctx, C.byref(pc), 1))
                pcd = pc.as_dict()
                assert cv.g1_from_bytes(out.raw) == ov.mul(ov.g1, _periodic_sum(r, tau, vals, 0, L)), (name, L, report, pcd)
                report["%s/%d" % (name, L)] = _form(pcd)
                assert pcd["msm_batches"] == 1 and _form(pcd) == mm.sort_form(p, count, L), (name, L, pcd)
                if name == "uniform" and L == count and count <= ORC_MSM_MAX:
                    from oracle import c_oracle
                    clib = clib or c_oracle.load()
                    want = C.create_string_buffer(2 * cv.fp_bytes)
                    assert clib.orc_msm(cv.abi, bases, buf, L, oracle_threads(), want) == 0
                    assert out.raw == want.raw, ("orc_msm", L)
            # four ranges of mixed lengths, the last ending at the last base
            segs = [(0, 1), (1, 4097), (5, count // 3), (count // 2, count)]
            k = len(segs)
            ptrs, offs, ls = (C.c_void_p * k)(), (C.c_uint64 * k)(), (C.c_uint64 * k)()
            for i, (lo, hi) in enumerate(segs):
                ptrs[i], offs[i], ls[i] = d.value + 32 * lo, lo, hi - lo
            bout = C.create_string_buffer(k * 2 * cv.fp_bytes)
            rc = lib.apk_msm_g1_batch_device(ctx, 0, k, ptrs, offs, ls, bout)
            report["batch"] = rc
            if rc == 0:
                for (lo, hi), P in zip(segs, cv.g1_vector_decode(bout.raw)):
                    assert P == ov.mul(ov.g1, _periodic_sum(r, tau, vals, lo, hi)), (name, "batch", lo, hi)
            else:
                assert rc == _lib.APK_ERR_ARG, (rc, lib.apk_last_error())
        report["s"] = round(time.time() - t0, 1)
        print("large plan", cname, count, report)
    finally:
        if d.value:
            lib.apk_device_free(ctx, d)
        lib.apk_ctx_destroy(ctx)


@pytest.mark.gpu
def test_large_size_refusals(gpu):
    """A window the planner cannot serve is refused at creation with APK_ERR_ARG, not turned into a wrong MSM: 17 bits beyond the
    packed 16-bit counters' 786 432 bases, 19 bits at 2^23 bases (16 384 partitions: no room for the partition bits)."""
    cv, _ = CURVES["bn254"]
    for count, window, msg in ((786433, 17, "at most 786432"), (1 << 23, 19, "leave no room for the partition bits")):
        _, bases = _bases("bn254", count)
        ctx = C.c_void_p()
        assert lib.apk_msm_ctx_create(cv.abi, gpu, bases, count, window, C.byref(ctx)) == _lib.APK_ERR_ARG
        assert msg in lib.apk_last_error().decode(), lib.apk_last_error()
        with pytest.raises(mm.PlanError, match=msg):
            mm.plan(mm.curve_bits("bn254"), 8, window, mm.msm_only_log_size(count), count)


# ---- D: whole proofs at the untested sizes and with the realistic skew ------------------------------------------------------
PROOFS = [("bn254", 18, "random"), ("bn254", 20, "random"), ("bn254", 17, "skewed"), ("bn254", 20, "skewed"), ("bls12-381", 14, "skewed")]


@pytest.mark.gpu
@pytest.mark.parametrize("cname,log_n,kind", PROOFS, ids=["%s-2p%d-%s" % x for x in PROOFS])
def test_proofs_at_the_planner_sizes_match_the_c_oracle(gpu, cname, log_n, kind):
    """Byte for byte against the C oracle's prover: BN254 2^18 on a lone context (17-bit windows with packed LDS counters, a 2^20
    NTT for the quotient), and the bit-heavy witness of workloads.skewed_circuit (~80 % of the wire values in {0, 1}) with a
    Lagrange SRS, whose wire commitments go to the plain Lagrange table - bucket 1 of the lowest window then holds most of the
    entries - as msm_lagrange_wires must show for every proof."""
    from algoplonk_amd import MarshalProof, workloads
    from oracle import c_oracle
    cv, ov = CURVES[cname]
    t0 = time.time()
    wl = (workloads.skewed_circuit if kind == "skewed" else workloads.random_circuit)(cv, log_n, 0xD0 + log_n)
    n = wl.ccs.domain_size()
    srs = ap_setup.unsafe_srs(cv, n, wl.tau, device=gpu, lagrange=kind == "skewed")
    pk, vk = ap_plonk.Setup(wl.ccs, srs, device=gpu)
    try:
        assert pk.msm_window == mm.default_window(cname, log_n)
        pk.paths(reset=True)
        blobs = [MarshalProof(ap_plonk.Prove(wl.ccs, pk, wl.witness, wl.blinding)) for _ in range(2)]
        paths = pk.paths(reset=True)
    finally:
        pk.close()
    tr = frontend.build_trace(wl.ccs)
    L, R, O = frontend.wire_columns(wl.ccs, wl.solution)
    rc, want, _ = c_oracle.prove(c_oracle.load(), cv.abi, n, wl.ccs.GetNbPublicVariables(), srs.g1,
                                 [cv.fr_vector(x) for x in (tr.ql, tr.qr, tr.qm, tr.qo, tr.qk)], tr.perm, cv.fr_vector(L),
                                 cv.fr_vector(R), cv.fr_vector(O), cv.fr_vector(wl.witness.public), cv.fr_vector(wl.blinding),
                                 threads=oracle_threads())
    print("proof", cname, log_n, kind, "c =", mm.default_window(cname, log_n), paths, "%.1f s" % (time.time() - t0))
    assert rc == 0 and blobs[0] == want and blobs[1] == want
    assert paths["proofs"] == 2
    if kind == "skewed":
        assert paths["msm_lagrange_wires"] == 2, paths

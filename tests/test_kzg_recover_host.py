"""CPU tier of the recovery of a polynomial from a sufficient set of its cells (include/apk.h apk_kzg_recover_cosets*,
csrc/kernels_kzg_recover.h): steps (1) - (6) restated on big integers (tests/kzg_recover_model.py) and held to a direct Lagrange
interpolation; apk_kzg_recover_cosets_host held to the model byte for byte at the shapes of the GPU tier; the invariant that ANY k
rows give no coefficient at or above k l; the verdict; every argument rule at its edge, through the host call and through the
planner's dump (csrc/kzg_recover_plan.h via tools/kzg_recover_plan_dump), which is held to a Python restatement; the planner and
the host recovery stand-alone under ASAN + UBSAN; the exports; the argument errors that come before the device check; the Python
wrappers' argument errors.  No GPU."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess

import pytest

import kzg_recover_model as krm
from algoplonk_amd import _lib, kzg as ap_kzg
from algoplonk_amd._lib import lib
from helpers import CURVES
from oracle.prng import SplitMix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
NAMES = ["bn254", "bls12-381"]
OK, ERR_ARG, ERR_HIP, ERR_VERIFY = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_HIP, _lib.APK_ERR_VERIFY
NEW = ["apk_kzg_recover_cosets", "apk_kzg_recover_cosets_device", "apk_kzg_recover_cosets_host"]
GPU_SHAPES = [(3, 2), (3, 4), (7, 2), (7, 64), (9, 16), (10, 2)]      # (log n, l): tests/test_gpu_kzg_recover.py
WORDS = ["plans", "grids", "rules"]


def test_model_constants_are_the_librarys():
    assert (krm.OK, krm.ERR_ARG, krm.ERR_VERIFY) == (OK, ERR_ARG, ERR_VERIFY)
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    assert "#define APK_KZG_RECOVER_MAX_COSETS (1u << 16)" in hdr and krm.MAX_COSETS == 1 << 16
    plan = open(os.path.join(CSRC, "kzg_recover_plan.h")).read()
    assert "KZG_RECOVER_THREADS = %d;" % krm.THREADS in plan and "KZG_RECOVER_TILE = %d;" % krm.TILE in plan


def known_sets(np, g):
    """structured and random sets of known cosets, by name; the rows of the random ones come shuffled"""
    sets = {"all": list(range(np)), "one": [np - 1], "first-half": list(range(max(np // 2, 1))), "even": list(range(0, np, 2))}
    for k in sorted({1, max(np // 2, 1), np - 1} - {0}):
        pool = list(range(np))
        for i in range(np - 1, 0, -1):
            j = g.next() % (i + 1)
            pool[i], pool[j] = pool[j], pool[i]
        sets["random-%d" % k] = pool[:k]
    return sets


# ---- the model against the Lagrange witness ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 16, 64])
@pytest.mark.parametrize("cname", NAMES)
def test_model_equals_lagrange_interpolation(cname, n):
    """every l, every k from 1 to n' (a seeded random set each), and the structured sets: steps (1) - (6) on ARBITRARY rows give the
    polynomial below degree k l through the k l points, and nothing at or above k l"""
    cv, _ = CURVES[cname]
    r, w, gs = cv.r, cv.omega(n), cv.coset_shift
    g = SplitMix64(0xEC0 + n + cv.abi)
    l = 2
    while l <= n // 2:
        np = n // l
        sets = list(known_sets(np, g).values())
        for k in range(1, np + 1):
            pool = list(range(np))
            for i in range(np - 1, 0, -1):
                j = g.next() % (i + 1)
                pool[i], pool[j] = pool[j], pool[i]
            sets.append(pool[:k])
        if n == 64:      # (one model run costs O(n' m + n log n) multiplications, the witness O((k l)^2): a sample of the sets at 64)
            sets = sets[::3]
        for known in sets:
            rows = [[g.fr(r) for _ in range(l)] for _ in known]
            f = krm.steps(n, l, known, rows, w, gs, r)
            assert not any(f[len(known) * l:]), (cname, n, l, known)
            assert f[:len(known) * l] == krm.lagrange(n, l, known, rows, w, r), (cname, n, l, known)
        l *= 2


def test_model_returns_the_polynomial_whose_cells_it_is_given():
    cv, _ = CURVES["bn254"]
    r, n, l = cv.r, 64, 4
    w, gs = cv.omega(n), cv.coset_shift
    g = SplitMix64(0xEC1)
    f = [g.fr(r) for _ in range(n // 2)]
    cs = krm.cells(f, n, l, w, r)
    known = [15, 0, 3, 9, 8, 2, 11, 6]
    rows = [cs[i] for i in known]
    assert krm.recover(n, l, known, rows, n // 2, w, gs, r) == f
    assert krm.recover(n, l, known, rows, n // 2 - 1, w, gs, r) is None
    assert krm.recover(n, l, known + [1], rows + [cs[1]], n // 2, w, gs, r) == f      # a spare cell


# ---- apk_kzg_recover_cosets_host against the model -------------------------------------------------------------------------------------
def _host(cv, n, l, known, rows, length, out=None):
    """(rc, bytes)"""
    k = len(known)
    out = out or C.create_string_buffer(b"\xa5" * (32 * length), 32 * length)
    rc = lib.apk_kzg_recover_cosets_host(cv.abi, n, l, k, (C.c_uint64 * k)(*known), cv.fr_vector([v for row in rows for v in row]), length, out)
    return rc, out.raw


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "%dx%d" % (1 << s[0], s[1]))
@pytest.mark.parametrize("cname", NAMES)
def test_host_call_equals_the_model_byte_for_byte(cname, shape):
    cv, _ = CURVES[cname]
    r, n, l = cv.r, 1 << shape[0], shape[1]
    np, w, gs = n // l, cv.omega(n), cv.coset_shift
    g = SplitMix64(0xEC2 + 16 * shape[0] + l + cv.abi)
    f_full = [g.fr(r) for _ in range(n)]
    for name, known in known_sets(np, g).items():
        k = len(known)
        f = f_full[:k * l]
        cs = krm.cells(f, n, l, w, r)
        rows = [cs[i] for i in known]
        for length in sorted({k * l, k * l - l + 1}):
            fl = f[:length]
            rows_l = rows if length == k * l else [krm.cells(fl, n, l, w, r)[i] for i in known]
            rc, raw = _host(cv, n, l, known, rows_l, length)
            assert rc == OK, (cname, shape, name, length, lib.apk_last_error())
            assert raw == cv.fr_vector(fl), (cname, shape, name, length)
        if n <= 128:      # the model itself, on rows that are no polynomial's cells
            arb = [[g.fr(r) for _ in range(l)] for _ in known]
            rc, raw = _host(cv, n, l, known, arb, k * l)
            assert rc == OK and raw == cv.fr_vector(krm.steps(n, l, known, arb, w, gs, r)[:k * l]), (cname, shape, name)


@pytest.mark.parametrize("cname", NAMES)
def test_arbitrary_rows_have_no_coefficient_at_or_above_kl(cname):
    """through the host call: with len = k l every set of rows is accepted (there is nothing to check), and the polynomial it returns
    has the rows as its cells"""
    cv, _ = CURVES[cname]
    r, n, l = cv.r, 128, 8
    w = cv.omega(n)
    g = SplitMix64(0xEC3 + cv.abi)
    for known in ([5], [0, 15], [3, 1, 4, 15, 9, 2, 6], list(range(16))):
        rows = [[g.fr(r) for _ in range(l)] for _ in known]
        rc, raw = _host(cv, n, l, known, rows, len(known) * l)
        assert rc == OK, lib.apk_last_error()
        f = cv.fr_vector_decode(raw)
        cs = krm.cells(f, n, l, w, r)
        assert [cs[i] for i in known] == rows, known


@pytest.mark.parametrize("cname", NAMES)
def test_verdict_on_rows_of_a_longer_polynomial(cname):
    cv, _ = CURVES[cname]
    r, n, l = cv.r, 64, 4
    g = SplitMix64(0xEC4 + cv.abi)
    known = [7, 12, 1, 2, 10]
    kl = len(known) * l
    f = [g.fr(r) for _ in range(kl - 1)] + [g.fr(r) or 1]
    cs = krm.cells(f, n, l, cv.omega(n), r)
    rows = [cs[i] for i in known]
    mark = b"\xa5" * (32 * (kl - 1))
    out = C.create_string_buffer(mark, len(mark))
    rc, raw = _host(cv, n, l, known, rows, kl - 1, out)
    assert rc == ERR_VERIFY and raw == mark and b"not those of one polynomial" in lib.apk_last_error()
    rc, raw = _host(cv, n, l, known, rows, kl)
    assert rc == OK and raw == cv.fr_vector(f)
    # a non-zero coefficient anywhere in [len, k l) is seen: only coefficient len itself, and only the last one
    for top in (kl - 8, kl - 1):
        f2 = f[:kl - 8] + [0] * 8
        f2[top] = 1
        cs2 = krm.cells(f2, n, l, cv.omega(n), r)
        assert _host(cv, n, l, known, [cs2[i] for i in known], kl - 8)[0] == ERR_VERIFY, top
    cs3 = krm.cells(f[:kl - 8], n, l, cv.omega(n), r)
    assert _host(cv, n, l, known, [cs3[i] for i in known], kl - 8) == (OK, cv.fr_vector(f[:kl - 8]))


# ---- the rules at their edges, through the host call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", NAMES)
def test_argument_rules_of_the_host_call(cname):
    cv, _ = CURVES[cname]
    n, l, np = 64, 4, 16
    rows = C.create_string_buffer(32 * (n + l))
    mark = b"\xa5" * (32 * (n + 1))
    out = C.create_string_buffer(mark, len(mark))

    def call(n=n, l=l, idx=(0, 1, 2, 3), length=16, curve=cv.abi, rows=rows, out=out, indices=True):
        arr = (C.c_uint64 * max(len(idx), 1))(*idx)
        return lib.apk_kzg_recover_cosets_host(curve, n, l, len(idx), arr if indices else None, rows, length, out)

    assert call() == OK
    assert out.raw[:32 * 16] == bytes(32 * 16) and out.raw[32 * 16:] == mark[32 * 16:]      # zero rows: the zero polynomial, len words
    out.raw = mark
    cases = {
        "null indices": dict(indices=False), "null values": dict(rows=None), "null out": dict(out=None), "curve": dict(curve=7),
        "count=0": dict(idx=()), "len=0": dict(length=0), "l=0": dict(l=0), "l=1": dict(l=1), "l=3": dict(l=3), "l=n": dict(l=n, idx=(0,), length=1),
        "n=0": dict(n=0), "n=2": dict(n=2, l=2, idx=(0,), length=1), "n=48": dict(n=48), "n=2^25": dict(n=1 << 25), "n=2^40": dict(n=1 << 40),
        "count=n'+1": dict(idx=tuple(range(np + 1)), length=n), "len=kl+1": dict(length=17), "index=n'": dict(idx=(0, 1, 2, np)),
        "repeat": dict(idx=(0, 1, 2, 1)),
    }
    for name, kw in cases.items():
        assert call(**kw) == ERR_ARG, name
        assert lib.apk_last_error(), name
        assert out.raw == mark, name
    assert call(length=17) == ERR_ARG and b"too few cells" in lib.apk_last_error() and b"need 5 cells" in lib.apk_last_error()
    # the accepted side of every edge
    assert call(idx=tuple(range(np)), length=n) == OK                 # count = n'
    assert call(length=16) == OK                                      # len = k l
    assert call(idx=(0, 1, 2, np - 1)) == OK                          # index = n' - 1
    assert call(l=n // 2, idx=(1,), length=n // 2) == OK              # l = n / 2
    assert call(n=4, l=2, idx=(1,), length=2) == OK                   # the smallest domain


# ---- the planner: its dump held to the restatement ---------------------------------------------------------------------------------------
def _run(target, path, env=None, words=WORDS):
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, *path)] + list(words), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r


@pytest.fixture(scope="module")
def dump():
    lines = [json.loads(x) for x in _run("recover-plan-dump", ("tools", "kzg_recover_plan_dump")).stdout.splitlines()]
    return {"plans": [x for x in lines if "indices" in x], "grids": [x for x in lines if "indices" not in x and "np" in x],
            "rules": [x for x in lines if "rule" in x]}


def test_planner_row_map_launches_and_check_range(dump):
    assert len(dump["plans"]) >= 40
    seen = set()
    for p in dump["plans"]:
        n, l, idx = p["n"], p["l"], p["indices"]
        want = krm.plan(n, l, idx, p["len"])
        assert p["rc"] == OK == want["rc"], p
        for key in ("np", "k", "m", "row_of", "missing", "vanish", "scatter", "divide", "tiles", "check"):
            assert p[key] == want[key], (key, n, l, idx)
        assert p["logs"] == [n.bit_length() - 1, l.bit_length() - 1, (n // l).bit_length() - 1]
        # the row map is the inverse of the index list; the missing cosets are the rest, ascending
        assert all(p["row_of"][i] == row for row, i in enumerate(idx)) and sorted(p["missing"] + idx) == list(range(n // l))
        assert p["check"] == [p["len"], len(idx) * l]
        seen.add((n, l))
    assert seen == {(1 << k, l) for k in range(2, 7) for l in (2, 4, 8, 16, 32) if l <= (1 << k) // 2}
    assert any(p["indices"] != sorted(p["indices"]) for p in dump["plans"])       # rows in another order than the cosets


def test_planner_grids_cover_the_lanes_exactly(dump):
    grids = dump["grids"]
    assert [g["np"] for g in grids[:16]] == [2 << i for i in range(16)]
    for g in grids:
        np = g["np"]
        assert g["rc"] == OK
        for name, lanes in (("vanish", 2 * np), ("scatter", 2 * np), ("divide", 2 * np)):      # (the dump's domain is n = 2 n')
            got_lanes, grid, block, lds = g[name]
            assert got_lanes == lanes and block == krm.THREADS and grid * block >= lanes > (grid - 1) * block, (name, g)
            assert lds == (krm.TILE * 32 if name == "vanish" else 0)
        assert g["tiles"] == -(-g["m"] // krm.TILE)
    # n' = 2 (four lanes, one workgroup), 128 (2n' = one workgroup exactly), 256 (two), and the tile count around the tile
    by_np = {g["np"]: g for g in grids[:16]}
    assert by_np[2]["vanish"][:2] == [4, 1] and by_np[128]["vanish"][:2] == [256, 1] and by_np[256]["vanish"][:2] == [512, 2]
    assert by_np[65536]["vanish"][:2] == [131072, 512]
    assert [(g["m"], g["tiles"]) for g in grids[16:]] == [(0, 0), (1, 1), (255, 1), (256, 1), (257, 2)]


def test_planner_rules_at_their_edges(dump):
    rules = {x["rule"]: x for x in dump["rules"]}
    accepted = ["ok", "l=n/2", "count=n'", "len=kl", "index=n'-1", "np=2^16"]
    refused = ["count=0", "len=0", "l=0", "l=1", "l=3", "l=n", "count=n'+1", "len=kl+1", "index=n'", "repeat", "np=2^17"]
    assert sorted(accepted + refused) == sorted(k for k in rules if not k.startswith("order"))
    for k in accepted:
        assert rules[k]["rc"] == OK and rules[k]["message"] == "", k
    for k in refused:
        assert rules[k]["rc"] == ERR_ARG and rules[k]["message"].startswith("kzg: "), k
    assert "need 6 cells" in rules["len=kl+1"]["message"] and "at most 65536" in rules["np=2^17"]["message"]
    assert (rules["np=2^16"]["n"], rules["np=2^17"]["n"]) == (1 << 17, 1 << 18)
    # the order: the first rule that fails is the one reported
    assert "17 cells" in rules["order: count before index"]["message"]
    assert "coset 99" in rules["order: index before repeat"]["message"]
    assert "both coset 1" in rules["order: repeat before len"]["message"]
    assert "too few cells" in rules["order: len before np"]["message"]


SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_planner_under_address_and_undefined_sanitizers(dump):
    r = _run("san-recover-plan", ("tools", "san", "kzg_recover_plan_dump"), env=dict(os.environ, **SAN_ENV))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    assert lines == dump["plans"] + dump["grids"] + dump["rules"]


def test_host_recovery_under_address_and_undefined_sanitizers():
    """tools/san/kzg_recover_check.cpp: a program of its own around csrc/kzg_recover_host.h; every case it prints is held to the model"""
    r = _run("san-kzg-recover", ("tools", "san", "kzg_recover_check"), env=dict(os.environ, **SAN_ENV), words=())
    assert "KZG RECOVER CHECK OK" in r.stdout, r.stdout[-2500:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("R ")]
    assert len(lines) == 2 * 9 * 4
    verdicts = set()
    for ln in lines:
        head, idx, vals, co = (part.split() for part in ln.split(":"))
        abi, n, l, length, rc = (int(x) for x in head[1:])
        cv = [CURVES[c][0] for c in NAMES if CURVES[c][0].abi == abi][0]
        known = [int(x) for x in idx]
        flat = [int(x, 16) for x in vals]
        rows = [flat[i * l:(i + 1) * l] for i in range(len(known))]
        want = krm.recover(n, l, known, rows, length, cv.omega(n), cv.coset_shift, cv.r)
        assert (rc, [int(x, 16) for x in co]) == ((OK, want) if want is not None else (ERR_VERIFY, [])), head
        verdicts.add(rc)
    assert verdicts == {OK, ERR_VERIFY}


# ---- the exports ----------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "apk.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and ("int %s(" % name) in hdr
        assert getattr(lib, name).argtypes is not None, name
    assert _lib.ABI_VERSION == 5 and lib.apk_abi_version() == 5 and "#define APK_ABI_VERSION 5" in hdr          # additive


@pytest.mark.parametrize("cname", NAMES)
def test_argument_errors_come_before_the_device_and_write_nothing(cname):
    cv, _ = CURVES[cname]
    l, k = 4, 3
    rows = C.create_string_buffer(32 * l * k)
    mark = b"\xa5" * (32 * l * k)
    out = C.create_string_buffer(mark, len(mark))
    idx = (C.c_uint64 * k)(0, 1, 2)
    for fn in (lib.apk_kzg_recover_cosets, lib.apk_kzg_recover_cosets_device):
        for bad in ((l, k, None, rows, 8, out), (l, k, idx, None, 8, out), (l, k, idx, rows, 8, None), (l, 0, idx, rows, 8, out),
                    (l, k, idx, rows, 0, out), (0, k, idx, rows, 8, out), (1, k, idx, rows, 8, out), (3, k, idx, rows, 8, out), (6, k, idx, rows, 8, out)):
            assert fn(None, *bad) == ERR_ARG, bad[:2]
            assert lib.apk_last_error(), "an argument error carries a message"
    # everything but the context in order: the device is missed first where there is none
    want = ERR_HIP if _lib.device_count() == 0 else ERR_ARG
    for fn in (lib.apk_kzg_recover_cosets, lib.apk_kzg_recover_cosets_device):
        assert fn(None, l, k, idx, rows, 8, out) == want
    if want == ERR_HIP:
        assert b"no CPU fallback" in lib.apk_last_error()
    assert out.raw == mark


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------------
class _Key:
    def __init__(self, cv, n):
        self.curve, self.n = cv, n

    @property
    def ctx(self):
        raise AssertionError("the wrapper reached the library with bad arguments")


def test_python_wrappers_argument_errors():
    cv, _ = CURVES["bn254"]
    key = _Key(cv, 16)
    row = [1, 2, 3, 4]
    for fn in (ap_kzg.RecoverCosets, ap_kzg.RecoverCosetsAndProofs):
        for l in (0, 1, 3, 16):
            with pytest.raises(ValueError, match="coset size"):
                fn([0], [row], l, 1, key)
        with pytest.raises(ValueError, match="rows"):
            fn([], [], 4, 1, key)
        with pytest.raises(ValueError, match="rows"):
            fn([0, 1], [row], 4, 1, key)
        with pytest.raises(ValueError, match="values"):
            fn([0], [row[:3]], 4, 1, key)
        for length in (0, 5):
            with pytest.raises(ValueError, match="polynomial size"):
                fn([0], [row], 4, length, key)
    with pytest.raises(ValueError, match="PrepareCosets"):
        ap_kzg.RecoverCosetsAndProofs([0], [row], 4, 4, key)
    key.kzg_coset_size = 2
    with pytest.raises(ValueError, match="PrepareCosets"):
        ap_kzg.RecoverCosetsAndProofs([0], [row], 4, 4, key)
    # rows may be CosetOpeningProof entries; good arguments reach the library
    with pytest.raises(AssertionError, match="reached the library"):
        ap_kzg.RecoverCosets([3], [ap_kzg.CosetOpeningProof(cv.g1, row)], 4, 4, key)
    key.kzg_coset_size = 4
    with pytest.raises(AssertionError, match="reached the library"):
        ap_kzg.RecoverCosetsAndProofs([3], [row], 4, 4, key)

"""CPU tier of the FK20 openings' planner (algoplonk_amd/csrc/kzg_fk20_plan.h through tools/kzg_fk20_plan_dump): which SRS point
goes where in t, held to the big-integer models of both calls (tests/kzg_all_model.py, tests/kzg_cosets_model.py); the gather's
launches, run on an integer array with every launch's lanes unordered; the chunks of the small NTTs; the argument rules, held to a
Python restatement at their edges; and the dump tool once under ASAN + UBSAN.  No GPU."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

import kzg_all_model as kam
import kzg_cosets_model as kcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
OK, ERR_ARG = 0, 1          # include/apk.h
ARGS_MAX = 16               # csrc/ntt_plan.h NTT_ARGS_MAX
R, TAU = (1 << 61) - 1, 3   # a prime and a tau whose powers below 2^7 are distinct: the models take any modulus
WORDS = ["shape", "gather", "chunks", "rules"]
LOGS = range(3, 8)


def _run(target, path, env=None):
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, *path)] + WORDS, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r


@pytest.fixture(scope="module")
def dump():
    """the tool's lines, by word"""
    lines = [json.loads(x) for x in _run("fk20-plan-dump", ("tools", "kzg_fk20_plan_dump")).stdout.splitlines()]
    return {"shape": [x for x in lines if "t" in x], "gather": [x for x in lines if "m" in x], "chunks": [x for x in lines if "chunks" in x],
            "rules": [x for x in lines if "rule" in x]}


def _powers_of_two(lo, hi):
    return [1 << k for k in range(lo.bit_length() - 1, hi.bit_length()) if lo <= 1 << k <= hi]


# ---- the shape and the arrangement of t ----------------------------------------------------------------------------------------------
def test_shape_and_source_of_t_against_both_models(dump):
    assert [(s["log_n"], s["l"]) for s in dump["shape"]] == [(k, l) for k in LOGS for l in _powers_of_two(1, (1 << k) // 2)]
    for s in dump["shape"]:
        n, l, np = 1 << s["log_n"], s["l"], (1 << s["log_n"]) // s["l"]
        assert (s["n"], s["np"], s["pair"], s["sub_log"]) == (n, np, [2 * np, np], l.bit_length() - 1), s
        assert s["logs"] == [n.bit_length() - 1, l.bit_length() - 1, np.bit_length() - 1] and s["prepare_stages"] == (2 * np).bit_length() - 1, s
        src = s["t"]
        assert len(src) == 2 * n and all(-1 <= j <= n - l - 1 for j in src) and max(src) == n - l - 1, (n, l)
        t = [0 if j < 0 else pow(TAU, j, R) for j in src]
        f = [1] * n
        for c in range(l):
            assert t[c::l] == kcm.sequences(f, n, l, c, TAU, R)[1], (n, l, c)
            assert src[c::l].count(-1) == np + 1 and src[c::l][np - 1:] == [-1] * (np + 1), (n, l, c)
        if l == 1:
            assert t == kam.sequences(f, n, TAU, R)[1], n
        # every SRS point below n - l goes to exactly one position
        assert sorted(j for j in src if j >= 0) == list(range(n - l)), (n, l)


# ---- the gather ----------------------------------------------------------------------------------------------------------------------
def _bitrev(k, bits):
    return int(format(k, "0%db" % bits)[::-1], 2) if bits else 0


def test_gather_launches_on_an_integer_array(dump):
    assert [g["m"] for g in dump["gather"]] == _powers_of_two(2, 1 << 16)
    for g in dump["gather"]:
        m, launches = g["m"], [tuple(x) for x in g["launches"]]
        bits = m.bit_length() - 1
        # the ranges tile [0, m) once, in order
        assert launches[0][0] == 0 and launches[-1][1] == m and all(a[1] == b[0] for a, b in zip(launches, launches[1:])), g
        assert all(k0 < k1 for k0, k1 in launches), g
        if m >= 8:
            assert launches == [(0, 2), (2, m)], g
        orig = [1000 + i for i in range(2 * m)]       # c, natural order; 0 stands for infinity
        work = list(orig)
        for k0, k1 in launches:
            lanes = range(k0, k1)
            reads = {k: k + m - 2 for k in lanes if k != m - 1}
            writes = {k: _bitrev(k, bits) for k in lanes}
            assert len(set(writes.values())) == len(writes), g
            # unordered lanes: no lane writes what ANOTHER lane of the launch reads (m = 2: lane 0 reads and writes element 0)
            reader = {pos: k for k, pos in reads.items()}
            clash = [(a, reader[wa]) for a, wa in writes.items() if reader.get(wa, a) != a]
            assert not clash, (g, clash)
            if m != 2:
                assert not set(writes.values()) & set(reads.values()), g
            before = list(work)
            for k in lanes:
                work[writes[k]] = 0 if k == m - 1 else before[reads[k]]
        assert work[:m] == [0 if k == m - 1 else orig[k + m - 2] for k in (_bitrev(j, bits) for j in range(m))], g


# ---- the chunks of the small NTTs ------------------------------------------------------------------------------------------------------
def test_chunks_cover_both_parities_in_order(dump):
    assert [c["l"] for c in dump["chunks"]] == _powers_of_two(2, 1 << 10)
    for c in dump["chunks"]:
        l, chunks = c["l"], [tuple(x) for x in c["chunks"]]
        assert c["args_max"] == ARGS_MAX
        assert [x[0] for x in chunks] == sorted(x[0] for x in chunks), c       # all even chunks before the odd ones
        for odd in (0, 1):
            mine = [x for x in chunks if x[0] == odd]
            assert all(1 <= cnt <= ARGS_MAX for _, _, cnt in mine), c
            assert [c0 for _, c0, _ in mine] == sorted(c0 for _, c0, _ in mine), c
            assert [k for _, c0, cnt in mine for k in range(c0, c0 + cnt)] == list(range(l)), c
        # today's order: for odd in (0, 1): for c0 in 0, ARGS_MAX ..: (odd, c0, min(l - c0, ARGS_MAX))
        assert chunks == [(odd, c0, min(l - c0, ARGS_MAX)) for odd in (0, 1) for c0 in range(0, l, ARGS_MAX)], c


# ---- the argument rules ----------------------------------------------------------------------------------------------------------------
def _size_rule(n, l):
    return OK if l >= 2 and l & (l - 1) == 0 and l <= n // 2 else ERR_ARG


def test_argument_rules_at_their_edges(dump):
    rules = dump["rules"]
    by = {(x["rule"], x["n"], x["l"], x["x"]): x for x in rules}      # (edges that coincide, as n - l and n - 1 at l = 1, are printed twice)
    for k in LOGS:
        n = 1 << k
        for l in range(0, n + 2):
            x = by["size", n, l, 0]
            assert x["rc"] == _size_rule(n, l), x
            assert (x["message"] == "") == (x["rc"] == OK), x
            if x["rc"] != OK:
                assert x["message"] == "kzg: cosets of %d points in a domain of %d (a power of two, 2..n/2)" % (l, n), x
        for l in (1, 3, n // 2, n):
            assert by["size", n, l, 0]["rc"] == (OK if l == n // 2 else ERR_ARG)
        for l in _powers_of_two(1, n // 2):
            for count in {n - l - 2, n - l - 1, n - l, n - l + 1, n - 2, n - 1}:
                x = by["srs", n, l, count]
                assert x["rc"] == (OK if count >= n - l else ERR_ARG), x
                if x["rc"] != OK and l == 1:
                    assert x["message"] == "kzg: %d SRS points, the openings at every point need %d" % (count, n - 1), x
                if x["rc"] != OK and l > 1:
                    assert x["message"] == "kzg: %d SRS points, the openings on cosets of %d points need %d" % (count, l, n - l), x
            assert by["srs", n, l, n - l - 1]["rc"] == ERR_ARG and by["srs", n, l, n - l]["rc"] == OK
            for length in {0, 1, l, l + 1, n, n + 1}:
                x = by["len", n, l, length]
                assert x["rc"] == (OK if 1 <= length <= n else ERR_ARG), x
                assert x["has_quotient"] == (1 if length > l else 0), x
                if x["rc"] != OK:
                    what = "at every point" if l == 1 else "on every coset"
                    assert x["message"] == "kzg: %d coefficients, the openings %s take 1..%d" % (length, what, n), x
            assert by["len", n, l, l]["has_quotient"] == 0 and by["len", n, l, l + 1]["has_quotient"] == 1
    assert by["srs", 8, 1, 6]["rc"] == ERR_ARG and by["srs", 8, 1, 7]["rc"] == OK          # the whole domain: n - 2 and n - 1


# ---- the same program under ASAN + UBSAN -------------------------------------------------------------------------------------------------
def test_planner_under_address_and_undefined_sanitizers(dump):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = _run("san-fk20-plan", ("tools", "san", "kzg_fk20_plan_dump"), env)
    assert r.stderr == "", r.stderr[-3000:]
    assert len(r.stdout.splitlines()) == sum(len(v) for v in dump.values())

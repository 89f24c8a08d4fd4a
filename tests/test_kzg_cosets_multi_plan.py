"""CPU tier of the batched coset openings' planner (algoplonk_amd/csrc/kzg_fk20_plan.h "MANY polynomials", through the word `multi`
of tools/kzg_fk20_plan_dump): the groups of a call, the chunks of the small transforms over G l rows, the scratch sizes and the
grids, each held to a Python restatement; the LAYOUT, held to the big-integer model of the single call (tests/kzg_cosets_model.py):
three polynomials of different lengths side by side in arrays that are indexed through the dumped positions ONLY, once with
per-block transforms and once with a stage loop over the whole array (no butterfly crosses a block); the argument rules at their
edges and in their order; and the dump tool with the new word under ASAN + UBSAN.  No GPU."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

import kzg_all_model as kam
import kzg_cosets_model as kcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
OK, ERR_ARG, ERR_STATE = 0, 1, 3      # include/apk.h
ARGS_MAX, MULTI_MAX = 16, 64          # csrc/ntt_plan.h NTT_ARGS_MAX, include/apk.h APK_KZG_COSETS_MULTI_MAX
# a prime with 2^32 | p - 1 (the models take any modulus with the roots of unity they need), a generator of its units, a tau
P = (1 << 64) - (1 << 32) + 1
GEN, TAU = 7, 0x1234567890ABCDEF % P


def _run(target, path, env=None):
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, *path), "multi"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r


@pytest.fixture(scope="module")
def dump():
    """the lines of the word `multi`, by kind"""
    lines = [json.loads(x) for x in _run("fk20-plan-dump", ("tools", "kzg_fk20_plan_dump")).stdout.splitlines()]
    assert all("multi" in x for x in lines)
    kinds = {}
    for x in lines:
        kinds.setdefault(x["multi"], []).append(x)
    assert sorted(kinds) == ["check", "chunks", "groups", "layout", "not_device", "sizes"]
    return kinds


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- the groups ------------------------------------------------------------------------------------------------------------------------
def test_groups_of_every_count(dump):
    assert [g["count"] for g in dump["groups"]] == list(range(1, MULTI_MAX + 1))
    for g in dump["groups"]:
        count, groups = g["count"], [tuple(x) for x in g["groups"]]
        assert (g["max"], g["group_max"]) == (MULTI_MAX, ARGS_MAX)
        sizes = [s for _, s in groups]
        assert len(groups) == _cdiv(count, ARGS_MAX) and sum(sizes) == count, g
        assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True) and max(sizes) <= ARGS_MAX and min(sizes) >= 1, g
        # the groups tile 0 .. count - 1 in call order
        assert [b0 for b0, _ in groups] == [sum(sizes[:k]) for k in range(len(sizes))], g
    by = {g["count"]: [s for _, s in g["groups"]] for g in dump["groups"]}
    assert by[17] == [9, 8] and by[16] == [16] and by[33] == [11, 11, 11] and by[64] == [16] * 4


# ---- the chunks of the small transforms over G l rows -------------------------------------------------------------------------------------
def test_chunks_cover_the_rows_of_each_parity_once(dump):
    assert [(c["l"], c["G"]) for c in dump["chunks"]] == [(l, G) for l in (2, 16, 64) for G in (1, 3, 16)]
    for c in dump["chunks"]:
        rows, chunks = c["rows"], [tuple(x) for x in c["chunks"]]
        assert rows == c["G"] * c["l"] and c["args_max"] == ARGS_MAX
        assert [x[0] for x in chunks] == sorted(x[0] for x in chunks), c      # the even halves, then the odd halves
        for odd in (0, 1):
            mine = [x for x in chunks if x[0] == odd]
            assert all(1 <= cnt <= ARGS_MAX for _, _, cnt in mine), c
            assert [k for _, c0, cnt in mine for k in range(c0, c0 + cnt)] == list(range(rows)), c
            assert len(mine) == _cdiv(rows, ARGS_MAX), c


# ---- scratch and grids --------------------------------------------------------------------------------------------------------------------
def test_scratch_sizes_and_grids(dump):
    seen = set()
    for s in dump["sizes"]:
        n, l, G = 1 << s["log_n"], s["l"], s["G"]
        np = n // l
        seen.add(np)
        assert s["np"] == np
        assert (s["points"], s["scalars"], s["upload"]) == (3 * G * np, 5 * G * n, G * n), s
        assert (s["big_points"], s["small_points"]) == (G * 2 * np, G * np), s
        assert s["grid_scalars"] == _cdiv(G * n, 256), s
        log_group = min(l.bit_length() - 1 + 2, 6)
        assert s["log_group"] == log_group and s["grid_pointwise"] == [_cdiv(2 * np, 64 >> log_group), G], s
        # a lane per butterfly of a stage over 2 G n' points, per point of the gather and the finish; half as many in the small stages
        assert s["grid_points"] == _cdiv(G * np, 128) and s["grid_small_stage"] == _cdiv(G * np // 2, 128), s
    assert {2, 4, 64, 2048} <= seen
    # the two flagship contexts at G = 16, l = 64, in bytes: XYZZ points of 4 x 32 (BN254) and 4 x 48 (BLS12-381) bytes, scalars of 32
    by = {(s["log_n"], s["l"], s["G"]): s for s in dump["sizes"]}
    bn, bls = by[17, 64, 16], by[14, 64, 16]
    assert (bn["points"] * 128, (bn["scalars"] + bn["upload"]) * 32) == (12 << 20, 384 << 20)
    assert (bls["points"] * 192, (bls["scalars"] + bls["upload"]) * 32) == (9 << 18, 48 << 20)


# ---- the layout, held to the model ----------------------------------------------------------------------------------------------------------
def _bitrev(k, bits):
    return int(format(k, "0%db" % bits)[::-1], 2) if bits else 0


def _stages(arr, block, w_block, inverse):
    """Decimation-in-time stages over the WHOLE array - the lanes of kzg_all_stage_glv_kernel / lagrange_stage_kernel: butterfly bf
    pairs (i0, i0 + 2^t) with i0 = ((bf >> t) << (t + 1)) | low, low = bf mod 2^t, twiddle w_block^(+-(low << (log block - 1 - t))).
    `block`: the size of one transform (bit-reversed in, natural out); len(arr) is any multiple of it."""
    logb = block.bit_length() - 1
    w = pow(w_block, -1, P) if inverse else w_block
    for t in range(logb):
        for bf in range(len(arr) // 2):
            low = bf & ((1 << t) - 1)
            i0 = ((bf >> t) << (t + 1)) | low
            i1 = i0 | (1 << t)
            v = arr[i1] * pow(w, low << (logb - 1 - t), P) % P
            arr[i0], arr[i1] = (arr[i0] + v) % P, (arr[i0] - v) % P


@pytest.mark.parametrize("whole_array", [False, True], ids=["per-block", "whole-array-stages"])
def test_layout_against_the_model(dump, whole_array):
    assert [(x["n"], x["l"], x["G"]) for x in dump["layout"]] == [(8, 2, 3), (8, 4, 3), (64, 8, 3)]
    for L in dump["layout"]:
        n, l, G = L["n"], L["l"], L["G"]
        np, np2 = n // l, 2 * n // l
        w_2n = pow(GEN, (P - 1) // (2 * n), P)
        w, w_2np = w_2n * w_2n % P, pow(w_2n, l, P)
        assert L["skips_infinity_rows"] == 0
        # three polynomials of different lengths: full, not longer than l (every H infinity), in between - the short one in the MIDDLE
        lens = [n, l, n // 2 + 1]
        fs = [[(b * 1000003 + 7919 * k * k + 12345) % P for k in range(lens[b])] for b in range(G)]
        # every position is in range and used once
        for key, size in (("work_hat", G * np2), ("work_cc", G * np2), ("second", G * np), ("result", G * np), ("by_coset", G * n)):
            flat = [p for blk in L[key] for p in blk]
            assert sorted(flat) == list(range(size)), (n, l, key)
        assert L["value0"] == [b * n for b in range(G)] and [r for blk in L["row"] for r in blk] == list(range(G * l))
        # the values, coset-major, through by_coset
        vals = [None] * (G * n)
        for b in range(G):
            v = [kam.horner(fs[b], pow(w, k, P), P) for k in range(n)]
            for i in range(np):
                for j in range(l):
                    vals[L["by_coset"][b][i * l + j]] = v[i + np * j]
            assert [vals[b * n + k] for k in range(n)] == kcm.values_by_coset(fs[b], n, l, w, P)      # out_values[b n + i l + j]
        # step (3): the rows a_(b,c), A^ by two size-n' transforms, the pointwise sums over the SAME T^_c, to the bit-reversed block positions
        t_hat = [kcm.t_hat(n, l, c, w_2n, TAU, P) for c in range(l)]
        rows = [0] * (G * n)
        for b in range(G):
            f = kam.padded(fs[b], n)
            for c in range(l):
                for u in range(np - 1):
                    rows[L["row"][b][c] * np + u] = f[c + l * (u + 1)]
        assert not any(rows[L["row"][1][c] * np + u] for c in range(l) for u in range(np))      # len <= l: all-zero scalars
        scale = pow(np2, -1, P)
        work = [None] * (G * np2)
        for b in range(G):
            acc = [0] * np2
            for c in range(l):
                a = rows[L["row"][b][c] * np:(L["row"][b][c] + 1) * np]
                even = kam.dft(a, w_2np * w_2np % P, P)
                odd = kam.dft([x * pow(w_2np, u, P) % P for u, x in enumerate(a)], w_2np * w_2np % P, P)
                assert (even, odd) == kcm.a_hat_split(fs[b], n, l, c, w_2n, P)
                for i in range(np2):
                    a_hat = (odd if i & 1 else even)[i >> 1]
                    acc[i] = (acc[i] + a_hat * t_hat[c][i]) % P
            for i in range(np2):
                work[L["work_hat"][b][i]] = acc[i] * scale % P      # (the 1 / 2n' rides in A^)
        assert None not in work
        # the inverse transform: cc_b[k] at work_cc[b][k]
        if whole_array:
            _stages(work, np2, w_2np, True)
        else:
            for b in range(G):
                cc = kam.dft([work[L["work_hat"][b][i]] for i in range(np2)], pow(w_2np, -1, P), P)
                for k in range(np2):
                    work[L["work_cc"][b][k]] = cc[k]
        # the gather, out of place, through the dumped sources and destinations
        second = [None] * (G * np)
        for b in range(G):
            for k in range(np):
                src = L["gather_source"][b][k]
                assert (src == -1) == (k == np - 1)
                second[L["second"][b][k]] = 0 if src < 0 else work[src]
            assert [second[L["second"][b][m]] for m in range(np)] == kcm.h_terms(fs[b], n, l, TAU, P), (n, l, b)
        assert None not in second
        # the forward transform: H_(b,i) at result[b][i]
        if whole_array:
            _stages(second, np, w_2np * w_2np % P, False)
        else:
            for b in range(G):
                h = kam.dft([second[L["second"][b][m]] for m in range(np)], w_2np * w_2np % P, P)
                for i in range(np):
                    second[L["result"][b][i]] = h[i]      # (block b's own positions: the blocks after it are still unread)
        for b in range(G):
            got = [second[L["result"][b][i]] for i in range(np)]
            assert got == kcm.direct(fs[b], n, l, w, TAU, P), (n, l, b)
            assert (not any(got)) == (b == 1), (n, l, b)      # the infinity block stays one and does not leak


def test_whole_array_stages_are_the_per_block_transforms():
    """A self-check of this file's own helper, NOT coverage of the planner (it runs none of the repository's code and passes without
    the feature): the stage loop `_stages`, which test_layout_against_the_model relies on, against the plain sums, at block sizes
    2 .. 16 and a G that is no power of two."""
    for block in (2, 4, 8, 16):
        bits = block.bit_length() - 1
        wb = pow(GEN, (P - 1) // block, P)
        for G in (1, 3, 5):
            nat = [[(b * 31 + k * k + 5) % P for k in range(block)] for b in range(G)]
            for inverse in (False, True):
                arr = [nat[b][_bitrev(i, bits)] for b in range(G) for i in range(block)]
                _stages(arr, block, wb, inverse)
                want = [x for b in range(G) for x in kam.dft(nat[b], pow(wb, -1, P) if inverse else wb, P)]
                assert arr == want, (block, G, inverse)


# ---- the argument rules: their edges and their order --------------------------------------------------------------------------------------
def _verdict(x):
    """the Python restatement: (rc, message) of the FIRST rule that refuses"""
    n, count = x["n"], x["count"]
    if x["msm_only"]:
        return ERR_STATE, "MSM-only context has no NTT domain"
    if not x["prepared"]:
        return ERR_STATE, "kzg: apk_kzg_cosets_prepare has not run on this context"
    if count == 0 or count > MULTI_MAX:
        return ERR_ARG, "kzg: %d polynomials on every coset (1..%d)" % (count, MULTI_MAX)
    if x["null"] in ("polys", "lens", "out_h"):
        return ERR_ARG, "null argument"
    if x["null"] in ("first", "last"):
        return ERR_ARG, "kzg: polynomial %d is null" % (0 if x["null"] == "first" else count - 1)
    if x["bad_row"] >= 0 and not 1 <= x["len"] <= n:
        return ERR_ARG, "polynomial %d: kzg: %d coefficients, the openings on every coset take 1..%d" % (x["bad_row"], x["len"], n)
    return OK, ""


def test_argument_rules_in_their_order(dump):
    checks = dump["check"]
    for x in checks:
        assert (x["rc"], x["message"]) == _verdict(x), x
    by = {(x["msm_only"], x["prepared"], x["count"], x["null"], x["bad_row"], x["len"]): x for x in checks}
    # the edges: count 0, 64, 65; len 0, 1, n, n + 1 in the first and in the last row
    assert by[0, 1, 0, "", -1, 3]["rc"] == ERR_ARG and by[0, 1, 64, "", -1, 3]["rc"] == OK and by[0, 1, 65, "", -1, 3]["rc"] == ERR_ARG
    assert by[0, 1, 1, "", -1, 3]["rc"] == OK
    for count in (1, 2, 64):
        for row in (0, count - 1):
            assert [by[0, 1, count, "", row, length]["rc"] for length in (0, 1, 8, 9)] == [ERR_ARG, OK, OK, ERR_ARG], (count, row)
            assert by[0, 1, count, "", row, 9]["message"].startswith("polynomial %d: " % row)
    # the order: state before count before null before length
    assert by[1, 0, 0, "polys", 0, 0]["message"] == "MSM-only context has no NTT domain"
    assert by[0, 0, 65, "polys", 0, 0]["message"].endswith("has not run on this context")
    assert by[0, 1, 65, "polys", 0, 0]["message"].startswith("kzg: 65 polynomials")
    assert by[0, 1, 2, "last", 0, 0]["message"] == "kzg: polynomial 1 is null"
    assert by[0, 1, 2, "lens", 1, 9]["message"] == "null argument"
    assert [(x["row"], x["rc"], x["message"]) for x in dump["not_device"]] == [(0, ERR_ARG, "kzg: polynomial 0 is not device memory"),
                                                                            (63, ERR_ARG, "kzg: polynomial 63 is not device memory")]


# ---- the same program with the new word under ASAN + UBSAN -----------------------------------------------------------------------------------
def test_planner_with_the_new_word_under_address_and_undefined_sanitizers(dump):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = _run("san-fk20-plan", ("tools", "san", "kzg_fk20_plan_dump"), env)
    assert r.stderr == "", r.stderr[-3000:]
    assert len(r.stdout.splitlines()) == sum(len(v) for v in dump.values())

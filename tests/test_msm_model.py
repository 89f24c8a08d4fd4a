"""CPU tier: the plain-integer model of the MSM's signed-digit recoding and window planner (tests/msm_model.py), held to its own
definitions and - the planner - to the C++ it restates (algoplonk_amd/csrc/msm_plan.h through tools/msm_plan_dump), so that the
GPU tests built on it (tests/test_gpu_msm_edges.py) cannot pass vacuously."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

import msm_model as mm
from helpers import CURVES

WINDOWS = list(range(7, 21))


@pytest.mark.parametrize("cname", list(CURVES))
def test_bits_match_the_field_parameters(cname):
    cv, _ = CURVES[cname]
    assert mm.curve_bits(cname) == cv.r.bit_length()


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("cname", list(CURVES))
def test_layout_spreads_the_bits_wider_windows_first(cname, c):
    bits = mm.curve_bits(cname)
    lay = mm.layout(bits, c)
    assert lay.W == -(-(bits + 1) // c) and lay.W <= mm.MSM_MAX_WINDOWS
    assert lay.off[0] == 0 and lay.off[-1] == bits + 1
    assert all(lay.off[j + 1] - lay.off[j] == lay.width[j] for j in range(lay.W))
    assert max(lay.width) <= c and max(lay.width) - min(lay.width) <= 1
    assert list(lay.width) == sorted(lay.width, reverse=True)


@pytest.mark.parametrize("domain", ["raw", "canonical"])
@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("cname", list(CURVES))
def test_edge_words_recode_exactly_and_reach_every_reachable_edge(cname, c, domain):
    cv, _ = CURVES[cname]
    r, bits = cv.r, mm.curve_bits(cname)
    lay = mm.layout(bits, c)
    es = mm.edge_scalars(r, lay, domain)
    assert len(es.values) == len(es.labels) == len(set(es.values))
    assert all(0 <= m < r for m in es.values), "a family value is >= r"
    hit = [set() for _ in range(lay.W)]
    for m in es.values:
        d = mm.recode(m, lay)
        # the recoding is exact and balanced: sum d_j 2^off_j == m, |d_j| <= 2^(w_j - 1)
        assert sum(dj << lay.off[j] for j, dj in enumerate(d)) == m, (m, d)
        assert all(abs(dj) <= 1 << (lay.width[j] - 1) for j, dj in enumerate(d)), (m, d)
        for j, ks in enumerate(mm.window_kinds(m, lay)):
            hit[j] |= ks
    # every (window, kind) is hit, or listed as skipped - and only when no word below r reaches it
    listed = set(es.skipped)
    for j in range(lay.W):
        w, prev = lay.width[j], lay.width[j - 1] if j else 0
        for k in mm.EDGE_KINDS:
            v = mm.edge_value(k, w)
            cands = []
            if v < 1 << w:
                cands.append(v << lay.off[j])                                                     # carry-in 0
            if j and v >= 1:
                cands.append(((v - 1) << lay.off[j]) + (((1 << (prev - 1)) + 1) << lay.off[j - 1]))   # the least carry-in
            reachable = any(m < r for m in cands)
            skip = [s for s in listed if s.startswith("window %d: %s (" % (j, k))]
            if reachable:
                assert k in hit[j], ("window %d misses edge %s" % (j, k), es.skipped)
                assert not skip, skip
            else:
                assert k not in hit[j] and len(skip) == 1, (j, k, es.skipped)
    # the edges the issue names, in the windows below the top one: half stays positive, half + 1 turns negative and carries,
    # an all-ones field plus a carry is digit 0 carry 1
    for j in range(1, lay.W - 1):
        assert {"half", "half+1", "2^w"} <= hit[j]
    # the top window takes the largest field below r
    top = max((m >> lay.off[-2]) for m in es.values)
    assert top == (r - 1) >> lay.off[-2]


def test_recode_examples_by_hand():
    lay = mm.layout(254, 16)                                  # BN254 at c = 16: 16 windows, 15 of 16 bits and one of 15
    assert lay.W == 16 and lay.width[:2] == (16, 16) and lay.width[-1] == 15
    assert mm.recode(1 << 15, lay)[:2] == [1 << 15, 0]                       # half stays positive
    assert mm.recode((1 << 15) + 1, lay)[:2] == [-((1 << 15) - 1), 1]        # half + 1: negative, carry
    assert mm.recode((1 << 32) - 1, lay)[:3] == [-1, 0, 1]                   # all ones + carry: digit 0, carry 1
    es = mm.edge_scalars(CURVES["bn254"][0].r, lay, "raw")
    assert any(s.startswith("window 0: 2^w (") for s in es.skipped)          # window 0 has no carry-in


# the sizes where the planner's limits bind (MSM-only contexts: log_size = ceil(log2(count)))
PLANS = [("bn254", 1 << 18, 17, 256), ("bn254", 1 << 20, 19, 2048), ("bn254", 1 << 21, 19, 4096), ("bn254", (1 << 21) + 3, 18, 2048),
         ("bn254", 1 << 22, 18, 4096), ("bn254", 1 << 23, 18, 8192), ("bn254", 1 << 24, 16, 8192),
         ("bls12-381", 1 << 20, 19, 2048), ("bls12-381", 1 << 21, 19, 4096), ("bls12-381", (1 << 21) + 3, 18, 2048),
         ("bls12-381", 1 << 22, 18, 4096), ("bls12-381", 1 << 23, 18, 8192), ("bls12-381", 1 << 18, 15, None)]


@pytest.mark.parametrize("cname,count,c,P", PLANS)
def test_default_window_at_the_planner_limits(cname, count, c, P):
    lg = mm.msm_only_log_size(count)
    assert mm.default_window(cname, lg, bases=count) == c
    p = mm.plan(mm.curve_bits(cname), mm.CURVE_PARAMS[cname][1], 0, lg, count)
    if P is not None:
        assert p.P == P
    assert p.idx_bits + p.pb_log <= 31 and (p.P == 0 or p.P <= mm.MSM_PART_MAX)
    if count == 1 << 24:
        # 2^24: 18 bits fail (16 384 partitions), 16 bits take 8 192 partitions of 4 buckets; the first level's slices shrink to
        # fit the stage beside 2 x 8 192 cursors
        assert p.pb_log == 2 and mm.part_stage_max(p.P) == 24512
        assert mm.sort_form(p, count, count) in ("fused", "four-launch")


def test_proving_contexts_pass_log_n():
    # a proving context at n = 2^k has n + 3 bases and log_size = k: BN254 2^18 / 2^19 take the packed 17-bit counters,
    # BLS12-381 does not; 2^20 takes 19 bits
    assert mm.default_window("bn254", 18) == 17 and mm.default_window("bn254", 19) == 17
    assert mm.default_window("bls12-381", 18) == 15
    assert mm.default_window("bn254", 20) == 19 and mm.default_window("bls12-381", 14) == 12
    assert mm.default_window("bn254", 17) == 15 and mm.default_window("bn254", 17, slots=16) == 17


def test_refusals():
    bits, fp = mm.curve_bits("bn254"), 8
    mm.plan(bits, fp, 17, 20, 786432)                                         # the packed-counter limit itself
    with pytest.raises(mm.PlanError, match="at most 786432"):
        mm.plan(bits, fp, 17, 20, 786433)
    with pytest.raises(mm.PlanError, match="leave no room for the partition bits"):
        mm.plan(bits, fp, 19, 23, 1 << 23)                                    # 19 bits at 2^23: 16 384 partitions
    with pytest.raises(mm.PlanError):
        mm.plan(bits, fp, 21, 10, 1024)


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("cname", list(CURVES))
def test_the_digit_matrix_sizes_take_the_forms_the_gpu_tests_assert(cname, c):
    """n = 2^11 with a Lagrange SRS (2 051 bases): the default sort is one level up to 17 bits and two levels above.  Forced two
    levels, every window takes them except c = 8..10, whose fewer than four partitions leave the one-level sort; the fused form
    runs at some length for c = 7 and 11..17 (c >= 18: the runs per partition are too short for it)."""
    p = mm.plan(mm.curve_bits(cname), mm.CURVE_PARAMS[cname][1], c, 11, (1 << 11) + 3)
    lengths = (2051, 2049, 2048, 65, 2, 1)
    forms = {mm.sort_form(p, 2051, L) for L in lengths}
    assert forms == ({"one-level"} if c <= 17 else {"four-launch"}), forms
    assert (p.P >= 4) == (c not in (8, 9, 10)), p
    four = {mm.sort_form(p, 2051, L, sort2_env=1, fused_env=0) for L in lengths}
    assert four == ({"one-level"} if p.P < 4 else {"four-launch"}), four
    fused = {mm.sort_form(p, 2051, L, sort2_env=1) for L in lengths}
    assert ("fused" in fused) == (c == 7 or 11 <= c <= 17), fused


# ---- the model against the C++ planner --------------------------------------------------------------------------------------
GRID_BASES = [1 << 11, 2051, (1 << 13) + 3, (1 << 14) + 3, 1 << 16, (1 << 16) + 3, (1 << 17) + 3, 786432, 786433, (1 << 20) + 3,
              (1 << 21) + 3, (1 << 22) + 3, 1 << 24]
GRID_KNOBS = [(-1, 1), (1, 1), (1, 0)]          # (APK_MSM_SORT2, APK_MSM_SORT_FUSED)


def _grid():
    for cname in CURVES:
        for c in [0] + WINDOWS:
            for bases in GRID_BASES:
                for slots in (1, 16):
                    for maxlen in (1, 2049, bases):
                        for batch in (1, 4):
                            for sort2, fused in GRID_KNOBS:
                                yield cname, c, bases, slots, maxlen, batch, sort2, fused


def test_the_model_agrees_with_the_cpp_planner():
    """msm_plan.h decides in C++ what msm_model.py restates: the context's plan (msm_plan_context) and the sort a batch takes
    (msm_plan_batch), on the workspace msm_plan_workspace sizes and with no other proof in flight - the model's assumptions.
    One process of tools/msm_plan_dump answers the whole grid."""
    r = subprocess.run(["make", "-C", mm.CSRC, "msm-plan-dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = list(_grid())
    lines = []
    for cname, c, bases, slots, maxlen, batch, sort2, fused in cases:
        head = (mm.curve_bits(cname), mm.CURVE_PARAMS[cname][1], bases, mm.msm_only_log_size(bases), slots, c, sort2, fused, mm.SLICE)
        lines.append(" ".join(str(v) for v in head + (maxlen,) * batch))
    r = subprocess.run([os.path.join(mm.ROOT, "tools", "msm_plan_dump")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(out) == len(cases)
    refused = forms = 0
    for case, got in zip(cases, out):
        cname, c, bases, slots, maxlen, batch, sort2, fused = case
        bits, fp, lg = mm.curve_bits(cname), mm.CURVE_PARAMS[cname][1], mm.msm_only_log_size(bases)
        ctx = got["ctx"]
        try:
            p = mm.plan(bits, fp, c, lg, bases, slots)
        except mm.PlanError:
            assert ctx["rc"] == 1 and ctx["message"] and got["batch"] is None, (case, got)     # APK_ERR_ARG
            refused += 1
            continue
        assert ctx["rc"] == 0, (case, ctx)
        if c == 0:
            assert mm.default_window(cname, lg, slots, bases) == ctx["c"], (case, ctx)
        # (the packed entry's index bits mean nothing without partitions: the C++ leaves the whole layout zero, the model pb_log)
        assert (p.c, p.lay.W, list(p.lay.width), p.nb, p.idx_bits if p.P else 0, p.pb_log, p.P) == \
               (ctx["c"], ctx["W"], ctx["width"], ctx["NB"], ctx["idx_bits"], ctx["pb_log"], ctx["P"]), (case, p, ctx)
        b = got["batch"]
        if maxlen > bases:      # (2 049 scalars over 2^11 bases: refused before any plan; the model has no such call)
            assert b["rc"] == 1 and "exceed" in b["message"], (case, b)
            refused += 1
            continue
        try:
            form = mm.sort_form(p, bases, maxlen, batch, sort2_env=sort2, fused_env=fused)
        except mm.PlanError:
            assert b["rc"] == 3 and b["message"], (case, b)                                  # APK_ERR_STATE
            refused += 1
            continue
        assert b["rc"] == 0 and b["sort"] == form, (case, form, b)
        forms += 1
    assert refused and forms > len(cases) // 2        # both sides of the comparison happened

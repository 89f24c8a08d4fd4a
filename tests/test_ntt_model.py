"""CPU tier: the plain-integer model of the NTT's plan (tests/ntt_model.py), held to the C++ planner it restates
(algoplonk_amd/csrc/ntt_plan.h through tools/ntt_plan_dump), to the stage ranges the rule gave before it had a header of its own,
and to the invariants the pass kernel relies on - so that what a transform of any size takes can be read, and pinned, without a GPU."""
from __future__ import annotations

import itertools
import json
import os
import subprocess

import pytest

import ntt_model as nm

LOG_NS = range(1, 30)
TILE_KNOBS = (0, 4, 9, 10, 11)
STAGES_KNOBS = (0, 1, 3, 7, 9, 11)
RADIX4_KNOBS = (-1, 0, 1)
THREADS_KNOBS = (0, 64, 128)


def _grid():
    return list(itertools.product(LOG_NS, TILE_KNOBS, STAGES_KNOBS, RADIX4_KNOBS, THREADS_KNOBS, (0, 1), (0, 1), (0, 1)))


def _dump(lines):
    """one process of tools/ntt_plan_dump answers all the lines"""
    r = subprocess.run(["make", "-C", nm.CSRC, "ntt-plan-dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(nm.ROOT, "tools", "ntt_plan_dump")], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def grid_plans():
    """(case, the planner's answer) over the full grid, count = 3"""
    cases = _grid()
    lines = ["%d 3 %d %d %d %d %d %d %d" % c for c in cases]
    return list(zip(cases, _dump(lines)))


def test_the_model_agrees_with_the_cpp_planner(grid_plans):
    accepted = refused = 0
    for case, got in grid_plans:
        log_n, tile, stages, r4, thr, loaded, foreign, wide = case
        try:
            p = nm.plan(log_n, 3, tile_knob=tile, stages_knob=stages, radix4_knob=r4, threads_knob=thr, loaded=bool(loaded),
                        loaded_foreign=bool(foreign), have_wide=bool(wide))
        except nm.PlanError as e:
            assert (got["rc"], got["message"]) == (e.rc, e.message), (case, got)
            refused += 1
            continue
        assert got["rc"] == nm.APK_OK and got["message"] == "", (case, got)
        want = [[q.t0, q.t1, int(q.first), int(q.last), int(q.radix4)] for q in p.passes]
        assert (got["tile_log"], got["passes"], got["grid_x"], got["threads"], got["lds_bytes"], bool(got["needs_wide"]), got["paths"]) == \
               (p.tile_log, want, p.grid_x, p.threads, p.lds_bytes, p.needs_wide, p.paths), (case, p, got)
        accepted += 1
    assert refused and accepted > len(grid_plans) // 2        # both sides of the comparison happened


def test_invariants_on_every_accepted_plan(grid_plans):
    seen = 0
    for case, got in grid_plans:
        if got["rc"] != nm.APK_OK:
            continue
        log_n = case[0]
        ps, tile_log = got["passes"], got["tile_log"]
        # the passes partition [0, log_n)
        assert ps[0][0] == 0 and ps[-1][1] == log_n, (case, got)
        assert all(a[1] == b[0] for a, b in zip(ps, ps[1:])), (case, got)
        # a pass runs its stages out of one tile, and the tile fits the transform and the LDS a launch may ask for
        assert all(1 <= t1 - t0 <= tile_log for t0, t1, *_ in ps), (case, got)
        assert tile_log <= min(log_n, nm.NTT_TILE_LOG), (case, got)
        assert got["threads"] > 0 and got["threads"] % 64 == 0 and got["threads"] <= nm.NTT_THREADS, (case, got)
        assert got["lds_bytes"] <= (1 << nm.NTT_TILE_LOG) * 36, (case, got)
        assert bool(got["needs_wide"]) == (len(ps) > 1), (case, got)
        assert [q[2] for q in ps] == [1] + [0] * (len(ps) - 1) and [q[3] for q in ps] == [0] * (len(ps) - 1) + [1], (case, got)
        seen += 1
    assert seen > len(grid_plans) // 2


# With every knob at its default: tile_log and the stage ranges of the passes, computed from the rule as the transform runner stated
# it before ntt_plan.h (on the CPU).
DEFAULT_PLANS = {
    1: (1, [(0, 1)]), 2: (2, [(0, 2)]), 3: (3, [(0, 3)]), 4: (4, [(0, 4)]), 5: (5, [(0, 5)]), 6: (6, [(0, 6)]), 7: (7, [(0, 7)]),
    8: (8, [(0, 4), (4, 8)]),
    9: (9, [(0, 5), (5, 9)]), 10: (9, [(0, 5), (5, 10)]), 11: (9, [(0, 6), (6, 11)]), 12: (9, [(0, 6), (6, 12)]),
    13: (9, [(0, 7), (7, 13)]), 14: (9, [(0, 7), (7, 14)]),
    15: (9, [(0, 5), (5, 10), (10, 15)]), 16: (9, [(0, 6), (6, 11), (11, 16)]), 17: (9, [(0, 6), (6, 12), (12, 17)]),
    18: (9, [(0, 6), (6, 12), (12, 18)]), 19: (9, [(0, 7), (7, 13), (13, 19)]),
    20: (10, [(0, 7), (7, 14), (14, 20)]), 21: (10, [(0, 7), (7, 14), (14, 21)]), 22: (10, [(0, 8), (8, 15), (15, 22)]),
    23: (10, [(0, 8), (8, 16), (16, 23)]), 24: (10, [(0, 8), (8, 16), (16, 24)]), 25: (10, [(0, 9), (9, 17), (17, 25)]),
    26: (10, [(0, 9), (9, 18), (18, 26)]), 27: (10, [(0, 9), (9, 18), (18, 27)]),
    28: (10, [(0, 7), (7, 14), (14, 21), (21, 28)]), 29: (10, [(0, 8), (8, 15), (15, 22), (22, 29)]),
}


def test_default_plans_are_the_ones_the_rule_gave_before(grid_plans):
    assert sorted(DEFAULT_PLANS) == list(LOG_NS)
    seen = 0
    for case, got in grid_plans:
        log_n, tile, stages, r4, thr, loaded, foreign, wide = case
        if (tile, stages, r4, thr, wide) != (0, 0, -1, 0, 1):
            continue
        tile_log, ranges = DEFAULT_PLANS[log_n]
        assert got["rc"] == nm.APK_OK and got["tile_log"] == tile_log, (case, got)
        assert [(q[0], q[1]) for q in got["passes"]] == ranges, (case, got)
        # radix 4: from 2^20 up always, at 2^17..2^19 only when loaded, below 2^17 never
        radix4 = log_n >= 20 or (log_n >= 17 and bool(loaded))
        assert all(q[4] == int(radix4) for q in got["passes"]), (case, got)
        by_load = radix4 and log_n <= 19
        want = nm.PATH_SEQ | (nm.PATH_R4 if radix4 else 0) | (nm.PATH_R4_LOAD if by_load else 0) | (nm.PATH_DEVICE_LOAD if by_load and foreign else 0)
        assert got["paths"] == want, (case, got)
        assert got["threads"] == (256 if not radix4 else (1 << tile_log) // 4 if tile_log < 10 else 256), (case, got)
        # the model says the same without the tool
        m = nm.plan(log_n, 3, loaded=bool(loaded), loaded_foreign=bool(foreign))
        assert (m.tile_log, list(m.stages)) == (tile_log, ranges) and all(q.radix4 == radix4 for q in m.passes)
        seen += 1
    assert seen == len(LOG_NS) * 4
    assert [nm.reads_load(l) for l in (16, 17, 19, 20)] == [False, True, True, False]


def test_refusals():
    zero, seventeen, no_ws, one_pass = _dump(["12 0 0 0 -1 0 0 0 1", "12 17 0 0 -1 0 0 0 1", "8 1 0 0 -1 0 0 0 0", "7 16 0 0 -1 0 0 0 0"])
    assert (zero["rc"], zero["message"]) == (nm.APK_ERR_ARG, "ntt: batch of 0")
    assert (seventeen["rc"], seventeen["message"]) == (nm.APK_ERR_ARG, "ntt: batch of 17")
    assert (no_ws["rc"], no_ws["message"]) == (nm.APK_ERR_STATE, "ntt: no workspace for this stream")
    assert one_pass["rc"] == nm.APK_OK and not one_pass["needs_wide"]      # one pass needs no workspace; 16 transforms are a full launch
    for count in (0, 17):
        with pytest.raises(nm.PlanError, match="ntt: batch of %d" % count) as e:
            nm.plan(12, count)
        assert e.value.rc == nm.APK_ERR_ARG
    with pytest.raises(nm.PlanError, match="ntt: no workspace for this stream") as e:
        nm.plan(8, 1, have_wide=False)
    assert e.value.rc == nm.APK_ERR_STATE

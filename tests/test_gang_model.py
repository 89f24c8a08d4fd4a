"""CPU tier: the plain-integer model of a gang's meeting (tests/gang_model.py: gang_launch's and flush_cmds' loops as they stood in
the prover), held to the C++ planner that restates them (algoplonk_amd/csrc/gang_plan.h through tools/gang_plan_dump) over every
meeting of up to four requests and every gang of up to four members with up to three recorded launches each - and the invariants a
member relies on to get ITS OWN commitment back, asserted on every plan.  No GPU."""
from __future__ import annotations

import itertools
import json
import os
import subprocess

import pytest

import gang_model as gm

CAPS = ((4, 8), (8, 4), (12, 16), (16, 12))          # (MSM, NTT): every capacity for either kind, never the same for both
CHOICES = ["m%s%d" % (t, b) for t in "AB" for b in (1, 2, 3, 4)] + ["n%s%d" % (s, k) for s in "XY" for k in (1, 3, 4)] + ["f"]
KIND = {"m": gm.KIND_MSM, "n": gm.KIND_NTT, "f": gm.KIND_FLUSH}


def _req(name):
    return gm.Req(gm.KIND_FLUSH) if name == "f" else gm.Req(KIND[name[0]], int(name[2]), name[1])


def _dump(what):
    r = subprocess.run(["make", "-C", gm.CSRC, "gang-plan-dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(gm.ROOT, "tools", "gang_plan_dump"), what], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def meetings():
    """(capacities, request names, the planner's groups) of every enumerated meeting"""
    out = [json.loads(l) for l in _dump("meetings")]
    return [(tuple(p["caps"]), p["reqs"], p["groups"]) for p in out]


def test_the_enumeration_is_the_whole_space(meetings):
    want = {(caps, names) for caps in CAPS for k in (1, 2, 3, 4) for names in itertools.product(CHOICES, repeat=k)}
    got = [(caps, tuple(names)) for caps, names, _ in meetings]
    assert len(got) == len(want) == 4 * (15 + 15 ** 2 + 15 ** 3 + 15 ** 4) and set(got) == want


def test_the_model_agrees_with_the_cpp_planner_on_every_meeting(meetings):
    merged = 0
    for caps, names, groups in meetings:
        want = gm.meeting([_req(x) for x in names], caps[0], caps[1])
        got = [gm.Group(k, tuple(rq), tuple(first), total, base, tuple(off) if k == gm.KIND_MSM else ()) for k, rq, first, total, base, off in groups]
        assert got == want, (caps, names, got, want)
        merged += any(len(g.reqs) > 1 for g in want)
    assert merged > len(meetings) // 4


def test_invariants_of_every_meeting(meetings):
    deferred = 0
    for caps, names, groups in meetings:
        reqs = [_req(x) for x in names]
        what = (caps, names, groups)
        placed = [j for _, rq, *_ in groups for j in rq]
        # every request but the flushes is in exactly one group
        assert sorted(placed) == [j for j, r in enumerate(reqs) if r.kind != gm.KIND_FLUSH], what
        areas = []
        for gi, (kind, rq, first, total, base, off) in enumerate(groups):
            cap = caps[0] if kind == gm.KIND_MSM else caps[1]
            # one kind, one table / shape; within the capacity
            assert rq and all(reqs[j].kind == kind and reqs[j].key == reqs[rq[0]].key for j in rq), what
            assert total == sum(reqs[j].count for j in rq) <= cap, what
            # the members' operands: in request order, one range behind the other from 0
            assert rq == sorted(rq) and first == [sum(reqs[j].count for j in rq[:k]) for k in range(len(rq))], what
            # groups run in the order of their first requests
            assert gi == 0 or groups[gi - 1][1][0] < rq[0], what
            if kind == gm.KIND_MSM:
                assert off == [base + f for f in first], what
                areas += [(o, o + reqs[j].count) for o, j in zip(off, rq)]
            # a request waits for a later group only if it did not match this one's opener or did not fit when its turn came
            room = 0
            for j in range(rq[0], len(reqs)):
                if j in rq:
                    room += reqs[j].count
                elif reqs[j].kind == kind and reqs[j].key == reqs[rq[0]].key and not any(j in g[1] for g in groups[:gi]):
                    assert room + reqs[j].count > cap, what
                    deferred += 1
        # no two members' sums overlap, and the sequences' sums are one behind the other from 0
        areas.sort()
        assert all(a[1] == b[0] for a, b in zip(areas, areas[1:])) and (not areas or areas[0][0] == 0), what
    assert deferred > 1000          # "did not fit" happened: a short member behind a deferred one still joined where it fitted


def test_every_compared_field_separates_two_requests():
    got = dict(l.split() for l in _dump("shapes"))
    assert got.pop("ntt0") == "1" and got.pop("msm0") == "1"
    assert got == dict([("ntt%d" % f, "2") for f in range(1, 9)] + [("msm1", "2")])
    # the model's shape is the tuple of the same eight fields
    base = (1, False, 4096, "pre", "post", "scale", 0, False)
    for f, v in enumerate((0, True, 4095, "post", "scale", "pre", 1, True)):
        other = base[:f] + (v,) + base[f + 1:]
        assert len(gm.meeting([gm.Req(gm.KIND_NTT, 2, base), gm.Req(gm.KIND_NTT, 2, other)], 16, 16)) == 2
    got = dict(l.split() for l in _dump("sigs"))
    assert got == {"0": "1", "1": "2", "2": "2", "3": "2", "4": "2", "5": "2"}
    a = gm.Sig(0x1000, 8, 1, 256, 0)
    for f, v in enumerate((0x2000, 9, 2, 64, 1024)):
        assert len(gm.flush([[a], [a._replace(**{gm.Sig._fields[f]: v})]])) == 2
    assert gm.flush([[a], [a]]) == [(0, (0, 1))]


SIGS = {"a": gm.Sig(0x1000, 8, 1, 256, 0), "b": gm.Sig(0x1000, 9, 1, 256, 0), "c": gm.Sig(0x2000, 8, 1, 256, 0)}
LISTS = [""] + ["".join(p) for n in (1, 2, 3) for p in itertools.product("abc", repeat=n)]


def _step_is_right(column, launches):
    """One step of a flush as the dump printed it: `column` holds every member's record of the step (a letter, or - for none),
    `launches` the members of each launch ("02 1").  The model's launches, every record exactly once, one signature per launch."""
    got = tuple(tuple(int(m) for m in x) for x in launches.split())
    same = got == gm.flush_step(tuple(SIGS.get(c) for c in column))
    once = sorted(m for ms in got for m in ms) == [m for m, c in enumerate(column) if c != "-"]
    return same and once and all(len({column[m] for m in ms}) == 1 for ms in got)


def test_the_flush_agrees_with_the_model_and_launches_every_record_once_in_order():
    """A line of the dump has the launches step by step (step i in field i: a member's step i comes before its step i + 1), and a
    step's launches depend on the members' records of that step alone, so a (column, launches) pair seen before is not judged again."""
    lines = _dump("flush")
    assert len(lines) == 40 + 40 ** 2 + 40 ** 3 + 40 ** 4
    padded = {l: l.ljust(3, "-") for l in LISTS}
    judged = {}
    for line in lines:
        left, right = line.split(" = ")
        steps = right.split("|")
        assert len(steps) == 3, line
        for key in zip(zip(*[padded[l] for l in left.split(",")]), steps):
            ok = judged.get(key)
            if ok is None:
                ok = judged[key] = _step_is_right(*key)
            assert ok, line
    assert len(judged) == 4 + 4 ** 2 + 4 ** 3 + 4 ** 4    # every column of none / a / b / c came up, with ONE answer
    assert sum(len(k[1].split()) < sum(c != "-" for c in k[0]) for k in judged) > len(judged) // 2      # most of them merge something
    # the whole-list model says the same as its steps (1 - 3 members: every gang; 4 members: every 97th)
    for line in lines[:40 + 40 ** 2 + 40 ** 3] + lines[40 + 40 ** 2 + 40 ** 3::97]:
        left, right = line.split(" = ")
        got = [(i, tuple(int(m) for m in x)) for i, s in enumerate(right.split("|")) for x in s.split()]
        assert got == gm.flush([[SIGS[c] for c in l] for l in left.split(",")]), line
    assert [tuple(l.split(" = ")[0].split(",")) for l in lines[:40 + 40 ** 2]] == [(x,) for x in LISTS] + [(b, a) for a in LISTS for b in LISTS]
    assert len({l.split(" = ")[0] for l in lines}) == len(lines)

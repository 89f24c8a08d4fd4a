"""Plain-integer model of a gang's meeting (test infrastructure): which requests share a launch sequence, where every member's
operands and sums sit, and which recorded kernels go out as one launch.

It restates, loop for loop, what the prover's gang_launch and flush_cmds did when these decisions still stood between their
launches and their writes to the members' slots - so that a reader can hold it against the C++ planner
(algoplonk_amd/csrc/gang_plan.h gang_plan_meeting, gang_plan_flush_step) side by side, and so that tests/test_gang_model.py can
hold that planner to it through tools/gang_plan_dump:

  meeting   for every request i in member order that no group has yet, flush requests aside: it opens a group; every request
            j >= i of the same kind that no group has yet joins, in order, when it has the opener's table (MSM) or shape (NTT)
            and the group's operands so far plus its own do not exceed the capacity (ws_batch for MSMs, NTT_MAX_BATCH x gang size
            for transforms); a member's sums start at res_off = res_base + the group's operands before it, and res_base advances
            by the group's total after every MSM group
  flush     for every step i up to the longest list, for every member a in order whose record i no launch has yet: one launch
            for it and for every later member b whose record i has the same function, grid.x, grid.y, block.x and LDS
"""
from __future__ import annotations

import functools
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")

GANG_MAX = 4
KIND_MSM, KIND_NTT, KIND_FLUSH = 1, 2, 3


class Req(NamedTuple):
    kind: int
    count: int = 0                 # MSM: a.batch; NTT: count
    key: object = None             # MSM: the table; NTT: (which, inverse, out_len, pre, post, scale, sub_log, semi)


class Group(NamedTuple):
    kind: int
    reqs: Tuple[int, ...]
    first: Tuple[int, ...]         # where each member's operands start in the merged batch
    total: int
    res_base: int                  # MSM groups: lead.res_write_off of the sequence
    res_off: Tuple[int, ...]       # MSM groups: member->res_off


def meeting(reqs: Sequence[Req], ws_batch: int, ntt_cap: int) -> List[Group]:
    """gang_launch's grouping loops"""
    count = len(reqs)
    done = [False] * GANG_MAX
    res_base = 0
    out: List[Group] = []
    for i in range(count):
        if done[i]:
            continue
        if reqs[i].kind == KIND_FLUSH:
            done[i] = True
            continue
        if reqs[i].kind == KIND_MSM:
            first = reqs[i]
            batch = 0                                        # c.batch
            grp, firsts, offs = [], [], []
            for j in range(i, count):
                if done[j] or reqs[j].kind != KIND_MSM:
                    continue
                m = reqs[j]
                if m.key != first.key or batch + m.count > ws_batch:
                    continue
                offs.append(res_base + batch)                # m->member->res_off
                firsts.append(batch)
                batch += m.count
                grp.append(j)
                done[j] = True
            out.append(Group(KIND_MSM, tuple(grp), tuple(firsts), batch, res_base, tuple(offs)))     # run_msm with res_write_off = res_base
            res_base += batch
        else:
            first = reqs[i]
            total = 0
            grp, firsts = [], []
            for j in range(i, count):
                if done[j] or reqs[j].kind != KIND_NTT:
                    continue
                m = reqs[j]
                if m.key != first.key or total + m.count > ntt_cap:
                    continue
                firsts.append(total)
                total += m.count
                grp.append(j)
                done[j] = True
            out.append(Group(KIND_NTT, tuple(grp), tuple(firsts), total, 0, ()))
    return out


class Sig(NamedTuple):
    """what flush_cmds compares of two recorded launches"""
    multi: int
    grid_x: int
    grid_y: int
    block_x: int
    lds: int


@functools.lru_cache(maxsize=None)
def flush_step(column: Tuple[Optional[Sig], ...]) -> Tuple[Tuple[int, ...], ...]:
    """the body of flush_cmds' loop over the steps: the launches of ONE step, given every member's record of that step (None: the
    member's list is shorter).  It reads nothing else, which is why the results may be remembered."""
    done = set()
    out = []
    for a in range(len(column)):
        if a in done or column[a] is None:
            continue
        ca = column[a]
        grp = []
        for b in range(a, len(column)):
            if b in done or column[b] is None:
                continue
            if column[b] != ca:
                continue
            grp.append(b)
            done.add(b)
        out.append(tuple(grp))
    return tuple(out)


def flush(cmds: Sequence[Sequence[Sig]]) -> List[Tuple[int, Tuple[int, ...]]]:
    """flush_cmds: the launches in order, each (step, the members it carries).  Members are numbered as given (the original walks
    only the members that have recorded anything; the others have no step to launch)."""
    longest = max([len(c) for c in cmds], default=0)
    out = []
    for i in range(longest):
        out += [(i, grp) for grp in flush_step(tuple(c[i] if i < len(c) else None for c in cmds))]
    return out

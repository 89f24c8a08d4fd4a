"""Plain-integer model of the MSM's signed-digit recoding and of the planner that picks its window (test infrastructure).

What it restates, rule by rule, so that a reader can hold it against the C++ side by side:
  * layout()          - the window layout of msm_plan_window (algoplonk_amd/csrc/msm_plan.h);
  * recode()          - the digit loop, written out three times in kernels_msm.h: msm_digits_kernel, msm_part_kernel and
                        msm_for_each_digit (the fused two-level sort and msm_density_kernel);
  * plan()            - msm_plan_context's default branch and msm_plan_window's limits (msm_plan.h), with the two-level sort's
                        packed-entry layout (MsmPartCfg);
  * sort_form()       - which sort msm_plan_batch takes for one MSM batch (msm_plan.h; msm_slice_one_level / _two_level,
                        msm_sort2_wanted);
  * edge_scalars()    - the words whose digits sit on every edge of the recoding, in every window where m < r allows it.

The kernel splits a 32-bit-limb word m < r.  On the canonical table (basis 0) m is the scalar's raw Montgomery word a R mod r
(the table holds R^-1 P); on the plain Lagrange table (basis 1) m is the canonical value (the PLAIN kernels leave the form first).
"""
from __future__ import annotations

import os
import random
import re
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")

LIMBS = 8                      # Fe<FR>::N for both scalar fields (ff_params.h: FrBN254 / FrBLS12381 N = 8)
R_MONT = 1 << 256              # gnark's Montgomery radix of Fr

# msm_plan.h constants the planner reads (same names there)
MSM_MAX_WINDOWS = 40
MSM_PACKED_NB = 65536
MSM_PART_MAX = 8192
MSM_PART_GMAX = 16384
MSM_LDS_WORDS = 40960
MSM_PART_TILE = 36864
MSM_PART_STAGE = 35584
MSM_G_MAX = 256
SLICE = 2048                   # MsmKnobs::slice (APK_MSM_SLICE default)


def ff_bits(struct: str) -> int:
    """FRP::BITS of a parameter struct of ff_params.h (FrBN254, FrBLS12381)."""
    src = open(os.path.join(CSRC, "ff_params.h")).read()
    m = re.search(r"struct %s\s*\{(.*?)\n\};" % struct, src, re.S)
    assert m, struct
    return int(re.search(r"static constexpr int BITS = (\d+);", m.group(1)).group(1))


@dataclass(frozen=True)
class Layout:
    W: int
    off: Tuple[int, ...]       # W + 1 entries, off[W] = BITS + 1
    width: Tuple[int, ...]


def layout(bits: int, c: int) -> Layout:
    """msm_plan_window: W = ceil((BITS + 1) / c) windows, the BITS + 1 bits spread with the wider windows first."""
    W = (bits + 1 + c - 1) // c
    base, extra = (bits + 1) // W, (bits + 1) % W
    width = tuple(base + (1 if j < extra else 0) for j in range(W))
    off = [0]
    for w in width:
        off.append(off[-1] + w)
    return Layout(W, tuple(off), width)


def recode(m: int, lay: Layout) -> List[int]:
    """The digit loop of msm_digits_kernel (= msm_part_kernel = msm_for_each_digit), over the 32-bit limbs of m: stream the limbs through a
    64-bit buffer, peel each window off its low end, and after the last limb let the buffer's zeros feed the top windows.
    Returns the signed digits d_j (the kernel emits bucket |d_j| - 1 with the sign bit, and nothing for d_j = 0)."""
    assert 0 <= m < 1 << (32 * LIMBS)
    limbs = [(m >> (32 * i)) & 0xFFFFFFFF for i in range(LIMBS)]
    out: List[int] = []
    carry, buf, avail, j = 0, 0, 0, 0
    for li in range(LIMBS):
        buf |= limbs[li] << avail
        assert buf < 1 << 64, "the 64-bit buffer overflowed"
        avail += 32
        while j < lay.W and (avail >= lay.width[j] or li == LIMBS - 1):
            c = lay.width[j]
            half = 1 << (c - 1)
            d = (buf & ((1 << c) - 1)) + carry
            buf >>= c
            avail -= c
            if d > half:                                                # d in (half, 2^c] -> -(2^c - d), carry 1
                out.append(-((1 << c) - d))
                carry = 1
            else:                                                       # d <= half stays positive (d = half included)
                out.append(d)
                carry = 0
            j += 1
    assert j == lay.W
    assert carry == 0, "a carry out of the top window: m needs more than BITS bits"
    return out


def raw_digits(m: int, lay: Layout) -> List[Tuple[int, int]]:
    """(field + carry-in, carry-in) of every window: the value the kernel compares with half in the digit loop, before the sign."""
    out, carry = [], 0
    for j in range(lay.W):
        c = lay.width[j]
        d = ((m >> lay.off[j]) & ((1 << c) - 1)) + carry
        out.append((d, carry))
        carry = 1 if d > 1 << (c - 1) else 0
    return out


# ---- the planner ------------------------------------------------------------------------------------------------------------
class PlanError(Exception):
    """msm_plan_context returns APK_ERR_ARG (the message names the rule)."""


@dataclass(frozen=True)
class Plan:
    c: int
    lay: Layout
    nb: int                     # buckets per MSM, 2^(c-1)
    idx_bits: int
    pb_log: int
    P: int                      # partitions of the two-level sort (0: the context does not take it)


def part_stage_max(P: int) -> int:
    """msm_part_stage_max as msm_ctx_stage_max calls it (P = 0 counts as 4)."""
    P = P or 4
    v = MSM_LDS_WORDS - 2 * P - 1 - 63
    return v if v < MSM_PART_STAGE else MSM_PART_STAGE


def _plan_c(bits: int, c: int, bases: int) -> Plan:
    """msm_plan_window: for a window c already chosen, its limits and the two-level sort's layout."""
    if c < 7 or c > 20:
        raise PlanError("msm_window %d out of [7,20]" % c)
    if c == 17 and bases > MSM_G_MAX * 3072:
        raise PlanError("msm_window 17 supports at most %d bases" % (MSM_G_MAX * 3072))
    lay = layout(bits, c)
    nb = 1 << (c - 1)
    if bases * lay.W >= 1 << 31:
        raise PlanError("bases*windows exceeds 2^31 table entries")
    idx_bits = 1
    while (1 << idx_bits) < bases * lay.W:
        idx_bits += 1
    target = MSM_PART_TILE - 2048
    per_msm = bases * lay.W
    pb_log = min(c - 1, 8)
    if idx_bits < 31 and pb_log > 31 - idx_bits:
        pb_log = 31 - idx_bits
    while pb_log > 2 and (nb >> pb_log) < MSM_PART_MAX and per_msm // (nb >> pb_log) > target:
        pb_log -= 1
    P = 0
    if (idx_bits <= 29 and pb_log >= 2 and idx_bits + pb_log <= 31 and (nb >> pb_log) >= 4 and (nb >> pb_log) <= MSM_PART_MAX
            and per_msm // (nb >> pb_log) <= MSM_PART_TILE - 2048):
        P = nb >> pb_log
    if nb > 65536:                                                                                     # msm_one_level_ok
        if P < 4:
            raise PlanError("msm_window %d: leave no room for the partition bits of the two-level sort" % c)
        if -(-bases // MSM_PART_GMAX) * lay.W > part_stage_max(P):
            raise PlanError("msm_window %d: more than %d sort slices" % (c, MSM_PART_GMAX))
    return Plan(c, lay, nb, idx_bits, pb_log if P else 0, P)


def plan(bits: int, fp_limbs: int, requested: int, log_size: int, bases: int, slots: int = 1) -> Plan:
    """msm_plan_context(bits, fp_limbs, bases, log_size, slots, requested) with APK_MSM_WINDOW and APK_MSM_PART_PBLOG unset.  fp_limbs is FPP::N: 8 for BN254, 12 for BLS12-381."""
    c = requested
    if c == 0 and log_size >= 20:
        for cand in (19, 18):
            if cand == 19 and log_size >= 22:
                continue
            try:
                return _plan_c(bits, cand, bases)
            except PlanError:
                pass
        c = 16
    if c == 0:
        c = min(max(log_size - 2, 8), 15)
        if log_size >= 21 or (log_size >= 17 and slots > 2):
            c = 16
        elif slots > 2 and log_size == 14:
            c = 13
        elif slots > 2 and log_size in (15, 16):
            c = 15
        if slots > 2 and log_size == 16 and fp_limbs <= 8:
            c = 16
        if log_size in (18, 19) and fp_limbs <= 8:
            c = 17
        if log_size == 17 and slots > 2 and fp_limbs <= 8:
            c = 17
    return _plan_c(bits, c, bases)


def msm_only_log_size(count: int) -> int:
    """init_msm_only (backend_impl.h): ceil(log2(count)).  A proving context passes log2(n) for n + 3 bases."""
    lg = 0
    while (1 << lg) < count:
        lg += 1
    return lg


CURVE_PARAMS = {"bn254": ("FrBN254", 8), "bls12-381": ("FrBLS12381", 12)}


def curve_bits(curve: str) -> int:
    return ff_bits(CURVE_PARAMS[curve][0])


def default_window(curve: str, log_size: int, slots: int = 1, bases: Optional[int] = None) -> int:
    """The window msm_plan_context picks by default.  bases defaults to 2^log_size + 3 (a proving context at n = 2^log_size);
    an MSM-only context over `count` bases is default_window(curve, msm_only_log_size(count), bases=count)."""
    if bases is None:
        bases = (1 << log_size) + 3
    return plan(curve_bits(curve), CURVE_PARAMS[curve][1], 0, log_size, bases, slots).c


def sort_form(p: Plan, bases: int, maxlen: int, batch: int = 1, sort2_env: int = -1, fused_env: int = 1) -> str:
    """msm_plan_batch's sort for one MSM batch on a lone context (no other proofs in flight; the workspace's own limits - which the
    default workspaces, msm_plan_workspace, meet - left out): "one-level", "four-launch" or "fused"."""
    slice_eff = 3072 if p.nb >= MSM_PACKED_NB and SLICE > 3072 else SLICE
    stage_max = part_stage_max(p.P)
    sl2 = slice_eff
    if sl2 * p.lay.W > stage_max:
        sl2 = stage_max // p.lay.W
    G2 = -(-maxlen // sl2)
    if G2 > 1024 and -(-maxlen // 1024) * p.lay.W <= stage_max:
        G2 = 1024
    elif G2 > MSM_PART_GMAX and -(-maxlen // MSM_PART_GMAX) * p.lay.W <= stage_max:
        G2 = MSM_PART_GMAX
    G2 = max(G2, 1)
    one_level_ok = p.nb <= 65536
    want = (not one_level_ok) or (sort2_env != 0 if sort2_env >= 0 else bases >= 65536)               # msm_sort2_wanted, not loaded
    sort2 = want and p.P >= 4 and G2 <= MSM_PART_GMAX and batch * p.P <= 4 * MSM_PART_MAX
    if not sort2:
        if not one_level_ok:
            raise PlanError("two levels only, and this batch does not fit them")
        return "one-level"
    per_slice = -(-maxlen // G2)
    stage_cap = min(per_slice * p.lay.W, stage_max)
    fused = fused_env and stage_cap // p.P >= 64 and per_slice * p.lay.W <= stage_max
    return "fused" if fused else "four-launch"


# ---- edge words ---------------------------------------------------------------------------------------------------------------
# the values of (field + carry-in) in the digit loop where the recoding changes behaviour: 0 / 1 (bucket 0), half - 1, half (the largest
# digit that stays positive), half + 1 (the smallest that turns negative and carries), 2^w - 1 (digit -1) and 2^w (an all-ones
# field plus a carry: "digit 0, carry 1")
EDGE_KINDS = ("0", "1", "half-1", "half", "half+1", "2^w-1", "2^w")


def edge_value(kind: str, w: int) -> int:
    half = 1 << (w - 1)
    return {"0": 0, "1": 1, "half-1": half - 1, "half": half, "half+1": half + 1, "2^w-1": (1 << w) - 1, "2^w": 1 << w}[kind]


def window_kinds(m: int, lay: Layout) -> List[set]:
    """The edge kinds word m hits, window by window (by its raw value field + carry-in)."""
    out = []
    for j, (d, _) in enumerate(raw_digits(m, lay)):
        w = lay.width[j]
        out.append({k for k in EDGE_KINDS if edge_value(k, w) == d})
    return out


@dataclass
class EdgeSet:
    values: List[int]                       # words m < r, in a fixed order
    labels: List[str]                       # what each value is for
    skipped: List[str] = field(default_factory=list)   # edges that cannot occur below r (window, kind, why)


def _carry_into(j: int, lay: Layout) -> int:
    """low bits that make window j see a carry-in of 1: window j - 1 holds an all-ones field (raw 2^w - 1 > half, or 2^w)."""
    return ((1 << lay.width[j - 1]) - 1) << lay.off[j - 1]


def edge_scalars(r: int, c_or_lay, domain: str = "raw", bits: Optional[int] = None, seed: int = 0) -> EdgeSet:
    """Words m < r that put every window on every edge kind (EDGE_KINDS) where m < r allows it, plus the window-offset and limb
    boundaries and the field's own extremes.  domain: "raw" - the words are raw Montgomery words (basis 0: the scalar's value is
    m R^-1), so R mod r (the value 1) and the Montgomery words of small values are added; "canonical" - the words are values
    (basis 1: pass to_mont(m)), so the small values themselves are.  Edges that no m < r reaches are listed in .skipped."""
    if isinstance(c_or_lay, Layout):
        lay = c_or_lay
    else:
        lay = layout(bits if bits is not None else r.bit_length(), c_or_lay)
    vals: List[int] = []
    labels: List[str] = []
    skipped: List[str] = []
    seen = set()

    def add(m: int, label: str) -> bool:
        if not 0 <= m < r:
            return False
        if m not in seen:
            seen.add(m)
            vals.append(m)
            labels.append(label)
        return True

    W = lay.W
    # 1. one window on one edge kind, the others zero (carry-in 0), and the same with a carry into it
    for j in range(W):
        w = lay.width[j]
        for kind in EDGE_KINDS:
            v = edge_value(kind, w)
            ok0 = v < (1 << w) and add(v << lay.off[j], "w%d=%s" % (j, kind))
            okc = j > 0 and v >= 1 and add(((v - 1) << lay.off[j]) | _carry_into(j, lay), "w%d=%s+carry" % (j, kind))
            if not ok0 and not okc:
                why = "needs a carry-in, window 0 has none" if j == 0 and kind == "2^w" else "m >= r"
                skipped.append("window %d: %s (%s)" % (j, kind, why))
    # 2. every window the same field value (the top window the largest reachable): carry chains run the whole word
    for kind in ("1", "half-1", "half", "half+1", "2^w-1"):
        m = 0
        for j in range(W):
            v = edge_value(kind, lay.width[j])
            cand = m | (v << lay.off[j])
            if cand >= r:
                v = (r - 1 - m) >> lay.off[j]          # largest field below r
                cand = m | (v << lay.off[j])
            m = cand
        add(m, "all=%s" % kind)
    # 3. the kinds rotated over the windows: every kind after every kind of the window below
    for s in range(len(EDGE_KINDS) - 1):
        m = 0
        for j in range(W):
            v = edge_value(EDGE_KINDS[(j + s) % (len(EDGE_KINDS) - 1)], lay.width[j])
            if (m | (v << lay.off[j])) < r:
                m |= v << lay.off[j]
        add(m, "rot%d" % s)
    # 4. window-offset boundaries and limb boundaries (windows that straddle a 32-bit limb)
    for j in range(W):
        add((1 << lay.off[j]) - 1, "2^off%d-1" % j)
        add(1 << lay.off[j], "2^off%d" % j)
        add((1 << lay.off[j + 1]) - (1 << lay.off[j]), "2^off%d-2^off%d" % (j + 1, j))
    for k in range(1, LIMBS):
        add((1 << (32 * k)) - 1, "2^%d-1" % (32 * k))
        add(1 << (32 * k), "2^%d" % (32 * k))
    # 5. the field's extremes
    for m, label in ((r - 1, "r-1"), (r - 2, "r-2"), ((r - 1) // 2, "(r-1)/2"), (R_MONT % r, "R mod r"), (0, "0"), (1, "1"), (2, "2"),
                     ((r - 1) >> 1 << 1, "even below r"), ((1 << (r.bit_length() - 1)) - 1, "2^(bits-1)-1")):
        add(m, label)
    if domain == "raw":
        for v in (1, 2, 3, r - 1, 1 << 16):
            add(v * R_MONT % r, "mont(%d)" % v if v < r - 1 else "mont(r-1)")
    elif domain == "canonical":
        for v in range(3, 17):
            add(v, str(v))
    else:
        raise ValueError(domain)
    # 6. random words whose every window is an edge kind (the top window clamped below r)
    g = random.Random(seed * 1000003 + lay.W)
    for t in range(24):
        m = 0
        for j in range(W):
            v = edge_value(g.choice(EDGE_KINDS[:-1]), lay.width[j])
            if (m | (v << lay.off[j])) < r:
                m |= v << lay.off[j]
        add(m, "mix%d" % t)
    return EdgeSet(vals, labels, skipped)


def all_half(r: int, lay: Layout) -> int:
    """Every window's digit = half (the largest positive digit); the top window holds the largest field below r."""
    m = 0
    for j in range(lay.W):
        cand = m | (1 << (lay.width[j] - 1) << lay.off[j])
        if cand < r:
            m = cand
        else:
            m |= ((r - 1 - m) >> lay.off[j]) << lay.off[j]
    return m

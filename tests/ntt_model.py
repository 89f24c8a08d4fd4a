"""Plain-integer model of the NTT's plan (test infrastructure): what one launch sequence of same-size transforms takes.

It restates, rule by rule, what the prover's transform runner decided when the decisions still stood between its launches - so
that a reader can hold it against the C++ planner (algoplonk_amd/csrc/ntt_plan.h ntt_plan) side by side, and so that
tests/test_ntt_model.py can hold that planner to it through tools/ntt_plan_dump:

  tile_log    log_n <= 19 ? 9 : 10, then APK_NTT_TILE_LOG (0 = rule), then clamped to log_n
  max_s       log_n <= 19 ? 7 : 9, then APK_NTT_STAGES (0 = rule), then clamped to tile_log
  passes      ceil(log_n / max_s)
  pass p      ceil((log_n - t0) / (passes - p)) stages from t0, the stage the pass before it ended at
  radix4      APK_NTT_RADIX4 if it is >= 0, else log_n > 19 or (log_n >= 17 and loaded)
  threads     NTT_THREADS; with radix 4 clamp(2^tile_log / 4, 64, NTT_THREADS); then APK_NTT_THREADS (0 = rule)
  grid_x      2^(log_n - tile_log)
  lds_bytes   2^tile_log * fe_u_bytes

A batch outside 1..NTT_ARGS_MAX is refused (APK_ERR_ARG); so is a sequence of more than one pass on a stream without a workspace,
or above 2^29 (APK_ERR_STATE).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")

# ntt_plan.h constants (same names there)
NTT_TILE_LOG = 11
NTT_THREADS = 256
NTT_MAX_BATCH = 4
NTT_ARGS_MAX = 16
FE_U_BYTES = 36                # sizeof(FeU<Fr>) for both scalar fields: 9 limbs of 32 bits

APK_OK, APK_ERR_ARG, APK_ERR_STATE = 0, 1, 3      # include/apk.h

# path counters a sequence bumps (NttPathBit)
PATH_SEQ, PATH_R4, PATH_R4_LOAD, PATH_DEVICE_LOAD = 1, 2, 4, 8


class PlanError(Exception):
    def __init__(self, rc: int, message: str):
        super().__init__(message)
        self.rc, self.message = rc, message


@dataclass(frozen=True)
class Pass:
    t0: int
    t1: int
    first: bool
    last: bool
    radix4: bool


@dataclass(frozen=True)
class Plan:
    tile_log: int
    passes: Tuple[Pass, ...]
    grid_x: int
    threads: int
    lds_bytes: int
    needs_wide: bool
    paths: int

    @property
    def stages(self):
        return tuple((p.t0, p.t1) for p in self.passes)


def reads_load(log_n: int) -> bool:
    """the sizes whose radix-4 choice follows the device's load"""
    return 17 <= log_n <= 19


def plan(log_n: int, count: int = 1, *, tile_knob: int = 0, stages_knob: int = 0, radix4_knob: int = -1, threads_knob: int = 0,
         loaded: bool = False, loaded_foreign: bool = False, have_wide: bool = True, fe_u_bytes: int = FE_U_BYTES) -> Plan:
    if count < 1 or count > NTT_ARGS_MAX:
        raise PlanError(APK_ERR_ARG, "ntt: batch of %d" % count)
    tile_log = tile_knob or (9 if log_n <= 19 else 10)
    max_s = stages_knob or (7 if log_n <= 19 else 9)
    tile_log = min(tile_log, log_n)
    max_s = min(max_s, tile_log)
    passes = -(-log_n // max_s)
    if passes > 1 and (not have_wide or log_n > 29):
        raise PlanError(APK_ERR_STATE, "ntt: no workspace for this stream")
    radix4 = bool(radix4_knob) if radix4_knob >= 0 else (log_n > 19 or (log_n >= 17 and loaded))
    paths = PATH_SEQ
    if radix4:
        paths |= PATH_R4
        if radix4_knob == -1 and log_n <= 19:
            paths |= PATH_R4_LOAD
            if loaded_foreign:
                paths |= PATH_DEVICE_LOAD
    threads = NTT_THREADS
    if radix4:
        threads = max(64, min((1 << tile_log) // 4, NTT_THREADS))
    if threads_knob:
        threads = threads_knob
    out, t0 = [], 0
    for p in range(passes):
        s = -(-(log_n - t0) // (passes - p))
        out.append(Pass(t0, t0 + s, p == 0, p == passes - 1, radix4))
        t0 += s
    return Plan(tile_log, tuple(out), 1 << (log_n - tile_log), threads, (1 << tile_log) * fe_u_bytes, passes > 1, paths)

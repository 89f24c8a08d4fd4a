"""-m gpu: the statistics around an MSM batch (apk_stats_enable / apk_stats_read) - the four HIP events the launch sequence records
in front of the batch, behind the bucket scan, behind the accumulate kernel and behind the reduction (csrc/msm_run.h MsmEvents,
handed in by run_msm_body), and the counters beside them.  A BN254 proving context at n = 2^10 with the default window.

The events only watch: a result with the statistics on is the result with them off, byte for byte.
"""
import ctypes as C
import random

import pytest

from algoplonk_amd import ecc, plonk, setup, workloads
from algoplonk_amd._lib import lib, check

pytestmark = pytest.mark.gpu

LOG_N = 10


@pytest.fixture(scope="module")
def rig(gpu):
    cv = ecc.BN254
    wl = workloads.random_circuit(cv, LOG_N, 0x57A7)
    srs = setup.unsafe_srs(cv, wl.ccs.domain_size(), wl.tau, device=gpu)
    pk, _ = plonk.Setup(wl.ccs, srs, device=gpu)
    yield cv, wl, pk
    pk.close()


def _blob(proof) -> bytes:
    out = C.create_string_buffer(2048)
    ln = C.c_size_t(0)
    check(lib.apk_marshal_proof(C.byref(proof.raw), out, 2048, C.byref(ln)))
    return out.raw[: ln.value]


def test_single_msm_is_timed_and_counted(rig):
    cv, wl, pk = rig
    n = wl.ccs.domain_size()
    assert n == 1 << LOG_N
    rng = random.Random(0x57A8)
    scalars = [rng.randrange(cv.r) for _ in range(n)]
    plain = pk.msm(scalars)
    pk.enable_stats(True)
    try:
        pk.stats(reset=True)
        timed = pk.msm(scalars)
        st = pk.stats(reset=True)
    finally:
        pk.enable_stats(False)
    parts = {k: getattr(st, k) for k in ("msm_sort_ms", "msm_accumulate_ms", "msm_tail_ms")}
    print("single MSM of %d:" % n, parts, "total", st.msm_total_ms)
    assert st.msm_batches == 1 and st.msm_accumulate_launches == 1 and st.msm_pairs == n
    assert st.msm_total_ms > 0
    for k, v in parts.items():
        assert 0 < v <= st.msm_total_ms, (k, v, st.msm_total_ms)
    assert timed == plain


def test_a_proof_is_the_same_with_statistics_and_counts_its_batches(rig):
    cv, wl, pk = rig
    plain = _blob(plonk.Prove(wl.ccs, pk, wl.witness, wl.blinding))
    pk.enable_stats(True)
    try:
        s0, p0 = pk.stats().msm_batches, pk.paths()["msm_batches"]
        timed = _blob(plonk.Prove(wl.ccs, pk, wl.witness, wl.blinding))
        s1, p1 = pk.stats().msm_batches, pk.paths()["msm_batches"]
    finally:
        pk.enable_stats(False)
    assert timed == plain
    assert s1 - s0 == p1 - p0 and p1 - p0 > 0, (s0, s1, p0, p1)

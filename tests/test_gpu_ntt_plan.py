"""GPU tier: transforms on both sides of the one plan boundary the other GPU tests do not cross with default knobs - 2^14, the
last size of two passes, and 2^15, the first of three (algoplonk_amd/csrc/ntt_plan.h; tests/test_ntt_model.py pins the stage ranges
on the CPU) - with 2^12 and 2^13 beside them.  Every output is held byte for byte to the C oracle, and the path counters say that
each call was one launch sequence without radix 4.  Default knobs only: forced plans are pinned on the CPU and by the knob rows
of tests/test_gpu_parity.py."""
from __future__ import annotations

import ctypes as C

import pytest

import ntt_model as nm
from algoplonk_amd import plonk, setup
from algoplonk_amd._lib import check, lib
from helpers import CURVES, random_chain_ccs
from oracle import c_oracle
from oracle.prng import SplitMix64, tau_from_seed

pytestmark = pytest.mark.gpu

LOG_NS = (12, 13)                                   # contexts of n = 2^12, 2^13: transforms of n and 4n = 2^12, 2^14 and 2^13, 2^15
PASSES = {12: 2, 13: 2, 14: 2, 15: 3}


def test_the_sizes_sit_on_both_sides_of_the_boundary():
    assert {lg: len(nm.plan(lg).passes) for lg in PASSES} == PASSES
    assert not any(nm.plan(lg).passes[0].radix4 or nm.reads_load(lg) for lg in PASSES)


@pytest.fixture(scope="module")
def clib():
    return c_oracle.load()


@pytest.fixture(scope="module")
def values():
    """2^15 SplitMix64 elements per curve, drawn once; a transform of 2^k takes the first 2^k"""
    out = {}
    for cname, (cv, _) in CURVES.items():
        g = SplitMix64(0x177 + cv.abi)
        out[cname] = cv.fr_vector([g.fr(cv.r) for _ in range(1 << 15)])
    return out


@pytest.mark.parametrize("log_n", LOG_NS)
@pytest.mark.parametrize("cname", list(CURVES))
def test_transforms_across_the_pass_boundary_match_the_oracle(gpu, clib, values, cname, log_n):
    cv, _ = CURVES[cname]
    ccs, _, _ = random_chain_ccs(cv, log_n, 31)
    n = ccs.domain_size()
    assert n == 1 << log_n
    pk, _ = plonk.Setup(ccs, setup.unsafe_srs(cv, n, tau_from_seed(5, cv.r), device=gpu), device=gpu)
    try:
        for which, size in ((0, n), (1, 4 * n)):
            assert len(nm.plan(size.bit_length() - 1).passes) == PASSES[size.bit_length() - 1]
            data = values[cname][:32 * size]
            for inverse, coset in ((0, 0), (1, 0)) + (((0, 1), (1, 1)) if which else ()):
                want = C.create_string_buffer(data, len(data))
                assert clib.orc_ntt(cv.abi, want, size, inverse, coset) == 0
                got = C.create_string_buffer(data, len(data))
                before = pk.paths()
                check(lib.apk_ntt(pk.ctx, which, inverse, coset, got))
                after = pk.paths()
                assert got.raw == want.raw, (cname, size, "inverse" if inverse else "forward", "coset" if coset else "")
                assert after["ntt_sequences"] == before["ntt_sequences"] + 1, (before, after)
                assert (after["ntt_radix4"], after["ntt_radix4_by_load"]) == (before["ntt_radix4"], before["ntt_radix4_by_load"]), (before, after)
    finally:
        pk.close()

"""CPU tier: marshalled proofs read back and verified (include/apk.h apk_proof_blob_len, apk_unmarshal_proof,
apk_unmarshal_public_inputs, apk_verify_blob; csrc/proof_codec.h).

The yardstick is tests/golden/template_verdicts.json: 10 cases x 7 proof / public-input blob pairs (the `rekey` runs are a
transaction field, not a proof-system input) with the verdict the reference's own verifier templates gave when they were executed.
apk_verify_blob takes the blobs as they are, so it is held to all 70 - including `claimed_value_plus_r` and
`proof_truncated_by_one_word`, which no apk_proof struct can express.  Nothing here needs a GPU.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

from algoplonk_amd import _lib
from algoplonk_amd._lib import lib

from helpers import CURVES
from test_template_pin import CASES, FIX, IDS, _product_vk

OK, ARG, BAD = _lib.APK_OK, _lib.APK_ERR_ARG, _lib.APK_ERR_VERIFY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "algoplonk_amd", "csrc")
CNAMES = ["bn254", "bls12-381"]
# apk_verify_trace field -> the template's name for the value (the map of tests/test_template_pin.py)
NAMES = {"gamma": "gamma", "beta": "beta", "alpha": "alpha", "zeta": "zeta", "pi": "PI", "lin_at_zeta": "linearized_poly_at_z",
         "gamma_kzg": "gamma_kzg", "folded_claim": "folded_claims"}


def fields(cv, k):
    """the proof blob's fields in wire order (helper.go:27-88): (name, offset, bytes, kind), a point's X and Y apart"""
    out, off = [], 0

    def pt(name):
        nonlocal off
        for kind in "XY":
            out.append((name, off, cv.fp_bytes, kind))
            off += cv.fp_bytes

    def sc(name):
        nonlocal off
        out.append((name, off, 32, "s"))
        off += 32

    for name in ("L", "R", "O", "H1", "H2", "H3"):
        pt(name)
    for name in ("l(zeta)", "r(zeta)", "o(zeta)", "s1(zeta)", "s2(zeta)"):
        sc(name)
    pt("Z"); sc("z(zeta w)"); pt("W_zeta"); pt("W_zeta_w")
    for i in range(k):
        sc("qcp_%d(zeta)" % i)
    for i in range(k):
        pt("Bsb22_%d" % i)
    return out, off


def unmarshal(cv, blob):
    raw = _lib.Proof()
    C.memset(C.byref(raw), 0xAB, C.sizeof(raw))                  # the reader writes every byte of the struct
    return lib.apk_unmarshal_proof(cv.abi, blob, len(blob), C.byref(raw)), raw


def unmarshal_public(cv, blob, cap=None):
    cap = len(blob) // 32 if cap is None else cap
    out = C.create_string_buffer(32 * max(cap, 1) + 32)
    nb = C.c_uint32(77)
    rc = lib.apk_unmarshal_public_inputs(cv.abi, blob, len(blob), out, cap, C.byref(nb))
    return rc, cv.fr_vector_decode(out.raw[: 32 * nb.value]) if rc == OK else None


def marshal(raw):
    out, n = C.create_string_buffer(2048), C.c_size_t(0)
    assert lib.apk_marshal_proof(C.byref(raw), out, 2048, C.byref(n)) == OK
    return out.raw[: n.value]


def verify_blob(rv, blob, pib, tr=None):
    return lib.apk_verify_blob(C.byref(rv), blob, len(blob), pib, len(pib), C.byref(tr) if tr is not None else None)


def well_formed(cv, blob, pib):
    return unmarshal(cv, blob)[0] == OK and unmarshal_public(cv, pib)[0] == OK


# ---- 1. the executed templates' verdicts ------------------------------------------------------------------------------------------------

def test_the_fixture_holds_seventy_proof_system_verdicts():
    assert sum(1 for c in CASES for r in c["results"] if not r["rekey"]) == 70
    assert sum(1 for c in CASES for r in c["results"] if r["mutation"] in ("claimed_value_plus_r", "proof_truncated_by_one_word")) == 20


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_apk_verify_blob_reproduces_every_verdict_of_the_executed_template(case):
    """Every non-rekey result: the verdict is the template's; where the blobs are well-formed the trace is the template's
    intermediates (z_commitment_off_curve: both refuse the point, the AVM at its first use, libapk before the transcript)."""
    cv, _ = CURVES[case["curve"]]
    rv = _product_vk(cv, case["vk"]).raw()
    w = 2 * cv.fp_bytes
    seen = 0
    for res in case["results"]:
        if res["rekey"]:
            continue
        blob, pib = bytes.fromhex(res["proof"]), bytes.fromhex(res["public_inputs"])
        tr = _lib.VerifyTrace()
        rc = verify_blob(rv, blob, pib, tr)
        assert rc == (OK if res["verdict"] == "accept" else BAD), (res["mutation"], lib.apk_last_error())
        seen += 1
        if not well_formed(cv, blob, pib):
            assert res["mutation"] in ("claimed_value_plus_r", "proof_truncated_by_one_word"), res["mutation"]
            assert bytes(tr) == bytes(C.sizeof(tr))              # nothing behind the point of rejection
            assert re.search(rb"(proof|public inputs) blob: .*byte", lib.apk_last_error()), lib.apk_last_error()
            continue
        if res["mutation"] == "z_commitment_off_curve":
            continue
        want = res["intermediates"]
        for mine, theirs in NAMES.items():
            assert int.from_bytes(bytes(getattr(tr, mine)), "big") == int(want[theirs], 16), (res["mutation"], mine)
        assert bytes(tr.lin_commitment)[:w].hex() == want["lin_poly_com"], res["mutation"]
        assert bytes(tr.folded_digest)[:w].hex() == want["folded_digest"], res["mutation"]
        # the same verdict and the same trace as apk_verify_ex on the unmarshalled struct
        rc2, raw = unmarshal(cv, blob)
        tr2 = _lib.VerifyTrace()
        pub = unmarshal_public(cv, pib)[1]
        assert lib.apk_verify_ex(C.byref(rv), C.byref(raw), cv.fr_vector(pub), len(pub), C.byref(tr2)) == rc and bytes(tr2) == bytes(tr)
    assert seen == 7


def test_the_negative_control_is_rejected():
    """a BN254 pythagorean proof whose prover hashed infinity as 0x40 00..: well-formed bytes, rejected by the template and here"""
    nc = FIX["negative_control"]
    case = next(c for c in CASES if c["curve"] == "bn254" and c["circuit"] == "pythagorean")
    cv, _ = CURVES["bn254"]
    rv = _product_vk(cv, case["vk"]).raw()
    blob, pib = bytes.fromhex(nc["proof"]), bytes.fromhex(nc["public_inputs"])
    assert nc["verdict"] == "reject" and well_formed(cv, blob, pib)
    assert verify_blob(rv, blob, pib) == BAD
    assert b"pairing check" in lib.apk_last_error()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sizes_that_are_not_the_key_s_are_rejected(case):
    """a well-formed blob whose k is not the key's, and a public blob that is not 32 x nb_public bytes"""
    cv, _ = CURVES[case["curve"]]
    k = len(case["vk"]["qcp"])
    rv = _product_vk(cv, case["vk"]).raw()
    valid = case["results"][0]
    blob, pib = bytes.fromhex(valid["proof"]), bytes.fromhex(valid["public_inputs"])
    assert verify_blob(rv, blob, pib) == OK
    other = next(c for c in CASES if c["curve"] == case["curve"] and len(c["vk"]["qcp"]) != k)
    assert verify_blob(rv, bytes.fromhex(other["results"][0]["proof"]), pib) == BAD
    assert b"does not match the verifying key" in lib.apk_last_error()
    for bad in (pib + bytes(32), pib[:-32], pib[:-1], pib + b"\x00"):
        assert verify_blob(rv, blob, bad) == BAD, len(bad)
        assert b"public inputs blob" in lib.apk_last_error()
    assert lib.apk_verify_blob(None, blob, len(blob), pib, len(pib), None) == ARG
    assert lib.apk_verify_blob(C.byref(rv), None, len(blob), pib, len(pib), None) == ARG
    if pib:
        assert lib.apk_verify_blob(C.byref(rv), blob, len(blob), None, len(pib), None) == ARG
    rv.curve = 9
    assert verify_blob(rv, blob, pib) == ARG


# ---- 2. round trips -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_round_trips(case):
    cv, _ = CURVES[case["curve"]]
    k = len(case["vk"]["qcp"])
    nb = 0
    for res in case["results"]:
        blob, pib = bytes.fromhex(res["proof"]), bytes.fromhex(res["public_inputs"])
        if res["rekey"] or not well_formed(cv, blob, pib):
            continue
        nb += 1
        rc, p = unmarshal(cv, blob)
        assert rc == OK and (p.curve, p.nb_commitments) == (cv.abi, k)
        assert marshal(p) == blob
        # slot 0 of the claimed values and the five diagnostic challenges are not on the wire: written as zero
        assert bytes(p.claimed_values[0]) == bytes(32)
        for name in ("gamma", "beta", "alpha", "zeta", "gamma_kzg"):
            assert bytes(getattr(p, name)) == bytes(32)
        # unmarshal(marshal(q)) == q in every field of the proof, whatever q holds in the fields that do not travel
        q = _lib.Proof()
        C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
        C.memmove(q.claimed_values[0], cv.fr_to_mont_bytes(12345), 32)
        for name in ("gamma", "beta", "alpha", "zeta", "gamma_kzg"):
            C.memmove(getattr(q, name), cv.fr_to_mont_bytes(99), 32)
        rc, back = unmarshal(cv, marshal(q))
        assert rc == OK and bytes(back) == bytes(p)
        assert bytes(back.claimed_values)[32:] == bytes(q.claimed_values)[32:]
        # public inputs
        rc, pub = unmarshal_public(cv, pib)
        assert rc == OK and pub == [int.from_bytes(pib[i: i + 32], "big") for i in range(0, len(pib), 32)]
        out = C.create_string_buffer(max(len(pib), 1))
        assert lib.apk_marshal_public_inputs(cv.abi, cv.fr_vector(pub), len(pub), out, len(pib)) == OK and out.raw[: len(pib)] == pib
    assert nb >= 5


# ---- 3. malformed input --------------------------------------------------------------------------------------------------------------------

def _valid(cname, k):
    case = next(c for c in CASES if c["curve"] == cname and len(c["vk"]["qcp"]) == k)
    return bytes.fromhex(case["results"][0]["proof"]), bytes.fromhex(case["results"][0]["public_inputs"])


def _well_formed_by_k(cname):
    """a well-formed blob of every k, cut from the k = 2 proof (only ranges are checked by the reader)"""
    cv, _ = CURVES[cname]
    b2, _p = _valid(cname, 2)
    base, w = lib.apk_proof_blob_len(cv.abi, 0), 2 * cv.fp_bytes
    return [b2[:base], b2[:base] + b2[base: base + 32] + b2[base + 64: base + 64 + w], b2]


@pytest.mark.parametrize("cname", CNAMES)
def test_only_the_three_exact_lengths_parse(cname):
    cv, _ = CURVES[cname]
    wf = _well_formed_by_k(cname)
    lens = [lib.apk_proof_blob_len(cv.abi, k) for k in range(3)]
    assert [len(b) for b in wf] == lens
    parsed = {}
    for n in range(lens[2] + 34):
        src = next((b for b in wf if n <= len(b)), None) or wf[2] + bytes(n - lens[2])
        rc, p = unmarshal(cv, src[:n])
        if rc == OK:
            parsed[n] = p.nb_commitments
        else:
            assert rc == BAD and (b"proof blob: %d bytes" % n) in lib.apk_last_error(), (n, lib.apk_last_error())
            assert bytes(p) == bytes(C.sizeof(p))
    assert parsed == {lens[0]: 0, lens[1]: 1, lens[2]: 2}


@pytest.mark.parametrize("cname", CNAMES)
def test_values_out_of_range_are_named_with_their_offset(cname):
    cv, _ = CURVES[cname]
    blob, pib = _valid(cname, 2)
    case = next(c for c in CASES if c["curve"] == cname and len(c["vk"]["qcp"]) == 2)
    rv = _product_vk(cv, case["vk"]).raw()
    fl, total = fields(cv, 2)
    assert total == len(blob) and len(fl) == 2 * 11 + 8

    def rejected(mutated, name, off, what):
        rc, p = unmarshal(cv, mutated)
        err = lib.apk_last_error()
        assert rc == BAD and bytes(p) == bytes(C.sizeof(p)), (name, off)
        assert (b"%s at byte %d: " % (name.encode(), off)) in err and what in err, err
        assert verify_blob(rv, mutated, pib) == BAD and lib.apk_last_error() == err

    for name, off, size, kind in fl:
        if kind == "s":
            rejected(blob[:off] + cv.r.to_bytes(32, "big") + blob[off + 32:], name, off, b"scalar is not below r")
            assert unmarshal(cv, blob[:off] + (cv.r - 1).to_bytes(32, "big") + blob[off + 32:])[0] == OK
        else:
            for v in (cv.p, (1 << (8 * size)) - 1):
                rejected(blob[:off] + v.to_bytes(size, "big") + blob[off + size:], name, off, kind.encode() + b" is not below the field modulus")
            assert unmarshal(cv, blob[:off] + (cv.p - 1).to_bytes(size, "big") + blob[off + size:])[0] == OK     # range only: not a curve check
    # public inputs: one byte short, a value equal to r
    assert len(pib) >= 32
    rc, _v = unmarshal_public(cv, pib[:-1])
    assert rc == BAD and b"not a multiple of 32" in lib.apk_last_error()
    assert verify_blob(rv, blob, pib[:-1]) == BAD
    bad = pib[:-32] + cv.r.to_bytes(32, "big")
    rc, _v = unmarshal_public(cv, bad)
    assert rc == BAD and (b"value %d at byte %d: scalar is not below r" % (len(pib) // 32 - 1, len(pib) - 32)) in lib.apk_last_error()
    assert verify_blob(rv, blob, bad) == BAD
    assert unmarshal_public(cv, pib[:-32] + (cv.r - 1).to_bytes(32, "big"))[0] == OK
    assert unmarshal_public(cv, b"") == (OK, [])


@pytest.mark.parametrize("cname", CNAMES)
def test_argument_errors_and_lengths(cname):
    cv, _ = CURVES[cname]
    blob, pib = _valid(cname, 1)
    raw, nb, out = _lib.Proof(), C.c_uint32(0), C.create_string_buffer(64 + len(pib))
    assert lib.apk_unmarshal_proof(cv.abi, None, len(blob), C.byref(raw)) == ARG
    assert lib.apk_unmarshal_proof(cv.abi, blob, len(blob), None) == ARG
    assert lib.apk_unmarshal_proof(5, blob, len(blob), C.byref(raw)) == ARG and b"curve" in lib.apk_last_error()
    assert lib.apk_unmarshal_public_inputs(cv.abi, None, len(pib), out, 8, C.byref(nb)) == ARG
    assert lib.apk_unmarshal_public_inputs(cv.abi, pib, len(pib), None, 8, C.byref(nb)) == ARG
    assert lib.apk_unmarshal_public_inputs(cv.abi, pib, len(pib), out, 8, None) == ARG
    assert lib.apk_unmarshal_public_inputs(5, pib, len(pib), out, 8, C.byref(nb)) == ARG
    assert lib.apk_unmarshal_public_inputs(cv.abi, pib, len(pib), out, len(pib) // 32 - 1, C.byref(nb)) == ARG     # cap too small
    assert b"do not fit" in lib.apk_last_error()
    assert lib.apk_unmarshal_public_inputs(cv.abi, pib, len(pib), out, len(pib) // 32, C.byref(nb)) == OK and nb.value == len(pib) // 32
    want = {(0, 0): 768, (0, 1): 864, (0, 2): 960, (1, 0): 1056, (1, 1): 1184, (1, 2): 1312}
    for curve in (-1, 0, 1, 2):
        for k in (0, 1, 2, 3, 1 << 31):
            assert lib.apk_proof_blob_len(curve, k) == want.get((curve, k), 0)


# ---- 4. the codec stand-alone under ASAN + UBSAN ---------------------------------------------------------------------------------------------

def _library_counts(blobs):
    """the attempts of tools/san/proof_codec_check.cpp made through libapk: {(what, kind): [accepted, rejected]}"""
    counts = {(w, kd): [0, 0] for w in ("proof", "public") for kd in ("whole", "truncation", "flip", "zeros", "ones")}

    def attempt(cv, is_proof, data, kind):
        rc = unmarshal(cv, data)[0] if is_proof else unmarshal_public(cv, data)[0]
        assert rc in (OK, BAD)
        counts[("proof" if is_proof else "public", kind)][0 if rc == OK else 1] += 1
        return rc

    for cv, is_proof, blob in blobs:
        assert attempt(cv, is_proof, blob, "whole") == OK
        if is_proof:
            k = unmarshal(cv, blob)[1].nb_commitments
            edges = [e for _n, off, size, _k in fields(cv, k)[0] for e in (off, off + size - 1)]
        else:
            edges = [e for i in range(0, len(blob), 32) for e in (i, i + 31)]
        for cut in range(len(blob)):
            attempt(cv, is_proof, blob[:cut], "truncation")
        for e in edges:
            attempt(cv, is_proof, blob[:e] + bytes([blob[e] ^ 0xFF]) + blob[e + 1:], "flip")
        attempt(cv, is_proof, bytes(len(blob)), "zeros")
        attempt(cv, is_proof, b"\xff" * len(blob), "ones")
    return counts


def test_proof_codec_under_address_and_undefined_sanitizers(tmp_path):
    """proof_codec.h alone, as its own process: every truncation, both edge bytes of every field inverted, all 0x00, all 0xFF on
    exactly sized heap copies of the fixture's valid blobs.  It ends clean, and accepts / rejects what libapk does."""
    r = subprocess.run(["make", "-C", CSRC, "san-codec"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blobs, lines = [], []
    for case in CASES:
        cv, _ = CURVES[case["curve"]]
        valid = case["results"][0]
        for kind, hx in (("P", valid["proof"]), ("I", valid["public_inputs"])):
            blobs.append((cv, kind == "P", bytes.fromhex(hx)))
            lines.append("%d %s %s" % (cv.abi, kind, hx or "-"))
    path = tmp_path / "blobs.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tools", "san", "proof_codec_check"), str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "PROOF CODEC CHECK OK: %d blobs" % len(lines) in r.stdout, (r.stdout[-2500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = {(m.group(1), m.group(2)): [int(m.group(3)), int(m.group(4))]
           for m in re.finditer(r"^(proof|public) (\w+) accept (\d+) reject (\d+)$", r.stdout, re.M)}
    want = _library_counts(blobs)
    assert got == want
    # the counts are not vacuous: whole blobs parse, no truncation of a valid k = 0 blob does, all-0xFF never does, all-zero always
    assert want[("proof", "whole")] == [10, 0] and want[("proof", "ones")] == [0, 10] and want[("proof", "zeros")] == [10, 0]
    assert want[("proof", "truncation")][1] > 9000 and want[("proof", "flip")][0] > 0 and want[("proof", "flip")][1] > 0

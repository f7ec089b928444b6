"""CPU tier of the raw-message entries of the generic verifiers (include/sbv.h: sbv_p256_verify_msgs, sbv_secp256k1_verify_msgs,
sbv_p256_verify_msgs_sharded; consensus_amd/csrc/sha256_dev.h: msg_frontend_tuple_lane).

tests/emul/msgs_generic_emul.cc compiles the lane the gfx950 kernel is built from with g++.  Every case of tests/msgs_generic_cases.py
goes through it: the tuple equals strict_rs | hashlib.sha256 | key byte for byte, and the tuple's verdict by the C oracles (and, for
P-256, OpenSSL) equals `want`.  A host model of the kernel's slice check gets offsets below the base, above the upload and decreasing:
each gives an empty message and an empty signature.  The same source, built as a program of its own with AddressSanitizer and UBSan
and every message, signature and key in a heap buffer of exactly its length, holds the rule that nothing outside msg[0 .. len),
der[0 .. dlen) and key[0 .. 64) is read."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import pytest

import frontend_cases as fc
import msgs_generic_cases as mg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_SRC = os.path.join(HERE, "emul", "msgs_generic_emul.cc")
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
EMPTY = bytes(64) + hashlib.sha256(b"").digest()


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in ("sha256_dev.h", "sbv_common.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(HERE, "emul", "libsbv_msgs_generic_emul.so")
    if _stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-misleading-indentation", EMUL_SRC, "-o", so])
    lib = ctypes.CDLL(so)
    C, S, U64 = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64
    lib.sbvmg_lane.argtypes = [C, S, C, S, C, ctypes.c_void_p]
    lib.sbvmg_lane.restype = None
    lib.sbvmg_kernel.argtypes = [C, ctypes.POINTER(U64), C, ctypes.POINTER(U64), C, S, ctypes.c_void_p, U64, U64, U64, U64]
    lib.sbvmg_kernel.restype = None
    return lib


def _all_cases(scheme):
    fams = mg.families(scheme)
    return [c for f in sorted(fams) for c in fams[f]] + mg.key_cases(scheme) + mg.empty_batch(scheme) + mg.filler(scheme)


def _verdict(scheme, t):
    o = fc.oracle()
    if scheme == "p256":
        o.sbvo_p256_verify_tuple.argtypes = [ctypes.c_char_p]
        return bool(o.sbvo_p256_verify_tuple(t))
    return bool(o.sbvo_k256_verify_raw(t[:32], t[32:64], t[64:96], t[96:128], t[128:160]))


def _offsets(parts, base=0):
    o = (ctypes.c_uint64 * (len(parts) + 1))()
    o[0] = base
    for i, p in enumerate(parts):
        o[i + 1] = o[i] + len(p)
    return o


# ---- the cases themselves -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_cases_drop_the_slot_rule_and_keep_every_front_end_case(scheme):
    fams, theirs = mg.families(scheme), fc.families(scheme)
    assert sorted(fams) == ["a", "b", "c", "d", "e"]
    for f in fams:
        assert [(c.name, c.key, c.msg, c.sig) for c in fams[f]] == [(c.name, c.key, c.msg, c.sig) for c in theirs[f]]
        for mine, c in zip(fams[f], theirs[f]):
            assert mine.want == (c.want if c.rule == fc.OWN else fc.judge(scheme, c.key, c.msg, c.sig)), c.name
    named = {c.name: c for c in fams["e"]}
    assert named["e_slot_eq_nkeys"].want and named["e_slot_ffffffff"].want        # rejected for their slots by the keyed entries, accepted on their signatures here
    assert not named["e_key_is_no_point"].want
    keys = mg.key_cases(scheme)
    assert [c.name for c in keys] == ["k_honest", "k_qx_eq_p", "k_qy_eq_p_plus_1", "k_qy_eq_1_reduced", "k_qy_bit_flipped", "k_zero_zero",
                                      "k_other_curve", "k_negated"]
    assert [c.want for c in keys] == [True] + [False] * 7
    p = fc.CURVES[scheme].P
    assert int.from_bytes(keys[1].key[:32], "big") == p and int.from_bytes(keys[2].key[32:], "big") == p + 1
    assert keys[2].key[:32] == keys[3].key[:32] and fc.CURVES[scheme].mod.on_curve(int.from_bytes(keys[3].key[:32], "big"), 1)
    assert len({c.sig for c in keys}) == 1 and len({c.msg for c in keys}) == 1


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_long_tail_has_the_layout_and_the_oracle_agrees_with_its_generator(scheme):
    """12 signers above 256 uses, 12 at 85, 100 keys used once; the expected bits of the generator are the C oracle's on every tuple"""
    import collections
    cases = mg.long_tail(scheme)
    assert len(cases) == mg.MAIN
    every = collections.Counter(c.key for c in cases)
    uses = sorted(every.values())
    assert len(every) == 124 and uses[:100] == [1] * 100                      # the keys used once
    assert all(64 <= v <= mg.LIGHT_USES for v in uses[100:112])              # grouped (>= 64 uses), below the 256 uses of a full table
    assert all(v > 256 for v in uses[112:])
    assert [c.want for c in cases] == [i % 5 != 4 for i in range(mg.MAIN)]
    blob = mg.tuples(cases)
    o = fc.oracle()
    out = ctypes.create_string_buffer((mg.MAIN + 7) // 8)
    name = "sbvo_p256_verify_batch" if scheme == "p256" else "sbvo_k256_verify_batch"
    getattr(o, name).argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    getattr(o, name)(blob, mg.MAIN, out, min(os.cpu_count() or 1, 16))
    got = [bool((out.raw[i >> 3] >> (i & 7)) & 1) for i in range(mg.MAIN)]
    assert got == [c.want for c in cases]


# ---- the lane -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_lane_writes_the_host_routes_tuple_and_the_oracles_judge_it_as_wanted(scheme, emul):
    """every case: the lane's 160 bytes are strict_rs | hashlib.sha256 | key (zeros for a refused signature), and the tuple's verdict
    by the C oracle — for P-256 by OpenSSL too — is `want`"""
    ssl = fc.openssl()
    if ssl is not None:
        ssl.sbvssl_p256_verify_tuple.argtypes = [ctypes.c_char_p]
    out = ctypes.create_string_buffer(160)
    cases = _all_cases(scheme)
    assert len(cases) > 1300
    for c in cases:
        emul.sbvmg_lane(c.msg, len(c.msg), c.sig, len(c.sig), c.key, out)
        assert out.raw == (fc.strict_rs(c.sig) or bytes(64)) + hashlib.sha256(c.msg).digest() + c.key == mg.tuple_of(c), c.name
        assert _verdict(scheme, out.raw) == c.want, c.name
        if scheme == "p256" and ssl is not None:
            assert bool(ssl.sbvssl_p256_verify_tuple(out.raw)) == c.want, c.name


def test_openssl_third_opinion_is_there():
    """the P-256 comparison above must not pass by absence"""
    assert fc.openssl() is not None


# ---- the kernel's slice check -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_kernel_model_reads_the_packed_batch_and_empties_a_lane_with_a_bad_slice(scheme, emul):
    """the kernel model over a packed batch with bases above 0 gives every lane's tuple; an offset below the base, above the upload or
    decreasing turns the lanes that read it into an empty message and an empty signature, and the Python model of the check agrees"""
    cases = mg.families(scheme)["e"] + mg.key_cases(scheme) + mg.families(scheme)["b"][:8] + [c for c in mg.ladder(scheme)[0] if len(c.msg) in (0, 55, 56, 64, 119, 1025)]
    msgs, sigs, keys, _ = mg.batch(cases)
    n = len(cases)
    mbase, sbase = 4096, 123
    mblob, sblob, kblob = b"".join(msgs), b"".join(sigs), b"".join(keys)
    honest = [mg.tuple_of(c) for c in cases]

    def run(mo, so):
        out = ctypes.create_string_buffer(160 * n)
        emul.sbvmg_kernel(mblob, mo, sblob, so, kblob, n, out, mbase, sbase, len(mblob), len(sblob))
        return [out.raw[160 * i:160 * i + 160] for i in range(n)]

    assert run(_offsets(msgs, mbase), _offsets(sigs, sbase)) == honest
    at = next(i for i in range(2, n - 2) if len(msgs[i - 1]) and len(msgs[i]) and len(sigs[i]))
    assert honest[at] != EMPTY + keys[at]
    for table in ("m", "s"):
        good = _offsets(msgs, mbase) if table == "m" else _offsets(sigs, sbase)
        base, size = (mbase, len(mblob)) if table == "m" else (sbase, len(sblob))
        assert good[at] > base
        for what, where, value in (("below the base", at, base - 1), ("above the upload", at + 1, base + size + 1), ("decreasing", at + 1, good[at] - 1)):
            mo, so = _offsets(msgs, mbase), _offsets(sigs, sbase)
            (mo if table == "m" else so)[where] = value
            got = run(mo, so)
            assert mg.lane_slice(mo, so, at, mbase, sbase, len(mblob), len(sblob)) == (0, 0, 0, 0), (table, what)
            assert got[at] == EMPTY + keys[at], (table, what)                  # an empty message AND an empty signature
            for i in range(n):                                                 # every lane is what the model of the check says, none reads outside
                m0, m1, s0, s1 = mg.lane_slice(mo, so, i, mbase, sbase, len(mblob), len(sblob))
                want = (fc.strict_rs(sblob[s0:s1]) or bytes(64)) + hashlib.sha256(mblob[m0:m1]).digest() + keys[i]
                assert got[i] == want, (table, what, i)
                if i not in (where - 1, where):
                    assert got[i] == honest[i], (table, what, i)


# ---- the sanitizer program ----------------------------------------------------------------------------------------------------------
def test_sanitizer_build_runs_every_case_as_a_program_of_its_own(tmp_path):
    """the same source with its own main under AddressSanitizer and UBSan, one run per curve's cases: every message, signature and key
    from a heap buffer of exactly its length, through the lane alone and through the kernel model with honest and bent tables"""
    exe = str(tmp_path / "msgs_generic_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-Wno-misleading-indentation", EMUL_SRC, "-o", exe])
    for scheme in mg.SCHEMES:
        cases = _all_cases(scheme)
        path = tmp_path / ("cases_%s.txt" % scheme)
        path.write_text("".join(" ".join(x.hex() or "-" for x in (c.msg, c.sig, c.key, mg.tuple_of(c))) + "\n" for c in cases))
        run = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert run.returncode == 0, (scheme, run.stdout[-2000:], run.stderr[-4000:])
        assert "%d cases, 7 table forms, 0 mismatches" % len(cases) in run.stdout


# ---- the header and the Go adapter --------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entries_and_keeps_its_counts():
    hdr = open(os.path.join(ROOT, "include", "sbv.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for name in ("sbv_p256_verify_msgs", "sbv_secp256k1_verify_msgs", "sbv_p256_verify_msgs_sharded"):
        assert re.search(r"\bint %s\(const uint8_t\* msgs, const uint64_t\* msg_offsets, const uint8_t\* sigs, const uint64_t\* sig_offsets, "
                         r"const uint8_t\* keys, size_t n, " % name, flat), name
        assert not name.endswith("_dev")
    assert hdr.count("int sbv_secp256k1_") == 12           # the one-line prototypes three other CPU tiers count
    assert "ALWAYS splits contiguously" in hdr
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    go = os.path.join(ROOT, "go", "gpuverifier")
    _, problems, protos = check_cgo.check(go, os.path.join(ROOT, "include", "sbv.h"))
    assert not problems, problems
    u8, u64, S = ("uint8_t", True), ("uint64_t", True), ("size_t", False)
    assert protos["sbv_p256_verify_msgs"] == protos["sbv_secp256k1_verify_msgs"] == [u8, u64, u8, u64, u8, S, u8]


def test_library_exports_the_three_entries():
    """the symbols of the built library, where it has been built (build() builds it before any test runs)"""
    so = os.path.join(ROOT, "consensus_amd", "libsbv.so")
    assert os.path.exists(so), "libsbv.so is built by build()"
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("sbv_p256_verify_msgs", "sbv_secp256k1_verify_msgs", "sbv_p256_verify_msgs_sharded"):
        assert re.search(r" T %s$" % name, syms, re.M), name


# ---- the host Verifier on the callback backend --------------------------------------------------------------------------------------
def unregistered_clients(lib, hx, scheme, count=5):
    """`count` clients registered while device client keys are off: they hold no slot, so their requests carry their keys"""
    lib.sbvh_set_device_client_keys(hx.v, 0)
    for i in range(count):
        s = lib.sbvh_signer_new_scheme(scheme, 0, hashlib.sha256(b"open client %d" % i).digest())
        q = ctypes.create_string_buffer(64)
        lib.sbvh_signer_public_key(s, q)
        lib.sbvh_register_client(hx.v, b"bob%d" % i, q.raw)
        hx.clients["bob%d" % i] = s


def proposals_of_unregistered_clients(lib, hx, n=150):
    """n requests of slotted and unslotted clients in one proposal: OK through ONE batch of the raw-message form; with one corrupt
    signature INVALID; returns how many raw-message batches the backend ran"""
    import hostlib
    lib.sbvh_backend_msgs_batches.restype = ctypes.c_uint64
    lib.sbvh_backend_msgs_batches.argtypes = [ctypes.c_void_p]
    lib.sbvh_backend_keyed_batches.restype = ctypes.c_uint64
    lib.sbvh_backend_keyed_batches.argtypes = [ctypes.c_void_p]
    before, keyed = lib.sbvh_backend_msgs_batches(hx.v), lib.sbvh_backend_keyed_batches(hx.v)
    reqs = [hx.request(("bob%d" % (i % 5)) if i % 3 else ("alice%d" % (i % 3)), "r%d" % i, payload=bytes([i & 255]) * (i % 70)) for i in range(n)]
    st, infos = hx.verify_proposal((hostlib.payload_encode(reqs), b"h", b"m", 0))
    assert st == hostlib.OK and len(infos) == n
    assert lib.sbvh_backend_msgs_batches(hx.v) == before + 1 and lib.sbvh_backend_keyed_batches(hx.v) == keyed
    for at in (0, 1, n - 1):
        bent = list(reqs)
        who = ("bob%d" % (at % 5)) if at % 3 else ("alice%d" % (at % 3))
        bent[at] = hx.request(who, "r%d" % at, payload=bytes([at & 255]) * (at % 70), corrupt=True)
        assert hx.verify_proposal((hostlib.payload_encode(bent), b"h", b"m", 0))[0] == hostlib.INVALID, at
    assert hx.verify_proposal((hostlib.payload_encode(reqs), b"h", b"m", 0))[0] == hostlib.OK
    return lib.sbvh_backend_msgs_batches(hx.v) - before


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_verifier_sends_unregistered_clients_through_the_raw_message_form(scheme, kind, oracle):
    """callback backend, with and without a key registry; P-256, Ed25519 (sbv_ed25519_verify_msgs in place of make_tuple_ed25519 per
    request) and secp256k1: the backend's CPU loop builds the tuples the host workers used to build, so the stand-in judges the same
    bytes: one callback batch of n tuples per proposal"""
    import hostlib
    from test_host_verifier import Harness
    lib = hostlib.load()
    for name in ("sbvo_p256_verify_batch", "sbvo_ed25519_verify_batch", "sbvo_k256_verify_batch"):      # the harness's callback hands them addresses
        getattr(oracle, name).argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    hx = Harness(lib, oracle, backend_kind=kind, wait_us=10, scheme=scheme)
    try:
        unregistered_clients(lib, hx, scheme)
        hx.batches.clear()
        assert proposals_of_unregistered_clients(lib, hx) == 5
        assert hx.batches == [150] * 5
    finally:
        hx.close()


def test_go_adapter_has_the_optional_interface():
    go = os.path.join(ROOT, "go", "gpuverifier")
    assert "type RawMessageVerifier interface" in open(os.path.join(go, "backend.go")).read()
    src = open(os.path.join(go, "backend_cgo.go")).read()
    assert "func (b *gpuBackend) VerifyMsgs(scheme Scheme, items []Item)" in src
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    called = {name for name, _, _ in check_cgo.calls(src)}
    assert {"sbv_p256_verify_msgs_sharded", "sbv_secp256k1_verify_msgs"} <= called

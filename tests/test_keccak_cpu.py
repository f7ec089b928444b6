"""CPU tier of Keccak-256 and the Ethereum-style addresses (include/sbv.h: sbv_keccak256_msgs, sbv_secp256k1_addresses,
sbv_secp256k1_recover_addresses; consensus_amd/csrc/keccak256_dev.h).

The model of tests/keccak_cases.py is first held to hashlib as SHA3-256 (the same code under the other domain byte) and to the four
published values of tests/golden/keccak256.json.  tests/emul/keccak_emul.cc then compiles the lane code the kernels are made of with
g++ and runs it as the kernels do, byte for byte against the model: messages, permutation states, the 64-byte forms, and the fused
recovery lane on a capped grid.  The host forms and Verifier::RecoverAddresses / Keccak256Batch on the CPU backend run the same cases.
The same source, built as a program of its own with AddressSanitizer and UBSan and every message in a heap buffer of exactly its
length, holds the rule that nothing outside msg[0 .. len) is read."""
import ctypes
import hashlib
import os
import subprocess
import sys

import pytest

import hostlib
import k256_py as kp
import k256_recover_cases as rc
import k256_sign_cases as sc
import keccak_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_SRC = os.path.join(HERE, "emul", "keccak_emul.cc")
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
LOW_S = rc.LOW_S


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


class Emul:
    """the emulator library behind the calling conventions of consensus_amd's wrappers"""

    def __init__(self):
        so = os.path.join(HERE, "emul", "libsbv_keccak_emul.so")
        if _stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", "-DSBV_K256_CHECK",
                                   EMUL_SRC, "-o", so])
        lib = ctypes.CDLL(so)
        V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        lib.sbvkk_msgs.argtypes = [ctypes.c_char_p, V, S, U, V]
        lib.sbvkk_msgs.restype = None
        lib.sbvkk_op.argtypes = [ctypes.c_int, ctypes.c_char_p, V, S]
        lib.sbvkk_hash64.argtypes = [ctypes.c_char_p, S, V]
        lib.sbvkk_hash64.restype = None
        lib.sbvkk_addresses.argtypes = [ctypes.c_char_p, S, V]
        lib.sbvkk_addresses.restype = None
        lib.sbvkk_recover_addr.argtypes = [ctypes.c_char_p] * 3 + [S, U, S, V, V]
        lib.sbvkk_recover_addr.restype = None
        self.lib = lib

    def msgs(self, blob, offs, domain=kc.KECCAK):
        n = len(offs) - 1
        out = ctypes.create_string_buffer(max(1, 32 * n))
        self.lib.sbvkk_msgs(blob, (ctypes.c_uint64 * (n + 1))(*offs), n, domain, out)
        return [out.raw[32 * i:32 * i + 32] for i in range(n)]

    def op(self, op, states):
        n = len(states)
        out = ctypes.create_string_buffer(200 * n)
        assert self.lib.sbvkk_op(op, b"".join(states), out, n) == 0
        return [out.raw[200 * i:200 * i + 200] for i in range(n)]

    def hash64(self, pubs):
        n = len(pubs) // 64
        out = ctypes.create_string_buffer(32 * n)
        self.lib.sbvkk_hash64(pubs, n, out)
        return out.raw

    def addresses(self, pubs):
        n = len(pubs) // 64
        out = ctypes.create_string_buffer(20 * n)
        self.lib.sbvkk_addresses(pubs, n, out)
        return out.raw

    def recover_addr(self, sigs, recid, digests, flags=0, lanes=1 << 17):
        n = len(recid)
        addrs, ok = ctypes.create_string_buffer(max(1, 20 * n)), ctypes.create_string_buffer(max(1, n))
        self.lib.sbvkk_recover_addr(sigs, recid, digests, n, flags, lanes, addrs, ok)
        return addrs.raw[:20 * n], ok.raw[:n]


@pytest.fixture(scope="module")
def emul():
    return Emul()


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_model_as_sha3_256_equals_hashlib_on_every_message_case():
    """the sponge, the padding at every residue of the rate and the permutation, under the domain byte hashlib has"""
    msgs = kc.messages()
    assert {len(m) for m in msgs} >= set(range(2 * kc.RATE + 10)) | {5 * kc.RATE}
    for m, d in zip(msgs, kc.message_digests(kc.SHA3)):
        assert d == hashlib.sha3_256(m).digest(), len(m)
    assert kc.message_digests(kc.KECCAK) != kc.message_digests(kc.SHA3)


def test_model_equals_the_four_known_answers():
    g = kc.golden()
    assert len(g["digests"]) == 2 and len(g["addresses"]) == 2
    for v in g["digests"]:
        assert kc.keccak256(bytes.fromhex(v["msg"])).hex() == v["keccak256"]
    for v in g["addresses"]:
        pub = sc.pub_bytes(kp.pt_mul(int(v["d"], 16), kp.G))
        assert kc.address(pub).hex() == v["address"]


def test_round_constants_and_offsets_of_the_model():
    """a few published values of the tables the model derives, so that a broken LFSR cannot hide behind a broken hashlib comparison"""
    rcs = kc.round_constants()
    assert rcs[0] == 1 and rcs[1] == 0x8082 and rcs[2] == 0x800000000000808A and rcs[23] == 0x8000000080008008
    rho = kc.rho_offsets()
    assert sorted(rho.values())[:3] == [0, 1, 2] and rho[(1, 0)] == 1 and rho[(0, 2)] == 3 and rho[(1, 1)] == 44 and len(rho) == 25


def test_message_starts_fall_on_every_residue():
    blob, offs = kc.packed_messages()
    assert len(offs) == len(kc.messages()) + 1 and offs[-1] == len(blob)
    assert {o % 8 for o in offs[:-1]} == set(range(8))


# ---- the lane code as host code --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", [kc.KECCAK, kc.SHA3])
def test_emulated_messages_equal_the_model(emul, domain):
    blob, offs = kc.packed_messages()
    got = emul.msgs(blob, offs, domain)
    want = kc.message_digests(domain)
    bad = [(i, len(kc.messages()[i])) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])


def test_emulated_messages_equal_hashlib_directly(emul):
    """the device code against hashlib with no model in between"""
    blob, offs = kc.packed_messages()
    got = emul.msgs(blob, offs, kc.SHA3)
    assert got == [hashlib.sha3_256(m).digest() for m in kc.messages()]


def test_emulated_known_answers(emul):
    g = kc.golden()
    msgs = [bytes.fromhex(v["msg"]) for v in g["digests"]]
    assert [d.hex() for d in emul.msgs(b"".join(msgs), [0, len(msgs[0]), len(msgs[0]) + len(msgs[1])])] == [v["keccak256"] for v in g["digests"]]
    assert emul.msgs(None, [0, 0, 0]) == [kc.keccak256(b"")] * 2                   # no buffer at all when every message is empty
    pubs = b"".join(sc.pub_bytes(kp.pt_mul(int(v["d"], 16), kp.G)) for v in g["addresses"])
    assert emul.addresses(pubs).hex() == "".join(v["address"] for v in g["addresses"])


def test_emulated_decreasing_offsets_write_zeros(emul):
    got = emul.msgs(b"abcdef", [0, 3, 1, 6])
    assert got == [kc.keccak256(b"abc"), bytes(32), kc.keccak256(b"bcdef")]


def test_emulated_permutation_equals_the_model(emul):
    got = emul.op(0, kc.states())
    bad = [i for i, (g, w) in enumerate(zip(got, kc.states_after())) if g != w]
    assert len(kc.states()) == 2 + 50 + 32 and not bad, bad[:8]
    assert emul.lib.sbvkk_op(1, kc.states()[0], ctypes.create_string_buffer(200), 1) != 0
    assert emul.lib.sbvkk_op(-1, kc.states()[0], ctypes.create_string_buffer(200), 1) != 0


def test_emulated_key_forms_equal_the_model(emul):
    keys = kc.key_cases()
    blob = b"".join(keys)
    d = emul.hash64(blob)
    assert [d[32 * i:32 * i + 32] for i in range(len(keys))] == [kc.keccak256(k) for k in keys]
    a = emul.addresses(blob)
    assert [a[20 * i:20 * i + 20] for i in range(len(keys))] == kc.key_addresses()


def _differ(idx, addrs, ok):
    exp = kc.recover_expected_all()
    return [(i, rc.cases()[i][0]) for k, i in enumerate(idx) if (addrs[20 * k:20 * k + 20], ok[k]) != exp[i]]


@pytest.mark.parametrize("flags", [0, LOW_S])
@pytest.mark.parametrize("lanes", [7, 64])
def test_emulated_fused_recovery_equals_the_model(emul, flags, lanes):
    """every case of k256_recover_cases under both flag settings, with few lanes so that strips are reused"""
    idx, sigs, rid, digs, want_addrs, want_ok = kc.recover_by_flags(flags)
    addrs, ok = emul.recover_addr(sigs, rid, digs, flags, lanes)
    bad = _differ(idx, addrs, ok)
    assert not bad, (len(bad), bad[:8])
    assert (addrs, ok) == (want_addrs, want_ok)
    refused = [k for k in range(len(idx)) if not ok[k]]
    # under the low-S flag the case set refuses four high s and the two scalar edges n - 1 and (n + 1) / 2
    assert len(refused) >= (60 if flags == 0 else 6) and all(addrs[20 * k:20 * k + 20] == bytes(20) for k in refused)


# ---- the host forms ------------------------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_model():
    host = hostlib.load()
    host.sbvh_keccak256.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    host.sbvh_keccak256.restype = None
    host.sbvh_k256_address.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    host.sbvh_k256_address.restype = None
    host.sbvh_k256_recover_address.argtypes = [ctypes.c_char_p, ctypes.c_uint8, ctypes.c_char_p, ctypes.c_char_p]
    d, a = ctypes.create_string_buffer(32), ctypes.create_string_buffer(20)
    for m, want in zip(kc.messages(), kc.message_digests()):
        host.sbvh_keccak256(m if m else None, len(m), d)
        assert d.raw == want, len(m)
    for k, want in zip(kc.key_cases(), kc.key_addresses()):
        host.sbvh_k256_address(k, a)
        assert a.raw == want
    exp = kc.recover_expected_all()
    seen = [0, 0]
    for i, (cat, rs, rid, h, flags) in enumerate(rc.cases()):
        if flags:
            continue                                                    # the host form has no low-S rule: flags = 0
        r = host.sbvh_k256_recover_address(rs, min(rid, 255), h, a)
        assert (a.raw, 1 if r == 0 else 0) == exp[i], (i, cat)
        seen[exp[i][1]] += 1
    assert seen[0] >= 60 and seen[1] >= 600


def _verifier_entries(host):
    host.sbvh_recover_addresses.argtypes = [hostlib.V, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    host.sbvh_keccak256_batch.argtypes = [hostlib.V, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]


def test_recover_addresses_on_the_cpu_backend():
    """Verifier::RecoverAddresses: 65-byte r | s | v with v as 0..3 and as 27..30, any other v refused; only under Scheme::SECP256K1"""
    host = hostlib.load()
    _verifier_entries(host)
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    idx, sigs, rid, digs, want_addrs, want_ok = kc.recover_by_flags(0)
    n = len(idx)
    for shift in (0, 27):
        blob = b"".join(sigs[64 * k:64 * k + 64] + bytes([rid[k] + shift if rid[k] <= 3 else rid[k]]) for k in range(n))
        h = host.sbvh_verifier_new_scheme(2, 1, 0, cb, None, 64, 50, 0)
        try:
            addrs, ok = ctypes.create_string_buffer(20 * n), ctypes.create_string_buffer(n)
            assert host.sbvh_recover_addresses(h, blob, digs, n, addrs, ok) == hostlib.OK
            assert not _differ(idx, addrs.raw, ok.raw) and (addrs.raw, ok.raw) == (want_addrs, want_ok)
            for v in (4, 26, 31, 200):                                  # a valid signature under a v that names no id
                one = sigs[:64] + bytes([v])
                assert host.sbvh_recover_addresses(h, one, digs[:32], 1, addrs, ok) == hostlib.OK and ok.raw[0] == 0 and addrs.raw[:20] == bytes(20)
            assert host.sbvh_recover_addresses(h, blob, digs, 0, addrs, ok) == hostlib.OK
        finally:
            host.sbvh_verifier_free(h)
    h = host.sbvh_verifier_new_scheme(0, 1, 0, cb, None, 64, 50, 0)      # a P-256 Verifier has no recovery
    try:
        assert host.sbvh_recover_addresses(h, sigs[:64] + b"\x00", digs[:32], 1, ctypes.create_string_buffer(20), ctypes.create_string_buffer(1)) == hostlib.INVALID
    finally:
        host.sbvh_verifier_free(h)


def test_keccak256_batch_on_the_cpu_backend():
    host = hostlib.load()
    _verifier_entries(host)
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    blob, offs = kc.packed_messages()
    n = len(offs) - 1
    h = host.sbvh_verifier_new_scheme(2, 1, 0, cb, None, 64, 50, 0)
    try:
        out = ctypes.create_string_buffer(32 * n)
        assert host.sbvh_keccak256_batch(h, blob, (ctypes.c_uint64 * (n + 1))(*offs), n, out) == hostlib.OK
        assert out.raw == b"".join(kc.message_digests())
        two = ctypes.create_string_buffer(64)
        assert host.sbvh_keccak256_batch(h, None, (ctypes.c_uint64 * 3)(0, 0, 0), 2, two) == hostlib.OK and two.raw == kc.keccak256(b"") * 2
        assert host.sbvh_keccak256_batch(h, blob, (ctypes.c_uint64 * 3)(1, 2, 3), 2, two) == hostlib.INVALID     # does not start at 0
        assert host.sbvh_keccak256_batch(h, blob, (ctypes.c_uint64 * 3)(0, 5, 3), 2, two) == hostlib.INVALID     # decreases
        assert host.sbvh_keccak256_batch(h, None, (ctypes.c_uint64 * 3)(0, 5, 8), 2, two) == hostlib.INVALID     # bytes but no buffer
        assert host.sbvh_keccak256_batch(h, blob, (ctypes.c_uint64 * 3)(0, 5, 3), 0, two) == hostlib.OK
    finally:
        host.sbvh_verifier_free(h)


# ---- declarations ----------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sbv_keccak256_msgs", "sbv_keccak256_msgs_stream", "sbv_secp256k1_addresses", "sbv_secp256k1_addresses_stream",
           "sbv_secp256k1_recover_addresses", "sbv_secp256k1_recover_addresses_stream", "sbv_debug_keccak_op")


def test_header_declares_the_entries_and_the_wrappers_exist():
    hdr = open(os.path.join(ROOT, "include", "sbv.h")).read()
    api = open(os.path.join(CSRC, "sbv_api.hip")).read()
    for name in ENTRIES:
        assert name + "(" in hdr and 'extern "C" int ' + name + "(" in api, name
    assert "_dev(" not in "".join(line for line in hdr.splitlines() if "keccak" in line or "addresses" in line)
    import consensus_amd as sbv
    for name in ("keccak256_msgs", "keccak256_msgs_stream", "secp256k1_addresses", "secp256k1_addresses_stream", "secp256k1_recover_addresses",
                 "secp256k1_recover_addresses_stream", "debug_keccak_op"):
        assert callable(getattr(sbv, name)), name


def test_cgo_call_site_matches_the_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    go = os.path.join(ROOT, "go", "gpuverifier")
    seen, problems, protos = check_cgo.check(go, os.path.join(ROOT, "include", "sbv.h"))
    assert not problems, problems
    called = {name for fn in os.listdir(go) if fn.endswith(".go") for name, _, _ in check_cgo.calls(open(os.path.join(go, fn)).read())}
    assert "sbv_secp256k1_recover_addresses" in called
    u8, u32, u64, V, S = ("uint8_t", True), ("uint32_t", False), ("uint64_t", True), ("void", True), ("size_t", False)
    assert protos["sbv_keccak256_msgs"] == [u8, u64, S, u8]
    assert protos["sbv_keccak256_msgs_stream"] == [V, V, S, V, V]
    assert protos["sbv_secp256k1_addresses"] == [u8, S, u8]
    assert protos["sbv_secp256k1_addresses_stream"] == [V, S, V, V]
    assert protos["sbv_secp256k1_recover_addresses"] == [u8, u8, u8, S, u32, u8, u8]
    assert protos["sbv_secp256k1_recover_addresses_stream"] == [V, V, V, S, u32, V, V, V, S, V]
    assert protos["sbv_debug_keccak_op"] == [("int", False), u8, u8, S]
    src = open(os.path.join(go, "backend.go")).read()
    assert "type K256AddressRecoverer interface" in src and "RecoverAddressesSecp256k1(" in src


# ---- the read-bounds rule --------------------------------------------------------------------------------------------------------------
def test_sanitizer_build_hashes_as_a_program_of_its_own(tmp_path):
    """the same source with its own main under AddressSanitizer and UBSan, one run: every message from a heap buffer of exactly its
    length under both domain bytes, the states, the key forms into exactly 20 bytes, and every recovery case with 5 lanes (strips
    reused) and with one lane per case on exactly allocated strips"""
    exe = str(tmp_path / "keccak_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-DSBV_K256_CHECK", "-Wno-misleading-indentation", EMUL_SRC, "-o", exe])
    rows = []
    for domain in (kc.KECCAK, kc.SHA3):
        for m, d in zip(kc.messages(), kc.message_digests(domain)):
            rows.append(("M", "%02x" % domain, m.hex() or "-", d.hex()))
    for s, t in zip(kc.states(), kc.states_after()):
        rows.append(("S", s.hex(), t.hex()))
    for k, a in zip(kc.key_cases(), kc.key_addresses()):
        rows.append(("K", k.hex(), kc.keccak256(k).hex(), a.hex()))
    for (cat, rs, rid, h, flags), (addr, ok) in zip(rc.cases(), kc.recover_expected_all()):
        rows.append(("R", rs.hex(), "%02x" % min(rid, 255), h.hex(), "%02x" % flags, addr.hex() if ok else "-"))
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(r) + "\n" for r in rows))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases," % len(rows) in r.stdout and " 0 differ" in r.stdout, r.stdout + r.stderr

"""CPU tier of the secp256k1 batch signer (include/sbv.h: sbv_secp256k1_sign_batch, sbv_secp256k1_pubkeys; consensus_amd/csrc/k256_sign.h).

tests/emul/k256_sign_emul.cc compiles the lanes the kernels are made of with g++ and runs them as the kernels do.  The signature is
deterministic, so every byte is held to the community RFC 6979 known answers and to an independent signer made of Python's hmac /
hashlib and oracle/k256_py.py; the host signer and the C oracle are held to the same signer on the same cases; OpenSSL and the C oracle
verify every signature; a Python recovery returns the signer's key from every recovery id.  The retry path of the nonce and the
x >= n branch, which no real input reaches, are held through unit operations 1 and 3.  The same source, built as a program of its own
with AddressSanitizer and UBSan, runs the cases once."""
import ctypes
import os
import subprocess
import sys

import pytest

import hostlib
import k256_py as kp
import k256_sign_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL_SRC = os.path.join(HERE, "emul", "k256_sign_emul.cc")
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
N, LOW_S = cases.N, cases.LOW_S


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


class Emul:
    """the emulator library behind the calling conventions of consensus_amd's wrappers"""

    def __init__(self):
        so = os.path.join(HERE, "emul", "libsbv_k256_sign_emul.so")
        if _stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", "-DSBV_K256_CHECK",
                                   EMUL_SRC, "-o", so])
        lib = ctypes.CDLL(so)
        V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
        lib.sbvk256sign_sign.argtypes = [ctypes.c_char_p, U, V, ctypes.c_char_p, S, U, V, V, V]
        lib.sbvk256sign_sign.restype = None
        lib.sbvk256sign_pubkeys.argtypes = [ctypes.c_char_p, S, V, V]
        lib.sbvk256sign_pubkeys.restype = None
        lib.sbvk256sign_op.argtypes = [ctypes.c_int, ctypes.c_char_p, V, S]
        lib.sbvk256sign_with_nonce.argtypes = [ctypes.c_char_p] * 3 + [U, V, V]
        self.lib = lib

    def sign(self, keys, digests, key_index=None, flags=0):
        n, nk = len(digests) // 32, len(keys) // 32
        idx = (ctypes.c_uint32 * n)(*key_index) if key_index is not None else None
        sigs, rid, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n), ctypes.create_string_buffer(n)
        self.lib.sbvk256sign_sign(keys, nk, idx, digests, n, flags, sigs, rid, ok)
        return sigs.raw, rid.raw, ok.raw

    def pubkeys(self, keys):
        m = len(keys) // 32
        pubs, ok = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(m)
        self.lib.sbvk256sign_pubkeys(keys, m, pubs, ok)
        return pubs.raw, ok.raw

    def op(self, op, records):
        n = len(records)
        out = ctypes.create_string_buffer(cases.OP_OUT * n)
        assert self.lib.sbvk256sign_op(op, b"".join(records), out, n) == 0
        return [out.raw[cases.OP_OUT * i:cases.OP_OUT * (i + 1)] for i in range(n)]

    def with_nonce(self, d, k, e, flags=0):
        rs, rid = ctypes.create_string_buffer(64), ctypes.create_string_buffer(1)
        ok = self.lib.sbvk256sign_with_nonce(cases.be32(d), cases.be32(k), cases.be32(e), flags, rs, rid)
        return (rs.raw, rid.raw[0]) if ok else None


@pytest.fixture(scope="module")
def emul():
    return Emul()


@pytest.fixture(scope="module")
def signed(emul):
    """sign_cases() through the emulator under both flag settings, case i with key i: {flags: (sigs, recid, ok)}"""
    pairs = cases.sign_cases()
    keys, digests = b"".join(cases.be32(d) for d, _ in pairs), b"".join(h for _, h in pairs)
    return {f: emul.sign(keys, digests, None, f) for f in (0, LOW_S)}


def _sig(blob, i):
    return blob[64 * i:64 * i + 64]


def test_community_known_answers(emul):
    vs = cases.vectors()
    assert len(vs) == 4 and all(v["s_was_high"] for v in vs)
    keys, digests = b"".join(v["d"] for v in vs), b"".join(v["digest"] for v in vs)
    first = emul.op(0, [cases.op_record(v["d"], v["digest"]) for v in vs])
    assert [o[:32] for o in first] == [v["k"] for v in vs]
    low, low_rid, ok = emul.sign(keys, digests, None, LOW_S)
    assert ok == b"\x01" * 4 and [_sig(low, i) for i in range(4)] == [v["sig"] for v in vs]
    raw, raw_rid, ok = emul.sign(keys, digests, None, 0)
    assert ok == b"\x01" * 4
    for i, v in enumerate(vs):
        s = int.from_bytes(v["sig"][32:], "big")
        assert _sig(raw, i) == v["sig"][:32] + cases.be32(N - s)
        assert raw_rid[i] ^ low_rid[i] == 1


def test_emulator_equals_the_independent_signer(signed):
    pairs = cases.sign_cases()
    assert len(pairs) == 300 + len(cases.EDGE_KEYS) * len(cases.EDGE_DIGESTS)
    for flags in (0, LOW_S):
        sigs, rid, ok = signed[flags]
        assert ok == b"\x01" * len(pairs)
        want = cases.sign_expected(flags)
        bad = [i for i in range(len(pairs)) if (_sig(sigs, i), rid[i]) != want[i]]
        assert not bad, (flags, len(bad), bad[:8])


def test_host_signer_and_c_oracle_equal_the_independent_signer(oracle):
    host = hostlib.load()
    host.sbvh_k256_sign_rfc6979.argtypes = [ctypes.c_char_p] * 3
    oracle.sbvo_k256_sign.argtypes = [ctypes.c_char_p] * 4
    out = ctypes.create_string_buffer(64)
    want = cases.sign_expected(0)
    for i, (d, h) in enumerate(cases.sign_cases()):
        assert host.sbvh_k256_sign_rfc6979(cases.be32(d), h, out) == 0 and out.raw == want[i][0], i
        k = next(kb for kb, _, _ in cases.drbg_states(d, h) if 1 <= int.from_bytes(kb, "big") < N)
        assert oracle.sbvo_k256_sign(cases.be32(d), k, h, out) == 0 and out.raw == want[i][0], i
        r, s = kp.sign(d, int.from_bytes(k, "big"), h)
        assert cases.be32(r) + cases.be32(s) == want[i][0], i
    assert host.sbvh_k256_sign_rfc6979(bytes(32), bytes(32), out) != 0 and host.sbvh_k256_sign_rfc6979(cases.be32(N), bytes(32), out) != 0


def test_openssl_and_the_c_oracle_verify_every_signature(signed, oracle, openssl_check):
    oracle.sbvo_k256_verify_tuple.argtypes = [ctypes.c_char_p]
    openssl_check.sbvssl_k256_verify_tuple.argtypes = [ctypes.c_char_p]
    pairs = cases.sign_cases()
    _, pubs = cases_pubs()
    for flags in (0, LOW_S):
        sigs = signed[flags][0]
        for i, (d, h) in enumerate(pairs):
            t = _sig(sigs, i) + h + pubs[i]
            assert oracle.sbvo_k256_verify_tuple(t) == 1 and openssl_check.sbvssl_k256_verify_tuple(t) == 1, (flags, i)
            bit = 1 << (i % 250)                                        # one bit of s, a different one per case
            s2 = int.from_bytes(t[32:64], "big") ^ bit
            t2 = t[:32] + cases.be32(s2) + t[64:]
            assert oracle.sbvo_k256_verify_tuple(t2) == 0 and openssl_check.sbvssl_k256_verify_tuple(t2) == 0, (flags, i)


_PUBS = []


def cases_pubs():
    """the public keys of sign_cases() from the big-integer twin, once"""
    if not _PUBS:
        memo = {}
        for d, _ in cases.sign_cases():
            if d not in memo:
                memo[d] = cases.pub_bytes(kp.pt_mul(d, kp.G))
            _PUBS.append(memo[d])
    return None, _PUBS


def test_recovery_id_returns_the_signers_key(signed):
    _, pubs = cases_pubs()
    for flags in (0, LOW_S):
        sigs, rid, _ = signed[flags]
        for i, (d, h) in enumerate(cases.sign_cases()):
            assert rid[i] < 2                                           # bit 1 needs x >= n: see the op 3 test
            if flags and (_sig(sigs, i), rid[i]) == (_sig(signed[0][0], i), signed[0][1][i]):
                continue                                                # s was low already: the very signature recovered above
            q = cases.recover(_sig(sigs, i), rid[i], h)
            assert q is not None and cases.pub_bytes(q) == pubs[i], (flags, i)
            if i % 16 == 0:                                             # and the other parity recovers another key
                assert cases.pub_bytes(cases.recover(_sig(sigs, i), rid[i] ^ 1, h)) != pubs[i], (flags, i)


def test_low_s_halves_and_flips_the_parity(signed):
    (raw, raw_rid, _), (low, low_rid, _) = signed[0], signed[LOW_S]
    same = flipped = 0
    for i in range(len(cases.sign_cases())):
        r0, s0 = _sig(raw, i)[:32], int.from_bytes(_sig(raw, i)[32:], "big")
        r1, s1 = _sig(low, i)[:32], int.from_bytes(_sig(low, i)[32:], "big")
        assert r0 == r1 and 1 <= s1 <= cases.HALF, i
        if s0 <= cases.HALF:
            assert (s1, low_rid[i]) == (s0, raw_rid[i]), i
            same += i < 300
        else:
            assert (s1, low_rid[i]) == (N - s0, raw_rid[i] ^ 1), i
            flipped += i < 300
    assert same >= 75 and flipped >= 75, (same, flipped)             # neither branch can hide among the seeded cases


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_unit_operations_against_python(emul, op):
    ins, want = cases.all_op_cases()[op]
    got = emul.op(op, ins)
    bad = [i for i in range(len(ins)) if got[i] != want[i]]
    assert not bad, (op, len(bad), bad[:8])
    assert emul.lib.sbvk256sign_op(4, ins[0], ctypes.create_string_buffer(cases.OP_OUT), 1) != 0
    assert emul.lib.sbvk256sign_op(-1, ins[0], ctypes.create_string_buffer(cases.OP_OUT), 1) != 0


def test_op3_reaches_the_branches_no_nonce_reaches(emul):
    d, k, e = 0x1234567, 0x89ABCDEF, 0x1357
    for x in (N - 1, N, N + 1, kp.P - 1):
        for y_odd in (0, 1):
            out = emul.op(3, [cases.op_record(x, y_odd, d, k, e, 0)])[0]
            if x == N:
                assert out == bytes(cases.OP_OUT)                       # r = 0
                continue
            assert out[96:] == cases.be32(1) and out[:32] == cases.be32(x % N)
            assert out[95] == (y_odd | (2 if x >= N else 0))
    r = 0xFEDCBA987654321
    e0 = (N - r * d % N) % N                                            # e + r d = 0 mod n: s = 0
    assert emul.op(3, [cases.op_record(r, 0, d, k, e0, 0)])[0] == bytes(cases.OP_OUT)
    assert emul.op(3, [cases.op_record(r, 0, d, k, (e0 + 1) % N, 0)])[0][96:] == cases.be32(1)


def test_with_nonce_rejects_k_outside_the_group(emul):
    d, e = 0x1234567, 0x1357
    for k in (0, N, 2**256 - 1):
        assert emul.with_nonce(d, k, e) is None, hex(k)
    for k in (1, N - 1):
        for flags in (0, LOW_S):
            R = kp.pt_mul(k, kp.G)
            r, s, rid = cases.finish(R[0], R[1] & 1, d, k, e, flags)
            assert emul.with_nonce(d, k, e, flags) == (cases.be32(r) + cases.be32(s), rid), (hex(k), flags)


def test_public_keys(emul):
    host = hostlib.load()
    host.sbvh_k256_pubkey.argtypes = [ctypes.c_char_p] * 2
    keys, want = cases.pubkey_cases()
    assert len(keys) == len(cases.EDGE_KEYS) + 100
    blob = b"".join(cases.be32(d) for d in keys) + bytes(32) + cases.be32(N)
    pubs, ok = emul.pubkeys(blob)
    assert ok == b"\x01" * len(keys) + b"\x00\x00" and pubs[64 * len(keys):] == bytes(128)
    q = ctypes.create_string_buffer(64)
    for i, d in enumerate(keys):
        assert pubs[64 * i:64 * i + 64] == want[i], i
        assert host.sbvh_k256_pubkey(cases.be32(d), q) == 0 and q.raw == want[i], i
    assert host.sbvh_k256_pubkey(bytes(32), q) != 0 and host.sbvh_k256_pubkey(cases.be32(N), q) != 0


def test_rejected_lanes_write_zeros_and_leave_their_neighbours_alone(emul):
    good = [d for d, _ in cases.sign_cases()[:3]]
    keys = b"".join(cases.be32(d) for d in good + [0, N, 2**256 - 1])
    digests = b"".join(h for _, h in cases.sign_cases()[:9])
    idx = [0, 1, 3, 2, 4, 5, 6, 0xFFFFFFFF, 1]
    sigs, rid, ok = emul.sign(keys, digests, idx, LOW_S)
    for i, k in enumerate(idx):
        if k < 3:
            rs, r, _ = cases.py_sign(good[k], digests[32 * i:32 * i + 32], LOW_S)
            assert (ok[i], _sig(sigs, i), rid[i]) == (1, rs, r), i
        else:
            assert (ok[i], _sig(sigs, i), rid[i]) == (0, bytes(64), 0), i
    sigs, rid, ok = emul.sign(keys[:96], digests, None, 0)               # a null index: key i % n_keys
    assert ok == b"\x01" * 9
    for i in range(9):
        assert (_sig(sigs, i), rid[i]) == cases.py_sign(good[i % 3], digests[32 * i:32 * i + 32], 0)[:2], i


def test_sanitizer_build_signs_as_a_program_of_its_own(tmp_path, signed):
    """the same source with its own main under AddressSanitizer and UBSan: the known answers, the sign cases and three rejected keys, one run"""
    exe = str(tmp_path / "k256_sign_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-DSBV_K256_CHECK", "-Wno-misleading-indentation", EMUL_SRC, "-o", exe])
    _, pubs = cases_pubs()
    rows = []
    for v in cases.vectors():
        s = int.from_bytes(v["sig"][32:], "big")
        rid = cases.py_sign(int.from_bytes(v["d"], "big"), v["digest"], LOW_S)[1]
        pub = cases.pub_bytes(kp.pt_mul(int.from_bytes(v["d"], "big"), kp.G))
        rows.append((v["d"].hex(), v["digest"].hex(), (v["sig"][:32] + cases.be32(N - s)).hex(), "%02x" % (rid ^ 1), v["sig"].hex(), "%02x" % rid, pub.hex()))
    want0, want1 = cases.sign_expected(0), cases.sign_expected(LOW_S)
    for i, (d, h) in enumerate(cases.sign_cases()):
        rows.append((cases.be32(d).hex(), h.hex(), want0[i][0].hex(), "%02x" % want0[i][1], want1[i][0].hex(), "%02x" % want1[i][1], pubs[i].hex()))
    for d in (0, N, 2**256 - 1):
        rows.append((cases.be32(d).hex(), "22" * 32, "-", "00", "-", "00", "-"))
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(r) + "\n" for r in rows))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 differ" % len(rows) in r.stdout, r.stdout + r.stderr


def test_cgo_call_site_matches_the_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_cgo
    go = os.path.join(ROOT, "go", "gpuverifier")
    seen, problems, protos = check_cgo.check(go, os.path.join(ROOT, "include", "sbv.h"))
    assert not problems, problems
    called = {name for fn in os.listdir(go) if fn.endswith(".go") for name, _, _ in check_cgo.calls(open(os.path.join(go, fn)).read())}
    assert "sbv_secp256k1_sign_batch" in called
    u8, u32 = ("uint8_t", True), ("uint32_t", False)
    assert protos["sbv_secp256k1_sign_batch"] == [u8, u32, ("uint32_t", True), u8, ("size_t", False), u32, u8, u8, u8]
    V = ("void", True)
    assert protos["sbv_secp256k1_sign_batch_stream"] == [V, u32, V, V, ("size_t", False), u32, V, V, V, V]
    assert protos["sbv_secp256k1_pubkeys"] == [u8, ("size_t", False), u8, u8]
    assert protos["sbv_secp256k1_pubkeys_stream"] == [V, ("size_t", False), V, V, V]
    assert protos["sbv_debug_secp256k1_sign_op"] == [("int", False), u8, u8, ("size_t", False)]

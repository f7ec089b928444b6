"""Batch signing (consensus_amd/csrc/p256_sign.h), CPU tier: the per-lane device source compiled for the
host (tests/emul), pinned on the RFC 6979 A.2.5 known answers and diffed against the host Signer (consensus_amd/host,
sign_rfc6979) and the oracle's verifier on random keys and digests."""
import ctypes
import hashlib

import numpy as np
import pytest

import hostlib
from test_emul_device_algo import emul  # noqa: F401  (fixture: builds tests/emul/libsbv_emul.so)

N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


@pytest.fixture(scope="module")
def host():
    return hostlib.load()


def sign(emul, keys: bytes, digests: bytes, index=None):
    n, nk = len(digests) // 32, len(keys) // 32
    sigs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
    idx = None if index is None else (ctypes.c_uint32 * n)(*index)
    emul.sbve_p256_sign_batch.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
                                          ctypes.c_char_p, ctypes.c_char_p]
    emul.sbve_p256_sign_batch.restype = None
    emul.sbve_p256_sign_batch(keys, nk, idx, digests, n, sigs, ok)
    return sigs.raw, ok.raw


def test_rfc6979_known_answers(emul, rfc6979):
    d = bytes.fromhex(rfc6979["private_key"])
    kat = [s for s in rfc6979["signatures"] if s["hash_alg"] == "sha256"]
    assert len(kat) == 2
    sigs, ok = sign(emul, d, b"".join(bytes.fromhex(s["hash"]) for s in kat))
    assert ok == b"\x01\x01"
    for i, s in enumerate(kat):
        assert sigs[64 * i:64 * i + 64].hex() == s["r"] + s["s"], s["message"]


def test_matches_the_host_signer_and_verifies_under_the_oracle(emul, host, oracle):
    rng = np.random.default_rng(6979)
    nk, n = 5, 48
    keys = b"".join(int.to_bytes(int.from_bytes(rng.bytes(32), "big") % (N_ORDER - 1) + 1, 32, "big") for _ in range(nk))
    digests = b"".join(hashlib.sha256(b"msg %d" % i).digest() for i in range(n - 3))
    digests += b"\x00" * 32 + b"\xff" * 32 + N_ORDER.to_bytes(32, "big")            # e = 0, e >= N (reduced once), e = N
    index = [int(x) for x in rng.integers(0, nk, n)]
    sigs, ok = sign(emul, keys, digests, index)
    assert ok == b"\x01" * n
    for i in range(n):
        d = keys[32 * index[i]:32 * index[i] + 32]
        rs = ctypes.create_string_buffer(64)
        assert host.sbvh_sign_rfc6979(d, digests[32 * i:32 * i + 32], rs) == 0
        assert sigs[64 * i:64 * i + 64] == rs.raw, i
        q = ctypes.create_string_buffer(64)
        assert host.sbvh_pubkey(d, q) == 0
        assert oracle.sbvo_p256_verify_tuple(sigs[64 * i:64 * i + 64] + digests[32 * i:32 * i + 32] + q.raw) == 1
    # default key choice: i % n_keys
    sigs2, ok2 = sign(emul, keys, digests[:32 * 7])
    for i in range(7):
        rs = ctypes.create_string_buffer(64)
        host.sbvh_sign_rfc6979(keys[32 * (i % nk):32 * (i % nk) + 32], digests[32 * i:32 * i + 32], rs)
        assert sigs2[64 * i:64 * i + 64] == rs.raw


def test_keys_outside_the_scalar_range_and_bad_indices_produce_nothing(emul):
    keys = b"\x00" * 32 + N_ORDER.to_bytes(32, "big") + b"\xff" * 32 + (1).to_bytes(32, "big") + (N_ORDER - 1).to_bytes(32, "big")
    digests = hashlib.sha256(b"x").digest() * 6
    sigs, ok = sign(emul, keys, digests, [0, 1, 2, 3, 4, 5])
    assert ok == b"\x00\x00\x00\x01\x01\x00"                                           # index 5 does not exist
    for i in (0, 1, 2, 5):
        assert sigs[64 * i:64 * i + 64] == b"\x00" * 64
    assert sigs[64 * 3:64 * 4] != b"\x00" * 64 and sigs[64 * 4:64 * 5] != b"\x00" * 64


# ---- the independent signer (tests/p256_sign_cases.py): hmac / hashlib, Python integers and oracle/p256_py.py ---------------------------
import os  # noqa: E402
import subprocess  # noqa: E402

import p256_sign_cases as cases  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N = cases.N


def _sig(blob, i):
    return blob[64 * i:64 * i + 64]


def _host_sign(host, d, digest):
    rs = ctypes.create_string_buffer(64)
    return rs.raw if host.sbvh_sign_rfc6979(cases.be32(d), digest, rs) == 0 else None


@pytest.fixture(scope="module")
def signed(emul):
    """sign_cases() through the emulator, case i under key i"""
    keys, digests = cases.blobs(cases.sign_cases())
    return sign(emul, keys, digests)


def test_emulator_equals_the_independent_signer(signed):
    pairs, want = cases.sign_cases(), cases.sign_expected()
    assert len(pairs) == 300 + len(cases.EDGE_KEYS) * len(cases.EDGE_DIGESTS)
    sigs, ok = signed
    assert ok == b"\x01" * len(pairs)
    bad = [i for i in range(len(pairs)) if _sig(sigs, i) != want[i]]
    assert not bad, (len(bad), bad[:8])


def test_host_signer_equals_the_independent_signer(host):
    want = cases.sign_expected()
    bad = [i for i, (d, h) in enumerate(cases.sign_cases()) if _host_sign(host, d, h) != want[i]]
    assert not bad, (len(bad), bad[:8])
    for d in cases.REJECTED_KEYS:
        assert _host_sign(host, d, bytes(32)) is None, hex(d)


def test_oracle_and_openssl_accept_every_signature_and_reject_a_flipped_digest_bit(signed, oracle, openssl_check):
    sigs, _ = signed
    for i, (d, h) in enumerate(cases.sign_cases()):
        t = _sig(sigs, i) + h + cases.pubkey(d)
        assert oracle.sbvo_p256_verify_tuple(t) == 1 and openssl_check.sbvssl_p256_verify_tuple(t) == 1, i
        bit = i % 256                                                  # 2^bit is no multiple of N: e changes with it
        h2 = cases.be32(int.from_bytes(h, "big") ^ (1 << bit))
        t2 = t[:64] + h2 + t[96:]
        assert oracle.sbvo_p256_verify_tuple(t2) == 0 and openssl_check.sbvssl_p256_verify_tuple(t2) == 0, i


def test_retry_vector_takes_the_second_candidate(emul, host, oracle):
    """RFC 6979 section 3.2 h: the first candidate is >= N, K and V are updated over V || 00 (the 33-byte shape of hmac_v_tag) and the
    second candidate signs.  No seeded input reaches this: the chance is 2^-32 per signature."""
    v = cases.retry_vector()
    d, h = cases.be32(v["d"]), v["digest"]
    assert cases.py_sign(v["d"], h) == (v["sig"], 1, 1)
    assert sign(emul, d, h) == (v["sig"], b"\x01")
    assert _host_sign(host, v["d"], h) == v["sig"]
    rs = ctypes.create_string_buffer(b"\x5a" * 64, 64)
    assert host.sbvh_sign_with_nonce(d, cases.be32(v["k1"]), h, rs) != 0 and rs.raw == b"\x5a" * 64
    assert host.sbvh_sign_with_nonce(d, cases.be32(v["k2"]), h, rs) == 0 and rs.raw == v["sig"]
    assert oracle.sbvo_p256_verify_tuple(v["sig"] + h + cases.pubkey(v["d"])) == 1
    # between ordinary lanes, under an explicit index
    pairs = cases.sign_cases()[:4]
    keys, digests = cases.blobs(pairs[:2] + [(v["d"], h)] + pairs[2:])
    sigs, ok = sign(emul, keys, digests, [0, 1, 2, 3, 4])
    assert ok == b"\x01" * 5 and _sig(sigs, 2) == v["sig"]
    assert [_sig(sigs, i) for i in (0, 1, 3, 4)] == cases.sign_expected()[:4]


def _with_nonce(emul, d, k, e):
    emul.sbve_p256_sign_with_nonce.argtypes = [ctypes.c_char_p] * 4
    rs = ctypes.create_string_buffer(64)
    return rs.raw if emul.sbve_p256_sign_with_nonce(cases.be32(d), cases.be32(k), cases.be32(e), rs) else None


def test_with_nonce_refuses_k_outside_the_group_and_signs_at_its_ends(emul, host):
    d, e = 0x1234567, 0x1357
    rs = ctypes.create_string_buffer(64)
    for k in (0, N, 2**256 - 1):
        assert _with_nonce(emul, d, k, e) is None, hex(k)
        assert host.sbvh_sign_with_nonce(cases.be32(d), cases.be32(k), cases.be32(e), rs) != 0, hex(k)
    for k in (1, N - 1):
        r, s = cases.finish(cases.pp.pt_mul(k, cases.pp.G)[0], d, k, e)
        assert _with_nonce(emul, d, k, e) == cases.be32(r) + cases.be32(s), hex(k)
        assert host.sbvh_sign_with_nonce(cases.be32(d), cases.be32(k), cases.be32(e), rs) == 0 and rs.raw == cases.be32(r) + cases.be32(s), hex(k)
    v = cases.retry_vector()
    e = int.from_bytes(v["digest"], "big") % N
    assert _with_nonce(emul, v["d"], v["k1"], e) is None and _with_nonce(emul, v["d"], v["k2"], e) == v["sig"]


def test_rejected_lanes_write_zeros_and_leave_their_neighbours_alone(emul):
    good = [d for d, _ in cases.sign_cases()[:3]]
    keys = b"".join(cases.be32(d) for d in good + cases.REJECTED_KEYS)
    digests = b"".join(h for _, h in cases.sign_cases()[:10])
    idx = [0, 1, 3, 2, 4, 5, 0, 6, 0xFFFFFFFF, 1]                       # d = 0, N, 2^256 - 1; n_keys and 0xFFFFFFFF as an index
    sigs, ok = sign(emul, keys, digests, idx)
    for i, k in enumerate(idx):
        if k < 3:
            assert (ok[i], _sig(sigs, i)) == (1, cases.py_sign(good[k], digests[32 * i:32 * i + 32])[0]), i
        else:
            assert (ok[i], _sig(sigs, i)) == (0, bytes(64)), i
    sigs, ok = sign(emul, keys[:96], digests)                           # a null index: key i % n_keys
    assert ok == b"\x01" * 10
    for i in range(10):
        assert _sig(sigs, i) == cases.py_sign(good[i % 3], digests[32 * i:32 * i + 32])[0], i


def test_sanitizer_build_signs_as_a_program_of_its_own(tmp_path, rfc6979):
    """the emulator source with its own main under AddressSanitizer and UBSan: the known answers, the sign cases, the retry vector and
    three rejected keys, one run; nothing is loaded into an interpreter"""
    src = os.path.join(HERE, "emul", "emul.cc")
    exe = str(tmp_path / "emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-DSBV_F29_CHECK", "-DSBV_F25_CHECK", "-DSBV_K256_CHECK", "-Wno-misleading-indentation", src, "-o", exe])
    rows = [(rfc6979["private_key"], s["hash"], s["r"] + s["s"]) for s in rfc6979["signatures"] if s["hash_alg"] == "sha256"]
    assert len(rows) == 2
    want = cases.sign_expected()
    rows += [(cases.be32(d).hex(), h.hex(), want[i].hex()) for i, (d, h) in enumerate(cases.sign_cases())]
    v = cases.retry_vector()
    rows.append((cases.be32(v["d"]).hex(), v["digest"].hex(), v["sig"].hex()))
    rows += [(cases.be32(d).hex(), "22" * 32, "-") for d in cases.REJECTED_KEYS]
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(r) + "\n" for r in rows))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 differ" % len(rows) in r.stdout, r.stdout + r.stderr

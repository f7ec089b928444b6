"""CPU tier of the Ed25519 batch signer (include/sbv.h: sbv_ed25519_expand_keys, sbv_ed25519_sign_msgs; consensus_amd/csrc/ed25519_sign.h).

tests/emul/ed_sign_emul.cc compiles the lanes the kernels are made of with g++ and runs them as the kernels do.  The signature is
deterministic, so every byte is held to RFC 8032 and to four independent signers; the pieces (sha512_head_msg, sc25519_muladd,
sc25519_reduce256, encode([s]B)) are held to hashlib, Python integers and oracle/ed25519_py.py.  The same source, built as a program of
its own with AddressSanitizer and UBSan, signs the RFC vectors and a few hundred mixed-length messages once."""
import ctypes
import ctypes.util
import hashlib
import os
import subprocess

import pytest

import ed25519_py as ed
import ed_sign_cases as cases
import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_SRC = os.path.join(HERE, "emul", "ed_sign_emul.cc")
CSRC = os.path.join(HERE, "..", "consensus_amd", "csrc")


def _stale(target):
    deps = [EMUL_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(HERE, "emul", "libsbv_ed_sign_emul.so")
    if _stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", EMUL_SRC, "-o", so])
    lib = ctypes.CDLL(so)
    V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.sbvedsign_expand.argtypes = [ctypes.c_char_p, S, V, V]
    lib.sbvedsign_expand.restype = None
    lib.sbvedsign_sign.argtypes = [ctypes.c_char_p, U, V, ctypes.c_char_p, V, S, V, V]
    lib.sbvedsign_sign.restype = None
    lib.sbvedsign_op.argtypes = [ctypes.c_int, ctypes.c_char_p, V, S]
    lib.sbvedsign_sha512_head_msg.argtypes = [ctypes.c_char_p, S, ctypes.c_char_p, S, V]
    lib.sbvedsign_sha512_head_msg.restype = None
    return lib


def _expand(emul, seeds):
    m = len(seeds)
    exp, pks = ctypes.create_string_buffer(96 * m), ctypes.create_string_buffer(32 * m)
    emul.sbvedsign_expand(b"".join(seeds), m, exp, pks)
    return exp.raw, [pks.raw[32 * i:32 * i + 32] for i in range(m)]


def _sign(emul, expanded, msgs, key_index=None):
    n, n_keys = len(msgs), len(expanded) // 96
    payload, off = cases.pack_messages(msgs)
    moff = (ctypes.c_uint64 * (n + 1))(*off)
    idx = (ctypes.c_uint32 * n)(*key_index) if key_index is not None else None
    sigs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
    emul.sbvedsign_sign(expanded, n_keys, idx, payload + b"\0", moff, n, sigs, ok)
    return [sigs.raw[64 * i:64 * i + 64] for i in range(n)], list(ok.raw)


def _op(emul, op, blobs):
    n = len(blobs)
    out = ctypes.create_string_buffer(32 * n)
    assert emul.sbvedsign_op(op, b"".join(blobs), out, n) == 0
    return [out.raw[32 * i:32 * i + 32] for i in range(n)]


def test_rfc8032_vectors_byte_for_byte(emul):
    vs = cases.rfc_vectors()
    assert [v["name"] for v in vs] == ["rfc8032_test1", "rfc8032_test2", "rfc8032_test3", "rfc8032_test_sha_abc"]
    expanded, pks = _expand(emul, [v["seed"] for v in vs])
    assert pks == [v["pk"] for v in vs]
    for i, v in enumerate(vs):                                         # the record: a mod L | prefix | A_enc
        a, prefix = ed.secret_expand(v["seed"])
        assert expanded[96 * i:96 * i + 96] == cases.le32(a % ed.L) + prefix + v["pk"]
    sigs, ok = _sign(emul, expanded, [v["msg"] for v in vs], list(range(len(vs))))
    assert ok == [1] * len(vs) and sigs == [v["sig"] for v in vs]


class _OpenSSL:
    """EVP Ed25519 through ctypes, when libcrypto loads"""

    def __init__(self):
        name = ctypes.util.find_library("crypto")
        self.lib = ctypes.CDLL(name) if name else None
        if self.lib is not None and not hasattr(self.lib, "EVP_PKEY_new_raw_private_key"):
            self.lib = None
        if self.lib is None:
            return
        c, V, S = self.lib, ctypes.c_void_p, ctypes.c_size_t
        c.EVP_PKEY_new_raw_private_key.restype = V
        c.EVP_PKEY_new_raw_private_key.argtypes = [ctypes.c_int, V, ctypes.c_char_p, S]
        c.EVP_MD_CTX_new.restype = V
        c.EVP_DigestSignInit.argtypes = [V, V, V, V, V]
        c.EVP_DigestSign.argtypes = [V, ctypes.c_char_p, ctypes.POINTER(S), ctypes.c_char_p, S]
        c.EVP_MD_CTX_free.argtypes = [V]
        c.EVP_PKEY_free.argtypes = [V]

    def sign(self, seed, msg):
        c = self.lib
        key = c.EVP_PKEY_new_raw_private_key(1087, None, seed, 32)     # EVP_PKEY_ED25519 = NID_ED25519
        ctx = c.EVP_MD_CTX_new()
        try:
            assert key and ctx and c.EVP_DigestSignInit(ctx, None, None, None, key) == 1
            out, ln = ctypes.create_string_buffer(64), ctypes.c_size_t(64)
            assert c.EVP_DigestSign(ctx, out, ctypes.byref(ln), msg, len(msg)) == 1 and ln.value == 64
            return out.raw
        finally:
            c.EVP_MD_CTX_free(ctx)
            c.EVP_PKEY_free(key)


def test_mixed_batch_equals_four_independent_signers(emul, oracle, capsys):
    """500 messages over 37 seeds: every length of cases.LENGTHS, the rest random up to 300 bytes, shuffled"""
    n, seeds = 500, cases.seeds(37)
    msgs = cases.mixed_messages(n, 0x51617)
    assert set(cases.LENGTHS) <= {len(m) for m in msgs}
    key_index = [(7 * i + i // 37) % 37 for i in range(n)]
    expanded, pks = _expand(emul, seeds)
    sigs, ok = _sign(emul, expanded, msgs, key_index)
    assert ok == [1] * n
    oracle.sbvo_ed25519_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    oracle.sbvo_ed25519_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    host = hostlib.load()
    signers = [host.sbvh_signer_new_scheme(1, 1, s) for s in seeds]
    ssl = _OpenSSL()
    if ssl.lib is None:
        with capsys.disabled():
            print("\n  libcrypto did not load: the OpenSSL opinion is left out, three signers remain")
    try:
        for j, s in enumerate(seeds):
            pk = ctypes.create_string_buffer(32)
            oracle.sbvo_ed25519_public_key(s, pk)
            assert pks[j] == pk.raw == ed.public_key(s)
        out, csig = ctypes.create_string_buffer(80), ctypes.create_string_buffer(64)
        for i, m in enumerate(msgs):
            s = seeds[key_index[i]]
            assert sigs[i] == ed.sign(s, m), (i, len(m))
            oracle.sbvo_ed25519_sign(s, m, len(m), csig)
            assert sigs[i] == csig.raw, (i, len(m))
            assert host.sbvh_sign(signers[key_index[i]], m, len(m), out, 80) == 64 and sigs[i] == out.raw[:64], (i, len(m))
            if ssl.lib is not None:
                assert sigs[i] == ssl.sign(s, m), (i, len(m))
    finally:
        for h in signers:
            host.sbvh_signer_free(h)


def test_rejected_lanes_write_zeros_and_leave_their_neighbours_alone(emul):
    seeds = cases.seeds(3)
    expanded, _ = _expand(emul, seeds)
    msgs = [b"m%d" % i for i in range(8)]
    idx = [0, 1, 3, 2, 0xFFFFFFFF, 0, 1, 2]
    sigs, ok = _sign(emul, expanded, msgs, idx)
    assert ok == [1, 1, 0, 1, 0, 1, 1, 1]
    for i in range(8):
        assert sigs[i] == (bytes(64) if idx[i] >= 3 else ed.sign(seeds[idx[i]], msgs[i]))
    sigs, ok = _sign(emul, expanded, msgs)                              # a null index: key i % n_keys
    assert ok == [1] * 8 and sigs == [ed.sign(seeds[i % 3], msgs[i]) for i in range(8)]


def test_sha512_head_msg_against_hashlib(emul):
    head = bytes(range(101, 165))
    body = hashlib.shake_128(b"sha512-head-msg").digest(300)
    out = ctypes.create_string_buffer(64)
    for head_len in (32, 64):
        for mlen in range(301):
            emul.sbvedsign_sha512_head_msg(head[:head_len], head_len, body[:mlen] + b"\0", mlen, out)
            assert out.raw == hashlib.sha512(head[:head_len] + body[:mlen]).digest(), (head_len, mlen)


def test_sc25519_muladd_against_python_integers(emul):
    blobs, want = cases.muladd_cases()
    assert len(blobs) == 7**3 + 2000
    assert _op(emul, 0, blobs) == want


def test_sc25519_reduce256_against_python_integers(emul):
    blobs, want = cases.reduce_cases()
    assert _op(emul, 1, blobs) == want


def test_encode_sB_against_ed25519_py(emul):
    blobs, want = cases.encode_cases()
    assert _op(emul, 2, blobs) == want


def test_sanitizer_build_signs_as_a_program_of_its_own(tmp_path):
    """the same source with its own main under AddressSanitizer and UBSan: the RFC vectors and 300 mixed-length messages, one run"""
    exe = str(tmp_path / "ed_sign_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DSBV_EMUL_MAIN", "-Wno-misleading-indentation", EMUL_SRC, "-o", exe])
    rows = [(v["seed"], v["pk"], v["msg"], v["sig"]) for v in cases.rfc_vectors()]
    seeds = cases.seeds(300, b"ed-sign-san")
    for s, m in zip(seeds, cases.mixed_messages(300, 0x5A17)):
        rows.append((s, ed.public_key(s), m, ed.sign(s, m)))
    path = tmp_path / "cases.txt"
    path.write_text("".join("%s %s %s %s\n" % (s.hex(), p.hex(), m.hex() or "-", g.hex()) for s, p, m, g in rows))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "%d cases, 0 differ" % len(rows) in r.stdout, r.stdout + r.stderr

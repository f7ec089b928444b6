"""Cases and model of the raw-message ECDSA signers (include/sbv.h: sbv_sha256_msgs, sbv_p256_sign_msgs, sbv_secp256k1_sign_msgs;
consensus_amd/csrc/ecdsa_sign_msgs.h), shared by the CPU tier (tests/test_ecdsa_sign_msgs_cpu.py) and the GPU tier
(tests/test_gpu_ecdsa_sign_msgs.py).

The model is Python integers, hashlib and hmac: SHA-256 by hashlib, the RFC 6979 nonce by hmac, the signing equation on integers
over the big-integer twins of the oracle (oracle/p256_py.py, oracle/k256_py.py), DER by p256_py.der_encode_sig and back through the
strict parser frontend_cases.strict_rs uses.  It shares nothing with the C lanes."""
import functools
import hashlib
import hmac
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import k256_py as kc  # noqa: E402
import p256_py as pc  # noqa: E402

import frontend_cases as fc  # noqa: E402

CURVES = ("p256", "k256")
CURVE_ID = {"p256": 0, "k256": 1}
MOD = {"p256": pc, "k256": kc}
LOW_S = 1
HASH_LENGTHS = list(range(261)) + [1023, 1024, 1025, 4097]
GEOMETRY = (1, 63, 64, 65, 255, 256, 257, 8229)
LARGE = 8229


def order(curve):
    return MOD[curve].N


def be32(v):
    return v.to_bytes(32, "big")


# ---- DER --------------------------------------------------------------------------------------------------------------------------------
def der_values():
    """1, 0x7f, 0x80, 0xff, 0x100, one value with each count of leading zero bytes 1 .. 31 in both states of the top bit of the first
    byte kept, 2^255 - 1, 2^255 and the largest order minus 1"""
    vals = [1, 0x7F, 0x80, 0xFF, 0x100]
    for z in range(1, 32):
        sig = 32 - z                                                  # significant bytes
        tail = hashlib.sha256(b"der value %d" % z).digest()[:sig - 1]
        low = int.from_bytes(b"\x5a" + tail, "big")                   # top bit of the first byte kept clear
        high = int.from_bytes(b"\xda" + tail, "big")                  # ... and set: a 00 goes in front
        vals += [low, high]
    vals += [(1 << 255) - 1, 1 << 255, kc.N - 1]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


def der_model(r, s):
    return pc.der_encode_sig(r, s)


@functools.lru_cache(maxsize=None)
def der_cases():
    """all pairs (r, s, der): every total length 8 .. 72 occurs, and every encoding parses back to (r, s) under the strict parser"""
    vals = der_values()
    assert 60 <= len(vals) <= 80
    cases = []
    for r in vals:
        for s in vals:
            der = der_model(r, s)
            assert fc.strict_rs(der) == be32(r) + be32(s), (r, s)
            cases.append((r, s, der))
    assert {len(c[2]) for c in cases} == set(range(8, 73))
    return cases


def leading_zero_bytes(v):
    return 32 - max(1, (v.bit_length() + 7) // 8)


# ---- low-S ------------------------------------------------------------------------------------------------------------------------------
def low_s_model(curve, s):
    n = order(curve)
    return (n - s, True) if s > (n - 1) // 2 else (s, False)


def low_s_cases(curve):
    n = order(curve)
    return [1, (n - 1) // 2, (n - 1) // 2 + 1, n - 1]


# ---- hash -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hash_messages():
    rng = random.Random(0xEC5A)
    return [bytes(rng.randrange(256) for _ in range(n)) for n in HASH_LENGTHS]


def pack_at_alignments(msgs, shuffled=False):
    """(messages, starts): one packed batch in which every message of `msgs` occurs four times, its first byte at each of the four
    offsets mod 4 of the blob (starts[i] = offset of messages[i]); filler messages of 1 .. 3 bytes — messages of the batch like any
    other — stand between them where the alignment asks for it"""
    items = [(m, a) for m in msgs for a in range(4)]
    if shuffled:
        random.Random(7).shuffle(items)
    out, starts, at = [], [], 0
    for m, a in items:
        gap = (a - at) % 4
        if gap:
            out.append(b"\xee" * gap)
            starts.append(at)
            at += gap
        out.append(m)
        starts.append(at)
        at += len(m)
    return out, starts


# ---- signing ----------------------------------------------------------------------------------------------------------------------------
def rfc6979_nonce(curve, d, h1):
    """RFC 6979 section 3.2 with HMAC-SHA256 for a 256-bit order: the first candidate in [1, n-1] and how many were rejected"""
    n = order(curve)
    x = be32(d)
    hb = be32(int.from_bytes(h1, "big") % n)                 # bits2octets
    V, K = b"\x01" * 32, b"\x00" * 32
    K = hmac.new(K, V + b"\x00" + x + hb, hashlib.sha256).digest()
    V = hmac.new(K, V, hashlib.sha256).digest()
    K = hmac.new(K, V + b"\x01" + x + hb, hashlib.sha256).digest()
    V = hmac.new(K, V, hashlib.sha256).digest()
    while True:
        V = hmac.new(K, V, hashlib.sha256).digest()
        k = int.from_bytes(V, "big")
        if 1 <= k < n:
            return k
        K = hmac.new(K, V + b"\x00", hashlib.sha256).digest()
        V = hmac.new(K, V, hashlib.sha256).digest()


def sign_model(curve, d, msg, low_s=False):
    """(r, s, recid) of the deterministic signature of SHA-256(msg), or None for a key outside [1, n-1]"""
    mod, n = MOD[curve], order(curve)
    if not 1 <= d < n:
        return None
    h = hashlib.sha256(msg).digest()
    e = int.from_bytes(h, "big") % n
    k = rfc6979_nonce(curve, d, h)
    R = mod.pt_mul(k, (mod.GX, mod.GY))
    r = R[0] % n
    s = pow(k, -1, n) * (e + r * d) % n
    assert r and s
    recid = (R[1] & 1) | (2 if R[0] >= n else 0)
    if low_s:
        s, neg = low_s_model(curve, s)
        recid ^= 1 if neg else 0
    return r, s, recid


class SignCase:
    def __init__(self, name, d, msg, index=None):
        self.name, self.d, self.msg, self.index = name, d, msg, index


@functools.lru_cache(maxsize=None)
def sign_cases(curve):
    """300 seeded (key, message) pairs with lengths from the hash list; the keys 0, n and n - 1; the known answers.  Case i signs with
    key i of the case list (key_index = None), except where .index is set."""
    rng = random.Random(0x516E + CURVE_ID[curve])
    n = order(curve)
    cases = []
    for i in range(300):
        d = rng.randrange(1, n)
        ln = HASH_LENGTHS[i] if i < len(HASH_LENGTHS) else rng.choice(HASH_LENGTHS)
        cases.append(SignCase("seeded_%d" % i, d, bytes(rng.randrange(256) for _ in range(ln))))
    cases.append(SignCase("key_zero", 0, b"key zero"))
    cases.append(SignCase("key_n", n, b"key n"))
    cases.append(SignCase("key_n_minus_1", n - 1, b"key n minus 1"))
    if curve == "p256":
        g = json.load(open(os.path.join(HERE, "golden", "rfc6979_p256.json")))
        for m in ("sample", "test"):
            cases.append(SignCase("rfc6979_" + m, int(g["private_key"], 16), m.encode()))
    else:
        for j, v in enumerate(json.load(open(os.path.join(HERE, "golden", "rfc6979_k256.json")))["vectors"]):
            if "msg" in v:
                cases.append(SignCase("known_%d" % j, int(v["d"], 16), v["msg"].encode()))
    return cases


def known_answers(curve):
    """{case name: (r, s) as published}: RFC 6979 A.2.5 under SHA-256 as it is; the secp256k1 answers in their published low-S form"""
    if curve == "p256":
        g = json.load(open(os.path.join(HERE, "golden", "rfc6979_p256.json")))
        return {"rfc6979_" + v["message"]: (int(v["r"], 16), int(v["s"], 16)) for v in g["signatures"] if v["hash_alg"] == "sha256"}
    vs = json.load(open(os.path.join(HERE, "golden", "rfc6979_k256.json")))["vectors"]
    return {"known_%d" % j: (int(v["sig"][:64], 16), int(v["sig"][64:], 16)) for j, v in enumerate(vs) if "msg" in v}


@functools.lru_cache(maxsize=None)
def expected(curve, low_s):
    """per case of sign_cases: (der, recid, ok); a refused case is (b"", 0, 0)"""
    out = []
    for c in sign_cases(curve):
        got = sign_model(curve, c.d, c.msg, low_s)
        out.append((b"", 0, 0) if got is None else (der_model(got[0], got[1]), got[2], 1))
    return out


def pubkey(curve, d):
    mod = MOD[curve]
    q = mod.pt_mul(d, (mod.GX, mod.GY))
    return be32(q[0]) + be32(q[1])


def offsets_of(msgs):
    offs = [0]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    return offs

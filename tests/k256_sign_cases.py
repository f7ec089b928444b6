"""Cases and expected values of the secp256k1 batch-signing tests, shared by the CPU tier (tests/test_k256_sign_cpu.py: the emulated
lanes) and the GPU tier (tests/test_gpu_k256_sign.py: the kernels), so that both run the same cases.  Expected values come from
Python's hmac / hashlib (the RFC 6979 nonce), Python integers and oracle/k256_py.py only."""
import functools
import hashlib
import hmac
import json
import os
import random

import k256_py as kp

HERE = os.path.dirname(os.path.abspath(__file__))
N, P = kp.N, kp.P
HALF = (N - 1) // 2
LOW_S = 1                                      # SBV_K256_SIGN_LOW_S
EDGE_DIGESTS = [0, N - 1, N, N + 1, 2**256 - 1]
EDGE_KEYS = [1, 2, N - 2, N - 1]
OP_IN, OP_OUT = 192, 128                       # the records of sbv_debug_secp256k1_sign_op


def be32(x):
    return x.to_bytes(32, "big")


def vectors():
    """the four community known answers: d, k and sig as bytes, digest = SHA-256(msg)"""
    with open(os.path.join(HERE, "golden", "rfc6979_k256.json")) as f:
        out = []
        for v in json.load(f)["vectors"]:
            out.append({"d": bytes.fromhex(v["d"]), "k": bytes.fromhex(v["k"]), "sig": bytes.fromhex(v["sig"]),
                        "digest": hashlib.sha256(v["msg"].encode()).digest(), "s_was_high": v["s_was_high"]})
        return out


# ---- RFC 6979 section 3.2 with HMAC-SHA256, qlen = hlen = 256, from hmac / hashlib ---------------------------------------------------
def _mac(key, data):
    return hmac.new(key, data, hashlib.sha256).digest()


def drbg_states(d, digest):
    """generator of (k, K, V) per candidate: the candidate as bytes and the state behind it (V == k)"""
    x = be32(d)
    h1 = be32(int.from_bytes(digest, "big") % N)                    # bits2octets
    V, K = b"\x01" * 32, b"\x00" * 32
    for tag in (b"\x00", b"\x01"):
        K = _mac(K, V + tag + x + h1)
        V = _mac(K, V)
    while True:
        V = _mac(K, V)
        yield V, K, V
        K, V = drbg_reject(K, V)


def drbg_reject(K, V):
    """section 3.2 h after a rejected candidate: K' = HMAC(K, V || 00), V' = HMAC(K', V)"""
    K2 = _mac(K, V + b"\x00")
    return K2, _mac(K2, V)


def finish(x, y_odd, d, k, e, flags):
    """k256_sign_finish on integers -> (r, s, recid) or None"""
    r = x % N
    if r == 0:
        return None
    recid = (1 if y_odd else 0) | (2 if x >= N else 0)
    s = pow(k, -1, N) * (e + r * d) % N
    if s == 0:
        return None
    if flags & LOW_S and s > HALF:
        s, recid = N - s, recid ^ 1
    return r, s, recid


@functools.lru_cache(maxsize=None)
def _nonce_point(kb):
    return kp.pt_mul(int.from_bytes(kb, "big"), kp.G)


def py_sign(d, digest, flags=0):
    """the independent signer: (r | s, recid, ok); d outside [1, n-1] -> (64 zero bytes, 0, 0)"""
    if not 1 <= d < N:
        return bytes(64), 0, 0
    e = int.from_bytes(digest, "big") % N
    for kb, _, _ in drbg_states(d, digest):
        k = int.from_bytes(kb, "big")
        if not 1 <= k < N:
            continue
        R = _nonce_point(kb)                                        # shared by the two flag settings of a case
        got = finish(R[0], R[1] & 1, d, k, e, flags)
        if got is not None:
            return be32(got[0]) + be32(got[1]), got[2], 1


def recover(rs, recid, digest):
    """the public key from a signature and its recovery id: the point R with x = r (+ n) and the parity of bit 0, Q = r^-1 (s R - e G)"""
    r, s = int.from_bytes(rs[:32], "big"), int.from_bytes(rs[32:], "big")
    x = r + (N if recid & 2 else 0)
    if x >= P:
        return None
    y = pow(x**3 + 7, (P + 1) // 4, P)                              # p = 3 mod 4
    if (y * y - x**3 - 7) % P:
        return None
    if (y & 1) != (recid & 1):
        y = P - y
    e = int.from_bytes(digest, "big") % N
    ri = pow(r, -1, N)
    return kp.pt_add(kp.pt_mul(s * ri % N, (x, y)), kp.pt_mul((N - e) * ri % N, kp.G))


def pub_bytes(q):
    return be32(q[0]) + be32(q[1])


# ---- the signing cases ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sign_cases():
    """[(d, digest)]: 300 seeded pairs, then every edge digest under every edge key"""
    rng = random.Random(0x6979256)
    out = [(rng.randrange(1, N), rng.randbytes(32)) for _ in range(300)]
    out += [(d, be32(h)) for d in EDGE_KEYS for h in EDGE_DIGESTS]
    return out


@functools.lru_cache(maxsize=None)
def sign_expected(flags):
    """[(r | s, recid)] of sign_cases() from the independent signer"""
    return [py_sign(d, h, flags)[:2] for d, h in sign_cases()]


@functools.lru_cache(maxsize=None)
def pubkey_cases():
    """(keys, expected Qx | Qy): the edge keys and 100 seeded ones"""
    rng = random.Random(0x9B256)
    keys = EDGE_KEYS + [rng.randrange(1, N) for _ in range(100)]
    return keys, [pub_bytes(kp.pt_mul(d, kp.G)) for d in keys]


# ---- the unit operations: (input records, expected output records) -----------------------------------------------------------------
def op_record(*fields):
    """up to six integers or 32-byte strings -> one 192-byte input record"""
    b = b"".join(f if isinstance(f, bytes) else be32(f) for f in fields)
    return b + bytes(OP_IN - len(b))


def op_result(ok, *fields):
    if not ok:
        return bytes(OP_OUT)
    b = b"".join(f if isinstance(f, bytes) else be32(f) for f in fields)
    return b + bytes(OP_OUT - 32 - len(b)) + be32(1)


@functools.lru_cache(maxsize=None)
def op0_cases():
    pairs = sign_cases()[:40] + sign_cases()[300:] + [(0, bytes(32)), (N, b"\x11" * 32)]
    ins, outs = [], []
    for d, h in pairs:
        ins.append(op_record(d, h))
        if 1 <= d < N:
            k, K, V = next(drbg_states(d, h))
            outs.append(op_result(1, k, K, V))
        else:
            outs.append(op_result(0))
    return ins, outs


@functools.lru_cache(maxsize=None)
def op1_cases():
    """states taken from op 0 (the state behind a first candidate), and the all-zero and all-0xff states"""
    states = [next(drbg_states(d, h))[1:] for d, h in sign_cases()[:40]] + [(bytes(32), bytes(32)), (b"\xff" * 32, b"\xff" * 32),
                                                                           (bytes(32), b"\xff" * 32), (b"\xff" * 32, bytes(32))]
    ins, outs = [], []
    for K, V in states:
        K2, V2 = drbg_reject(K, V)
        ins.append(op_record(K, V))
        outs.append(op_result(1, K2, V2, _mac(K2, V2)))
    return ins, outs


@functools.lru_cache(maxsize=None)
def op2_cases():
    """one non-zero digit per comb window at both ends of the signed digit range, the edge scalars and seeded ones; 0, n and 2^256 - 1
    are outside the domain and answer ok = 0"""
    rng = random.Random(0x0256)
    vals = [1, 2, 3, N - 1, N - 2, HALF, HALF + 1] + [2**(16 * j) for j in range(16)] + [2**(16 * j) * 32768 for j in range(16)]
    vals += [rng.randrange(1, N) for _ in range(60)] + [0, N, 2**256 - 1]
    ins = [op_record(v) for v in vals]
    outs = [op_result(1, pub_bytes(kp.pt_mul(v, kp.G))) if 1 <= v < N else op_result(0) for v in vals]
    return ins, outs


@functools.lru_cache(maxsize=None)
def op3_cases():
    """k256_sign_finish: x around n (bit 1 of recid exactly for x >= n; x = n gives r = 0), an (e, d, r) with e + r d = 0 mod n, seeded
    ones; every case under both flag settings and both parities"""
    rng = random.Random(0x3256)
    quads = [(x, rng.randrange(1, N), rng.randrange(1, N), rng.randrange(N)) for x in (N - 1, N, N + 1, P - 1, 1, 2**256 - 1)]
    r, d = rng.randrange(1, N), rng.randrange(1, N)
    quads.append((r, d, rng.randrange(1, N), (N - r * d % N) % N))                         # s = 0
    quads.append((r + N if r + N < 2**256 else r, d, rng.randrange(1, N), (N - r * d % N) % N))
    quads += [(rng.randrange(2**256), rng.randrange(1, N), rng.randrange(1, N), rng.randrange(N)) for _ in range(60)]
    quads += [(rng.randrange(1, N), rng.choice(EDGE_KEYS), rng.choice(EDGE_KEYS), rng.choice([0, 1, N - 1])) for _ in range(20)]
    ins, outs = [], []
    for x, d, k, e in quads:
        for y_odd in (0, 1):
            for flags in (0, LOW_S):
                ins.append(op_record(x, y_odd, d, k, e, flags))
                got = finish(x, y_odd, d, k, e, flags)
                outs.append(op_result(0) if got is None else op_result(1, *got))
    return ins, outs


def all_op_cases():
    return [op0_cases(), op1_cases(), op2_cases(), op3_cases()]

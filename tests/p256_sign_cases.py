"""Cases and expected values of the P-256 batch-signing tests, shared by the CPU tier (tests/test_emul_sign.py: the emulated lanes
and the host signer) and the GPU tier (tests/test_gpu_sign.py: k_p256_sign), so that both run the same cases.  Expected values come
from Python's hmac / hashlib (the RFC 6979 nonce), Python integers and oracle/p256_py.py only: nothing here reads a header of the
product, so a reading of the RFC shared by p256_sign.h and p256_host.cc does not reach it."""
import functools
import hashlib
import hmac
import json
import os
import random

import p256_py as pp

HERE = os.path.dirname(os.path.abspath(__file__))
N, P = pp.N, pp.P
EDGE_DIGESTS = [0, 1, N - 1, N, N + 1, 2**255, 2**256 - 1]
EDGE_KEYS = [1, 2, N - 2, N - 1]
REJECTED_KEYS = [0, N, 2**256 - 1]


def be32(x):
    return x.to_bytes(32, "big")


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


def finish(x, d, k, e):
    """sign29_finish on integers: the affine x of k G, d and k in [1, N-1], e < N -> (r, s) or None"""
    r = x % N
    if r == 0:
        return None
    s = pow(k, -1, N) * (e + r * d) % N
    if s == 0:
        return None
    return r, s


@functools.lru_cache(maxsize=None)
def _nonce_x(kb):
    return pp.pt_mul(int.from_bytes(kb, "big"), pp.G)[0]


def py_sign(d, digest):
    """the independent signer: (r | s, ok, index of the accepted candidate); d outside [1, N-1] -> (64 zero bytes, 0, -1)"""
    if not 1 <= d < N:
        return bytes(64), 0, -1
    e = int.from_bytes(digest, "big") % N
    for index, (kb, _, _) in enumerate(drbg_states(d, digest)):
        k = int.from_bytes(kb, "big")
        if not 1 <= k < N:
            continue
        got = finish(_nonce_x(kb), d, k, e)
        if got is not None:
            return be32(got[0]) + be32(got[1]), 1, index


@functools.lru_cache(maxsize=None)
def pubkey(d):
    q = pp.pt_mul(d, pp.G)
    return be32(q[0]) + be32(q[1])


# ---- the signing cases ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sign_cases():
    """[(d, digest)]: 300 seeded pairs, then every edge digest under every edge key"""
    rng = random.Random(0x6979A25)
    out = [(rng.randrange(1, N), rng.randbytes(32)) for _ in range(300)]
    out += [(d, be32(h)) for d in EDGE_KEYS for h in EDGE_DIGESTS]
    return out


@functools.lru_cache(maxsize=None)
def sign_expected():
    """[r | s] of sign_cases() from the independent signer; every case is signed"""
    out = [py_sign(d, h) for d, h in sign_cases()]
    assert all(ok == 1 for _, ok, _ in out)
    return [rs for rs, _, _ in out]


def blobs(pairs):
    """(keys, digests) as the entries take them, case i under key i"""
    return b"".join(be32(d) for d, _ in pairs), b"".join(h for _, h in pairs)


@functools.lru_cache(maxsize=None)
def retry_vector():
    """the one known input whose first RFC 6979 candidate is >= N: tests/golden/rfc6979_p256_retry.json, every field checked against
    the independent signer before anything is compared with it"""
    with open(os.path.join(HERE, "golden", "rfc6979_p256_retry.json")) as f:
        v = json.load(f)
    d, digest = int(v["d"], 16), bytes.fromhex(v["digest"])
    k1, k2 = int(v["k1"], 16), int(v["k2"], 16)
    assert digest == hashlib.sha256(v["msg"].encode()).digest()
    assert k1 >= N and 1 <= k2 < N
    states = drbg_states(d, digest)
    assert [next(states)[0], next(states)[0]] == [be32(k1), be32(k2)]
    rs, ok, index = py_sign(d, digest)
    assert (ok, index) == (1, 1) and rs.hex() == v["r"] + v["s"]
    return {"d": d, "digest": digest, "k1": k1, "k2": k2, "sig": rs}

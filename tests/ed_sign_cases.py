"""Operand lists and expected values of the Ed25519 batch-signing tests, shared by the CPU tier (tests/test_ed25519_sign_cpu.py: the
emulated lanes) and the GPU tier (tests/test_gpu_ed25519_sign.py: the kernels), so that both run the same cases.  Expected values come
from Python integers and oracle/ed25519_py.py only."""
import functools
import hashlib
import json
import os
import random

import ed25519_py as ed

HERE = os.path.dirname(os.path.abspath(__file__))
L = ed.L
# every block boundary of both hashes: 32 + len + 17 (nonce) and 64 + len + 17 (challenge) cross a multiple of 128 at 48/80 - 1, ...
LENGTHS = [0, 1, 31, 32, 47, 48, 63, 64, 79, 80, 111, 112, 127, 128, 175, 176, 207, 208, 239, 240, 255, 256, 1023, 4096]


def rfc_vectors():
    with open(os.path.join(HERE, "golden", "rfc8032_sign.json")) as f:
        return [{k: (bytes.fromhex(v) if k != "name" else v) for k, v in e.items()} for e in json.load(f)["vectors"]]


def le32(x):
    return x.to_bytes(32, "little")


def seeds(count, label=b"ed-sign-seed"):
    return [hashlib.sha256(label + b"%d" % i).digest() for i in range(count)]


def mixed_messages(n, rng_seed, max_random=300):
    """n messages: every length of LENGTHS at least once, the rest random lengths <= max_random, shuffled so that neighbours (the
    lanes of a wavefront) differ in their block counts"""
    rng = random.Random(rng_seed)
    lens = list(LENGTHS) + [rng.randrange(max_random + 1) for _ in range(n - len(LENGTHS))]
    rng.shuffle(lens)
    return [rng.randbytes(k) for k in lens]


def pack_messages(msgs):
    """-> (payload bytes, offsets list of len(msgs) + 1)"""
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    return b"".join(msgs), off


# ---- unit operations: (input blobs, expected 32-byte outputs) ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def muladd_cases():
    edge = [0, 1, 2, L - 2, L - 1, 2**252, 2**252 - 1]
    rng = random.Random(0x5C25519)
    trip = [(k, a, r) for k in edge for a in edge for r in edge] + [tuple(rng.randrange(L) for _ in range(3)) for _ in range(2000)]
    return ([le32(k) + le32(a) + le32(r) for k, a, r in trip], [le32((k * a + r) % L) for k, a, r in trip])


@functools.lru_cache(maxsize=None)
def reduce_cases():
    rng = random.Random(0x25519)
    vals = [0, 1, L - 1, L, L + 1, 2 * L, 7 * L + 3, 2**255 - 8, 2**256 - 1] + [rng.randrange(2**256) for _ in range(500)]
    return ([le32(v) for v in vals], [le32(v % L) for v in vals])


@functools.lru_cache(maxsize=None)
def encode_cases():
    """one non-zero digit per comb window at both ends of the signed digit range: 2^(16 j) is digit +1 of window j, 2^(16 j) * 32768 is
    digit -32768 of window j with a carry into window j + 1.  In the top window the second value is 2^255, beyond the operation's domain
    s < L (and beyond ed_add_sB's S < 2^253): it enters as 2^255 mod L, the scalar a signer would walk for it."""
    rng = random.Random(0xED5167)
    vals = [0, 1, 2, 3, L - 1, L - 2, 2**252]
    vals += [2**(16 * j) for j in range(16)] + [2**(16 * j) * 32768 % L for j in range(16)]
    vals += [rng.randrange(L) for _ in range(100)]
    return ([le32(v) for v in vals], [ed.encode(ed.pt_mul(v, ed.B)) for v in vals])

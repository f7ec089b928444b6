"""The model and the cases of the Keccak-256 tests, shared by the CPU tier (tests/test_keccak_cpu.py: the lane code as host code, the
host forms) and the GPU tier (tests/test_gpu_keccak.py: the kernels), so that both run the same cases.

The model is Keccak-f[1600] and the sponge at rate 136 on Python integers, written from the specification and not from the device
code: the rotation offsets come from the (t + 1)(t + 2) / 2 walk, the lane permutation from (x, y) -> (y, 2 x + 3 y), the round
constants from the degree-8 LFSR.  The domain byte is a parameter: with 0x06 the model is SHA3-256, which hashlib can check; with 0x01
it is Keccak-256, which hashlib does not have.  tests/golden/keccak256.json holds four published values."""
import functools
import json
import os
import random

import k256_recover_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
RATE = 136
KECCAK, SHA3 = 0x01, 0x06
M64 = (1 << 64) - 1


def _rotl(v, n):
    n %= 64
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


@functools.lru_cache(maxsize=None)
def rho_offsets():
    """{(x, y): offset} of the rho step"""
    out = {(0, 0): 0}
    x, y = 1, 0
    for t in range(24):
        out[(x, y)] = (t + 1) * (t + 2) // 2 % 64
        x, y = y, (2 * x + 3 * y) % 5
    return out


@functools.lru_cache(maxsize=None)
def round_constants():
    """the 24 iota constants: bit 2^j - 1 of round i is output 7 i + j of the LFSR x^8 + x^6 + x^5 + x^4 + 1"""
    def rc_bit(t):
        r = 1
        for _ in range(t % 255):
            r <<= 1
            if r & 0x100:
                r ^= 0x171
        return r & 1
    return [sum(rc_bit(7 * i + j) << ((1 << j) - 1) for j in range(7)) for i in range(24)]


def f1600(lanes):
    """Keccak-f[1600] on 25 integers A[x + 5 y]"""
    a = list(lanes)
    rho = rho_offsets()
    for rnd in round_constants():
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[x + 5 * y], rho[(x, y)])
        a = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & M64 & b[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
        a[0] ^= rnd
    return a


def f1600_bytes(state):
    """200 bytes (25 little-endian lanes) -> 200 bytes"""
    lanes = f1600([int.from_bytes(state[8 * i:8 * i + 8], "little") for i in range(25)])
    return b"".join(v.to_bytes(8, "little") for v in lanes)


def sponge256(msg, domain=KECCAK):
    """the 32-byte digest at rate 136 with `domain` after the message and 0x80 into the last byte of the last block"""
    pad = bytearray(msg) + bytes([domain]) + bytes(-(len(msg) + 1) % RATE)
    pad[-1] |= 0x80
    state = bytes(200)
    for off in range(0, len(pad), RATE):
        block = bytes(pad[off:off + RATE]) + bytes(200 - RATE)
        state = f1600_bytes(bytes(p ^ q for p, q in zip(state, block)))
    return state[:32]


def keccak256(msg):
    return sponge256(msg, KECCAK)


def address(pub64):
    return keccak256(pub64)[12:]


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(os.path.join(HERE, "golden", "keccak256.json")))


# ---- messages: every length 0 .. 2 * 136 + 9 and a few around 5 * 136, contents zeros, 0xff and a counter ------------------------------
MSG_LENGTHS = list(range(0, 2 * RATE + 10)) + [5 * RATE - 1, 5 * RATE, 5 * RATE + 1, 5 * RATE + 7]


@functools.lru_cache(maxsize=None)
def messages():
    """the message cases in packing order; contents cycle with the index so that every length class sees all three over the set"""
    out = []
    for i, n in enumerate(MSG_LENGTHS):
        kind = i % 3
        out.append(bytes(n) if kind == 0 else b"\xff" * n if kind == 1 else bytes((i + k) & 0xFF for k in range(n)))
    # the block edges under the other two contents as well, so that 135 / 136 / 137 and 271 / 272 / 273 meet zeros, 0xff and a counter
    for n in (RATE - 1, RATE, RATE + 1, 2 * RATE - 1, 2 * RATE, 2 * RATE + 1):
        i = MSG_LENGTHS.index(n)
        for kind in ((i + 1) % 3, (i + 2) % 3):
            out.append(bytes(n) if kind == 0 else b"\xff" * n if kind == 1 else bytes((7 + k) & 0xFF for k in range(n)))
    return out


@functools.lru_cache(maxsize=None)
def packed_messages():
    """(blob, offsets): the messages back to back; the lengths 0, 1, 2, ... put the starts on every residue mod 8"""
    msgs = messages()
    offs = [0]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    assert {o % 8 for o in offs[:-1]} == set(range(8))
    return b"".join(msgs), offs


@functools.lru_cache(maxsize=None)
def message_digests(domain=KECCAK):
    return [sponge256(m, domain) for m in messages()]


# ---- permutation states: zero, ones, one bit in each lane at bit 0 and bit 63, 32 seeded ------------------------------------------------
@functools.lru_cache(maxsize=None)
def states():
    rng = random.Random(0x6ECCA6)
    out = [bytes(200), b"\xff" * 200]
    for lane in range(25):
        for bit in (0, 63):
            out.append(bytes(8 * lane) + (1 << bit).to_bytes(8, "little") + bytes(8 * (24 - lane)))
    out += [rng.randbytes(200) for _ in range(32)]
    return out


@functools.lru_cache(maxsize=None)
def states_after():
    return [f1600_bytes(s) for s in states()]


# ---- keys and recovery: every case of k256_recover_cases, the address being the model's hash of the expected key ------------------------
@functools.lru_cache(maxsize=None)
def key_cases():
    """64-byte inputs of the pure hash: every distinct expected key of the recovery cases, zeros, ones and seeded bytes (no curve check)"""
    rng = random.Random(0xADD2)
    keys = sorted({pub for pub, ok in rc.expected_all() if ok})[:96]
    return keys + [bytes(64), b"\xff" * 64] + [rng.randbytes(64) for _ in range(30)]


@functools.lru_cache(maxsize=None)
def key_addresses():
    return [address(k) for k in key_cases()]


@functools.lru_cache(maxsize=None)
def _address_of(pub):
    return address(pub)


@functools.lru_cache(maxsize=None)
def recover_expected_all():
    """[(address, ok)] of k256_recover_cases.cases(); a refused case expects 20 zero bytes"""
    return [(_address_of(pub), 1) if ok else (bytes(20), 0) for pub, ok in rc.expected_all()]


def recover_by_flags(flags):
    """(indices, sigs, recid, digests, addrs, ok) of the cases of one flag setting, as the arrays of a call and its expected result"""
    idx, sigs, rid, digs = rc.by_flags(flags)
    exp = recover_expected_all()
    return idx, sigs, rid, digs, b"".join(exp[i][0] for i in idx), bytes(exp[i][1] for i in idx)


def recover_tiled(flags, n, shift=0):
    """k256_recover_cases.tiled with addresses: (sigs, recid, digests, addrs, ok) of n items"""
    sigs, rid, digs, pubs, ok = rc.tiled(flags, n, shift)
    addrs = b"".join(_address_of(pubs[64 * i:64 * i + 64]) if ok[i] else bytes(20) for i in range(n))
    return sigs, rid, digs, addrs, ok

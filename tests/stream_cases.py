"""Complementary batches for the stream-ordering tier (tests/test_gpu_stream_order.py; no GPU needed here).

A pair (X, Y) of one scheme holds the same n tuples by the same signers, spoiled so that the verdicts differ at EVERY position: X accepts
exactly the even tuples, Y exactly the odd ones.  A kernel that reads a tuple, a key or a record from the wrong generation of a buffer flips
a verdict bit wherever it does so; a read that mixes the generations gives a bitmap equal to neither.

Construction: an all-valid batch from the oracle's generator (invalid_every = 0: tuple i is signed by key i % signers), then every second
tuple spoiled, rotating through three causes —
    0: one bit of s (Ed25519: of S),
    1: one bit of the hash (Ed25519: of k),
    2: the public key replaced by the valid key of another signer of the same batch
— the third being what catches a stale read by the grouping kernels, which read the keys only.  The keyed form of a pair is the same
tuples as records plus slots (the key bytes looked up among the pair's registered keys), so the key swap becomes another registered slot.
With `singles` > 0 the batch has a long tail: 24 signers with at least 64 uses each — twelve below and twelve above the 256 uses from which
the P-256 step fills a key's table — and that many keys used once, shuffled: the ungrouped list, the rows-only class and the full tables
of a grouped step then all have work on their own streams in one batch.

tests/test_stream_cases_cpu.py holds every pair used on the GPU to the oracles: the bitmaps are the intended ones, position by position."""
import ctypes
import os

import numpy as np

THREADS = min(os.cpu_count() or 1, 16)
#            name: (tuple bytes, key offset, key bytes, generator, batch verifier, offsets of (s, hash) — the fields of causes 0 and 1)
SCHEMES = {"p256": (160, 96, 64, "sbvo_gen_batch", "sbvo_p256_verify_batch", (32, 64)),
           "k256": (160, 96, 64, "sbvo_k256_gen_batch", "sbvo_k256_verify_batch", (32, 64)),
           "ed25519": (128, 64, 32, "sbvo_ed25519_gen_batch", "sbvo_ed25519_verify_batch", (32, 96))}
SIGNERS = 24
MAIN, ABOVE_THRESHOLD, ONE_LANE = 8229, 70, 40          # the sizes of the GPU tier: ragged and key-sorted / just above the grouped threshold of 64 / the one-lane kernels
SINGLES = 100                                           # single-use keys of the long-tail batches (MAIN only)
LIGHT_USES = 85                                         # ... whose 24 signers are 12 with 85 uses each (P-256: a table of rows only, below 256 uses) and 12 with 592 or 593 (a full table)
N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
_GEN_ARGS = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
_VER_ARGS = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
_CACHE = {}


def prepare(oracle):
    """argtypes of the generators and batch verifiers of the three schemes on a ctypes handle of the oracle"""
    for _, _, _, gen, ver, _ in SCHEMES.values():
        getattr(oracle, gen).argtypes = _GEN_ARGS
        getattr(oracle, ver).argtypes = _VER_ARGS
    return oracle


def intended(n, accept_parity):
    """the bitmap that accepts exactly the tuples i with i % 2 == accept_parity"""
    return np.packbits((np.arange(n) % 2 == accept_parity).astype(np.uint8), bitorder="little").tobytes()


def oracle_bitmap(oracle, scheme, rows):
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0]
    out = ctypes.create_string_buffer((n + 7) // 8)
    getattr(oracle, SCHEMES[scheme][4])(rows.ctypes.data, n, out, THREADS)
    return out.raw


def _generate(oracle, scheme, seed, n, nkeys):
    stride, gen = SCHEMES[scheme][0], SCHEMES[scheme][3]
    tup, exp = ctypes.create_string_buffer(stride * n), ctypes.create_string_buffer((n + 7) // 8)
    getattr(oracle, gen)(seed, n, nkeys, 0, tup, exp, THREADS)
    assert exp.raw == np.packbits(np.ones(n, dtype=np.uint8), bitorder="little").tobytes(), "the generator's batch is not all valid"
    return np.frombuffer(tup.raw, dtype=np.uint8).reshape(n, stride).copy()


class Pair:
    """x, y: [n, stride] uint8; want_x, want_y: the intended bitmaps; keys: the distinct valid keys in order of first appearance (the
    registry of the keyed form); cause[i] = how tuple i was spoiled in the generation that rejects it."""

    def __init__(self, scheme, base):
        self.scheme = scheme
        self.stride, self.key_off, self.key_len, _, _, (s_off, h_off) = SCHEMES[scheme]
        self.n = n = base.shape[0]
        self.base = base
        ko, kl = self.key_off, self.key_len
        index, self.keys = {}, []
        for i in range(n):
            k = base[i, ko:ko + kl].tobytes()
            if k not in index:
                index[k] = len(self.keys)
                self.keys.append(k)
        self._index = index
        self.cause = (np.arange(n) // 2) % 3
        self.x, self.y = base.copy(), base.copy()
        for i in range(n):
            t = self.x[i] if i % 2 else self.y[i]             # X rejects the odd tuples, Y the even ones
            c = int(self.cause[i])
            bit = (7 * i + 3) % 248                            # below the top byte: s stays in range, the verdict falls to the curve equation
            if c == 0:
                t[s_off + 31 - (bit >> 3) if scheme != "ed25519" else s_off + (bit >> 3)] ^= 1 << (bit & 7)
            elif c == 1:
                t[h_off + 31 - (bit >> 3) if scheme != "ed25519" else h_off + (bit >> 3)] ^= 1 << (bit & 7)
            else:
                j = (i + 1) % n
                while base[j, ko:ko + kl].tobytes() == base[i, ko:ko + kl].tobytes():
                    j = (j + 1) % n
                    assert j != i, "a pair needs two signers"
                t[ko:ko + kl] = base[j, ko:ko + kl]
        self.want_x, self.want_y = intended(n, 0), intended(n, 1)

    def rows(self, g):
        return self.x if g == "x" else self.y

    def want(self, g):
        return self.want_x if g == "x" else self.want_y

    def keyed(self, g):
        """(records [n, 96] uint8, slots [n] uint32) of generation g: the tuple without its key, and the key's place among self.keys"""
        rows, ko, kl = self.rows(g), self.key_off, self.key_len
        recs = np.ascontiguousarray(np.concatenate([rows[:, :ko], rows[:, ko + kl:]], axis=1))
        slots = np.array([self._index[rows[i, ko:ko + kl].tobytes()] for i in range(self.n)], dtype=np.uint32)
        return recs, slots

    def tuples_of(self, g):
        """the 160 / 128-byte tuples the keyed form of generation g stands for (the oracle's input)"""
        recs, slots = self.keyed(g)
        keys = np.frombuffer(b"".join(self.keys), dtype=np.uint8).reshape(len(self.keys), self.key_len)
        return np.ascontiguousarray(np.concatenate([recs[:, :self.key_off], keys[slots], recs[:, self.key_off:]], axis=1))


def pair(oracle, scheme, n, singles=0, seed=0x57AE0000):
    """The pair of `scheme` with n tuples by SIGNERS signers in turn; with singles > 0 the long-tail batch instead: 12 signers with
    LIGHT_USES tuples each, 12 with the rest, `singles` keys used once, in a fixed random order.  Made once per process and shared:
    callers must not write into it."""
    key = (scheme, n, singles, seed)
    if key not in _CACHE:
        prepare(oracle)
        sid = list(SCHEMES).index(scheme)
        if singles:
            light = LIGHT_USES * (SIGNERS // 2)
            base = np.concatenate([_generate(oracle, scheme, seed + 16 * sid + 1, n - singles - light, SIGNERS // 2),
                                   _generate(oracle, scheme, seed + 16 * sid + 2, light, SIGNERS // 2),
                                   _generate(oracle, scheme, seed + 16 * sid + 3, singles, singles)])
            base = base[np.random.default_rng(seed + sid).permutation(n)]
        else:
            base = _generate(oracle, scheme, seed + 16 * sid, n, SIGNERS)
        _CACHE[key] = Pair(scheme, base)
    return _CACHE[key]


def digest_pair(n, seed=0x5169):
    """(private keys [nk x 32 bytes], key index [n] uint32, digests X, digests Y): two digest sets that differ at every position, so
    every RFC 6979 signature of one set differs from its twin in the other."""
    rng = np.random.default_rng(seed + n)
    nk = 37
    keys = b"".join(int.to_bytes(int.from_bytes(rng.bytes(32), "big") % (N_ORDER - 1) + 1, 32, "big") for _ in range(nk))
    index = rng.integers(0, nk, n).astype(np.uint32)
    dx = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    dy = dx.copy()
    dy[:, 31] ^= 0x5A
    return keys, index, dx, dy


def gpu_pairs():
    """(scheme, n, singles) of every pair the GPU tier uses — what the CPU tier holds to the oracles"""
    out = []
    for scheme in SCHEMES:
        out += [(scheme, MAIN, 0), (scheme, MAIN, SINGLES), (scheme, ABOVE_THRESHOLD, 0), (scheme, ONE_LANE, 0)]
    return out

"""GPU tier of the piece pipeline (consensus_amd/csrc/shard_pieces.h) at the smallest shapes: the three sharded entries with the piece
sizes at the library's minimum, SBV_SHARD_PIECE = SBV_SHARD_PIECE_KEYED = 512, every call on one device (info.shards == 1), so that
a share of n signatures is this call's pieces and nothing else.

With group = 4 the granule is 512 and n = 512, 1 024, 1 536, 1 541 go up as 1, 2, 3 and 4 pieces: three is the first shape that reuses a
staging set, four with a tail of 5 the first with a ragged last piece — one whole proposal and one signature that gets no quorum bit.
With group = 3 the granule is 1 536, above the piece size: n = 3 077 is one piece in the tuple form (whole launches) and 1 536, 1 536, 5
in the two registered-key forms (tests/test_shard_pieces_cpu.py holds these plans as literal cases).

One batch of 3 077 signatures by 16 keys serves every case as a prefix: messages of 0 to 40 bytes signed by the device's RFC 6979 signer,
then a seeded pseudo-random fifth with a bit of s flipped, so that no stretch of 512 verdicts looks like another and a bitmap written at
the wrong piece offset cannot pass.  Expected verdicts are the C oracle's (sbvo_p256_verify_batch for the tuples and records,
sbvo_p256_verify_asn1 for the DER form), expected quorum bits the numpy twin's (consensus_amd/shard.py: quorum_bits_slots) and, for the
tuple form, a count of distinct accepted keys."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import consensus_amd as sbv
import p256_py as ec
from consensus_amd import shard

pytestmark = pytest.mark.gpu

N, NKEYS = 3077, 16
CASES = [(512, 4, 3), (1024, 4, 3), (1536, 4, 3), (1541, 4, 3), (3077, 3, 2)]
PIECE_ENV = {"SBV_SHARD_PIECE": 1 << 18, "SBV_SHARD_PIECE_KEYED": 1 << 17}       # the variables and the library's defaults (sbv_api.hip)


class Batch:
    pass


@pytest.fixture(scope="module")
def batch(oracle):
    for k in PIECE_ENV:
        os.environ[k] = "512"
    try:
        sbv.shutdown()
        assert sbv.init_all() >= 1                   # the piece sizes are read here
        sbv.key_cache(True)                          # the tuple form cuts pieces only with the key-table cache on
        rng = random.Random(0x5AD0)
        b = Batch()
        ds = [rng.randrange(1, ec.N) for _ in range(NKEYS)]
        keys = [q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big") for q in (ec.pt_mul(d, ec.G) for d in ds)]
        slot_of = sbv.register_keys(keys)
        assert len(set(slot_of)) == NKEYS
        b.msgs = [bytes(rng.randrange(256) for _ in range(rng.randrange(41))) for _ in range(N)]
        digests = [hashlib.sha256(m).digest() for m in b.msgs]
        kidx = [rng.randrange(NKEYS) for _ in range(N)]
        rs, ok = sbv.sign_batch(b"".join(d.to_bytes(32, "big") for d in ds), b"".join(digests), kidx)
        assert ok == b"\x01" * N
        bad = set(rng.sample(range(N), N // 5))
        assert all([i in bad for i in range(o, o + 512)] != [i in bad for i in range(512)] for o in range(512, N - 512, 512))
        rs = bytearray(rs)
        for i in bad:
            rs[64 * i + 63] ^= 1                     # s with its lowest bit flipped: well-formed and wrong
        b.tuples = b"".join(bytes(rs[64 * i:64 * i + 64]) + digests[i] + keys[kidx[i]] for i in range(N))
        b.rsh = np.frombuffer(b.tuples, dtype=np.uint8).reshape(N, 160)[:, :96].copy().reshape(-1)
        b.slots = np.array([slot_of[k] for k in kidx], dtype=np.uint32)
        b.sigs = [ec.der_encode_sig(int.from_bytes(rs[64 * i:64 * i + 32], "big"), int.from_bytes(rs[64 * i + 32:64 * i + 64], "big")) for i in range(N)]
        want = ctypes.create_string_buffer((N + 7) // 8)
        tup = ctypes.create_string_buffer(b.tuples, len(b.tuples))
        oracle.sbvo_p256_verify_batch(ctypes.addressof(tup), N, ctypes.addressof(want), 8)
        b.want = sbv.bitmap_to_list(want.raw, N)
        b.want_der = [bool(oracle.sbvo_p256_verify_asn1(keys[kidx[i]][:32], keys[kidx[i]][32:], digests[i], 32, b.sigs[i], len(b.sigs[i]))) for i in range(N)]
        assert b.want == b.want_der == [i not in bad for i in range(N)]
        b.keys = [keys[k] for k in kidx]
        yield b
    finally:
        for k, default in PIECE_ENV.items():         # a later init_all keeps a size it is not given anew: hand it the defaults
            os.environ[k] = str(default)
        try:
            sbv.shutdown()
            sbv.init_all()
            sbv.clear_keys()
        finally:
            for k in PIECE_ENV:
                os.environ.pop(k, None)
            sbv.shutdown()


def pack(bits):
    return np.packbits(np.array(bits, dtype=np.uint8), bitorder="little").tobytes()


def check(n, group, got, qgot, info, want, want_q):
    assert info.shards == 1                          # one device's share, so the pieces are this call's
    bits = sbv.bitmap_to_list(got, n)
    assert bits == want[:n], [i for i in range(n) if bits[i] != want[i]][:12]
    props = n // group
    assert bytes(qgot) == want_q, [p for p in range(props) if sbv.bitmap_to_list(bytes(qgot), props)[p] != sbv.bitmap_to_list(want_q, props)[p]][:12]
    assert 0 < sum(sbv.bitmap_to_list(want_q, props)) < props          # the quorum bits are worth comparing
    assert info.h2d_us > 0 and info.kernels_us > 0


@pytest.mark.parametrize("n,group,quorum", CASES)
def test_tuple_entry_in_smallest_pieces(batch, n, group, quorum):
    b = batch
    props = n // group
    got = ctypes.create_string_buffer((n + 7) // 8)
    qgot = ctypes.create_string_buffer((props + 7) // 8)
    tup = ctypes.create_string_buffer(b.tuples[:160 * n], 160 * n)
    info = sbv.verify_batch_sharded(ctypes.addressof(tup), n, ctypes.addressof(got), group=group, quorum=quorum, quorum_out_ptr=ctypes.addressof(qgot))
    want_q = pack([len({b.keys[i] for i in range(p * group, (p + 1) * group) if b.want[i]}) >= quorum for p in range(props)])
    check(n, group, got.raw, qgot.raw, info, b.want, want_q)


@pytest.mark.parametrize("n,group,quorum", CASES)
def test_registered_key_entry_in_smallest_pieces(batch, n, group, quorum):
    b = batch
    props = n // group
    got = np.zeros((n + 7) // 8, dtype=np.uint8)
    qgot = np.zeros((props + 7) // 8, dtype=np.uint8)
    rsh, slots = b.rsh[:96 * n].copy(), b.slots[:n].copy()
    info = sbv.verify_batch_keyed_sharded(rsh.ctypes.data, slots.ctypes.data, n, got.ctypes.data, group, quorum, qgot.ctypes.data)
    check(n, group, got.tobytes(), qgot.tobytes(), info, b.want, shard.quorum_bits_slots(slots, pack(b.want[:n]), n, group, quorum))


@pytest.mark.parametrize("n,group,quorum", CASES)
def test_message_entry_in_smallest_pieces(batch, n, group, quorum):
    b = batch
    slots = b.slots[:n].tolist()
    got, qgot, info = sbv.verify_msgs_keyed_sharded(b.msgs[:n], b.sigs[:n], slots, group, quorum)
    check(n, group, got, qgot, info, b.want_der, shard.quorum_bits_slots(slots, pack(b.want_der[:n]), n, group, quorum))


def test_explicit_device_entry_in_smallest_pieces(batch):
    """verify_batch_on(0, ...): the tuple form without a group — 1 541 tuples as 512, 512, 512, 5."""
    n = 1541
    got = ctypes.create_string_buffer((n + 7) // 8)
    tup = ctypes.create_string_buffer(batch.tuples[:160 * n], 160 * n)
    sbv.verify_batch_on(0, ctypes.addressof(tup), n, ctypes.addressof(got))
    assert sbv.bitmap_to_list(got.raw, n) == batch.want[:n]

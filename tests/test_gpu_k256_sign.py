"""GPU tier of the secp256k1 batch signer (include/sbv.h: sbv_secp256k1_sign_batch, sbv_secp256k1_pubkeys and their _stream forms).

The signature is deterministic, so every byte the device writes is compared.  The expected bytes come from the emulator library
(tests/emul/k256_sign_emul.cc: the same lanes under g++), which tests/test_k256_sign_cpu.py pins to the independent signers; the
known answers and the ~300 cases of the independent Python signer also run through the device directly.  The unit operations run the
operand lists of the CPU tier (tests/k256_sign_cases.py); the _stream entries run under callers that do not synchronise — late
producer, early overwriter, X-Y-X — with the delay of tests/test_gpu_stream_order.py."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import consensus_amd as sbv
import hostlib
import k256_sign_cases as cases
from test_k256_sign_cpu import Emul

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LOW_S = cases.N, cases.LOW_S
EINVAL, ENOTINIT = -2, -5
SENTINEL = 0x3C
T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def _init():
    sbv.init(0)
    yield
    print("\n[secp256k1 sign] wall time of this file: %.1f s" % (time.perf_counter() - T0))


@pytest.fixture(scope="module")
def emul():
    return Emul()


def _sig(blob, i):
    return blob[64 * i:64 * i + 64]


def _keys(count, label=b"k256-sign-key"):
    return [int.from_bytes(hashlib.sha256(label + b"%d" % i).digest(), "big") % (N - 1) + 1 for i in range(count)]


def _digests(n, rng_seed):
    return random.Random(rng_seed).randbytes(32 * n)


def _dev(torch, data, dtype=np.uint8):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=dtype).copy()).cuda()


def test_community_known_answers():
    vs = cases.vectors()
    keys, digests = b"".join(v["d"] for v in vs), b"".join(v["digest"] for v in vs)
    low, low_rid, ok = sbv.secp256k1_sign_batch(keys, digests, None, low_s=True)
    assert ok == b"\x01" * 4 and [_sig(low, i) for i in range(4)] == [v["sig"] for v in vs]
    raw, raw_rid, ok = sbv.secp256k1_sign_batch(keys, digests, list(range(4)))
    assert ok == b"\x01" * 4
    for i, v in enumerate(vs):
        s = int.from_bytes(v["sig"][32:], "big")
        assert _sig(raw, i) == v["sig"][:32] + cases.be32(N - s) and raw_rid[i] ^ low_rid[i] == 1
    first = sbv.debug_secp256k1_sign_op(0, [cases.op_record(v["d"], v["digest"]) for v in vs])
    assert [o[:32] for o in first] == [v["k"] for v in vs]


def test_device_equals_the_independent_python_signer():
    """the 300 seeded pairs and the edge digests under the edge keys, case i under key i, both flag settings"""
    pairs = cases.sign_cases()
    keys, digests = b"".join(cases.be32(d) for d, _ in pairs), b"".join(h for _, h in pairs)
    for flags in (0, LOW_S):
        sigs, rid, ok = sbv.secp256k1_sign_batch(keys, digests, None, low_s=bool(flags))
        want = cases.sign_expected(flags)
        assert ok == b"\x01" * len(pairs)
        bad = [i for i in range(len(pairs)) if (_sig(sigs, i), rid[i]) != want[i]]
        assert not bad, (flags, len(bad), bad[:8])


def _geometry_digests(n):
    """random digests with the edge digests at the first and last lanes of a wavefront and of a workgroup (and of the batch)"""
    dig = bytearray(_digests(n, 0x6E0 + n))
    spots = [0, 63, 64, 127, 255, 256, 511, 8191, 8192, n - 1]
    for j, lane in enumerate(s for s in spots if s < n):
        dig[32 * lane:32 * lane + 32] = cases.be32(cases.EDGE_DIGESTS[j % len(cases.EDGE_DIGESTS)])
    return bytes(dig)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 8229])
def test_launch_geometry_every_byte_and_nothing_behind_n(emul, n):
    import torch
    nk = 37
    keys = b"".join(cases.be32(d) for d in _keys(nk))
    digests = _geometry_digests(n)
    rng = random.Random(0x37 + n)
    index = [rng.randrange(nk) for _ in range(n)]
    d_keys, d_dig = _dev(torch, keys), _dev(torch, digests)
    d_idx = torch.from_numpy(np.array(index, dtype=np.uint32).view(np.int32)).cuda()
    for idx, d_index, low_s in ((None, 0, False), (index, d_idx.data_ptr(), True)):
        want = emul.sign(keys, digests, idx, LOW_S if low_s else 0)
        assert want[2] == b"\x01" * n
        d_sig = torch.full((64 * (n + 2),), SENTINEL, dtype=torch.uint8, device="cuda")
        d_rid = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), nk, d_index, d_dig.data_ptr(), n, d_sig.data_ptr(), d_rid.data_ptr(), d_ok.data_ptr(),
                                        low_s=low_s)
        torch.cuda.synchronize()
        for name, got, exp in (("sigs", d_sig, want[0]), ("recid", d_rid, want[1]), ("ok", d_ok, want[2])):
            raw = got.cpu().numpy().tobytes()
            assert raw[:len(exp)] == exp, (name, n, low_s)
            assert raw[len(exp):] == bytes([SENTINEL]) * (len(raw) - len(exp)), (name, n, low_s, "bytes behind the last item were written")
        host = sbv.secp256k1_sign_batch(keys, digests, idx, low_s=low_s)              # the host-pointer form: the same bytes
        assert host == want, (n, low_s)


def test_rejected_lanes_in_the_middle_of_a_wave(emul):
    good = _keys(5, b"k256-sign-reject")
    keys = b"".join(cases.be32(d) for d in good + [0, N, 2**256 - 1])
    n = 192
    digests = _digests(n, 0x4EC7)
    idx = [i % 5 for i in range(n)]
    bad = {70: 5, 71: 6, 100: 7, 101: 8, 102: 0xFFFFFFFF, 130: 5}             # d = 0, n, 2^256 - 1, two indices >= n_keys
    for i, v in bad.items():
        idx[i] = v
    clean = emul.sign(keys, digests, [k if k < 5 else 0 for k in idx], LOW_S)
    sigs, rid, ok = sbv.secp256k1_sign_batch(keys, digests, idx, low_s=True)
    for i in range(n):
        if i in bad:
            assert (ok[i], _sig(sigs, i), rid[i]) == (0, bytes(64), 0), i
        else:
            assert (ok[i], _sig(sigs, i), rid[i]) == (1, _sig(clean[0], i), clean[1][i]), i
    assert (sigs, rid, ok) == emul.sign(keys, digests, idx, LOW_S)
    pubs, pok = sbv.secp256k1_pubkeys(keys)
    assert pok == b"\x01" * 5 + b"\x00" * 3 and pubs[64 * 5:] == bytes(192) and (pubs, pok) == emul.pubkeys(keys)


def test_refused_calls():
    import torch
    lib = sbv.load()
    V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.sbv_secp256k1_sign_batch.argtypes = [V, U, V, V, S, U, V, V, V]
    lib.sbv_secp256k1_sign_batch_stream.argtypes = [V, U, V, V, S, U, V, V, V, V]
    lib.sbv_secp256k1_pubkeys.argtypes = [V, S, V, V]
    lib.sbv_secp256k1_pubkeys_stream.argtypes = [V, S, V, V, V]
    n, nk = 3, 2
    keys = ctypes.create_string_buffer(b"".join(cases.be32(d) for d in _keys(nk)), 32 * nk)
    dig = ctypes.create_string_buffer(_digests(n, 0x4EF), 32 * n)
    idx = (ctypes.c_uint32 * n)(0, 1, 0)
    sig, rid, okb = (ctypes.create_string_buffer(bytes([SENTINEL]) * k, k) for k in (64 * n, n, n))
    good = [keys, nk, idx, dig, n, 0, sig, rid, okb]
    for pos in (0, 3, 6, 8):                                           # keys, digests, sigs, ok
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_sign_batch(*args) == EINVAL, pos
    assert lib.sbv_secp256k1_sign_batch(keys, 0, idx, dig, n, 0, sig, rid, okb) == EINVAL
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert lib.sbv_secp256k1_sign_batch(keys, nk, idx, dig, n, flags, sig, rid, okb) == EINVAL, flags
    assert lib.sbv_secp256k1_sign_batch(keys, nk, idx, dig, 0, 0, sig, rid, okb) == 0               # n = 0: nothing is written
    assert (sig.raw, rid.raw, okb.raw) == (bytes([SENTINEL]) * 64 * n, bytes([SENTINEL]) * n, bytes([SENTINEL]) * n)
    assert lib.sbv_secp256k1_sign_batch(*good) == 0 and okb.raw == b"\x01" * n
    sig2, ok2 = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
    assert lib.sbv_secp256k1_sign_batch(keys, nk, idx, dig, n, 0, sig2, None, ok2) == 0             # a null recid is accepted
    assert (sig2.raw, ok2.raw) == (sig.raw, okb.raw)
    pub, pok = ctypes.create_string_buffer(64 * nk), ctypes.create_string_buffer(nk)
    for args in ((None, nk, pub, pok), (keys, nk, None, pok), (keys, nk, pub, None)):
        assert lib.sbv_secp256k1_pubkeys(*args) == EINVAL
    assert lib.sbv_secp256k1_pubkeys(None, 0, None, None) == 0
    # the _stream forms: the same rules, and the 4-byte alignment of keys, index, digests, sigs (pubs)
    t = {k: torch.zeros(512, dtype=torch.uint8, device="cuda") for k in ("keys", "idx", "dig", "sig", "rid", "ok")}
    t["keys"][:32 * nk] = _dev(torch, keys.raw)
    t["dig"][:32 * n] = _dev(torch, dig.raw)
    t["idx"][:4 * n] = _dev(torch, bytes(idx))
    p = {k: v.data_ptr() for k, v in t.items()}
    good = [p["keys"], nk, p["idx"], p["dig"], n, 0, p["sig"], p["rid"], p["ok"], None]
    for pos in (0, 3, 6, 8):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_sign_batch_stream(*args) == EINVAL, pos
    for pos in (0, 2, 3, 6):
        for off in (1, 2):
            args = list(good)
            args[pos] += off
            assert lib.sbv_secp256k1_sign_batch_stream(*args) == EINVAL, (pos, off)
    args = list(good)
    args[1] = 0
    assert lib.sbv_secp256k1_sign_batch_stream(*args) == EINVAL
    for flags in (2, 0x80000000):
        args = list(good)
        args[5] = flags
        assert lib.sbv_secp256k1_sign_batch_stream(*args) == EINVAL, flags
    args = list(good)
    args[7] = None                                                     # a null recid, and odd addresses for the byte arrays
    args[8] += 1
    assert lib.sbv_secp256k1_sign_batch_stream(*args) == 0
    torch.cuda.synchronize()
    assert t["sig"].cpu().numpy().tobytes()[:64 * n] == sig.raw and t["ok"].cpu().numpy().tobytes()[1:1 + n] == b"\x01" * n
    assert lib.sbv_secp256k1_pubkeys_stream(None, nk, p["sig"], p["ok"], None) == EINVAL
    assert lib.sbv_secp256k1_pubkeys_stream(p["keys"], nk, None, p["ok"], None) == EINVAL
    assert lib.sbv_secp256k1_pubkeys_stream(p["keys"], nk, p["sig"], None, None) == EINVAL
    assert lib.sbv_secp256k1_pubkeys_stream(p["keys"] + 2, nk, p["sig"], p["ok"], None) == EINVAL
    assert lib.sbv_secp256k1_pubkeys_stream(p["keys"], nk, p["sig"] + 1, p["ok"], None) == EINVAL
    assert lib.sbv_secp256k1_pubkeys_stream(p["keys"], 0, p["sig"], p["ok"], None) == 0
    with pytest.raises(sbv.SbvError) as e:
        sbv.debug_secp256k1_sign_op(4, [bytes(cases.OP_IN)])
    assert e.value.code == EINVAL
    with pytest.raises(sbv.SbvError):
        sbv.debug_secp256k1_sign_op(-1, [bytes(cases.OP_IN)])


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_unit_operations_on_the_device(emul, op):
    ins, want = cases.all_op_cases()[op]
    got = sbv.debug_secp256k1_sign_op(op, ins)
    assert emul.op(op, ins) == want
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (op, len(bad), bad[:8])


def test_round_trip_through_the_verifiers():
    """device keys -> device signatures -> sbv_secp256k1_verify_batch and the registered-key entry, 8 229 tuples"""
    n, nk = 8229, 37
    keys = b"".join(cases.be32(d) for d in _keys(nk, b"k256-sign-roundtrip"))
    digests = _digests(n, 0x8229)
    idx = [(5 * i + i // nk) % nk for i in range(n)]
    pubs, pok = sbv.secp256k1_pubkeys(keys)
    assert pok == b"\x01" * nk
    for low_s in (False, True):
        sigs, _, ok = sbv.secp256k1_sign_batch(keys, digests, idx, low_s=low_s)
        assert ok == b"\x01" * n
        tup = [_sig(sigs, i) + digests[32 * i:32 * i + 32] + pubs[64 * idx[i]:64 * idx[i] + 64] for i in range(n)]
        assert sbv.bitmap_to_list(sbv.secp256k1_verify_batch(b"".join(tup), n), n) == [True] * n
        flipped = [t if i % 2 == 0 else t[:40 + i % 20] + bytes([t[40 + i % 20] ^ (1 << (i % 8))]) + t[41 + i % 20:] for i, t in enumerate(tup)]
        assert sbv.bitmap_to_list(sbv.secp256k1_verify_batch(b"".join(flipped), n), n) == [i % 2 == 0 for i in range(n)]
    sbv.secp256k1_clear_keys()
    try:
        slots = sbv.secp256k1_register_keys([pubs[64 * k:64 * k + 64] for k in range(nk)])
        rsh = b"".join(t[:96] for t in tup)
        bm = sbv.secp256k1_verify_batch_keyed(rsh, [slots[k] for k in idx], n)
        assert sbv.bitmap_to_list(bm, n) == [True] * n
        bm = sbv.secp256k1_verify_batch_keyed(b"".join(t[:96] for t in flipped), [slots[k] for k in idx], n)
        assert sbv.bitmap_to_list(bm, n) == [i % 2 == 0 for i in range(n)]
    finally:
        sbv.secp256k1_clear_keys()


_FIRST_CALL = r"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
keys, digests = bytes.fromhex(sys.argv[2]), bytes.fromhex(sys.argv[3])
n, nk = len(digests) // 32, len(keys) // 32
d_keys = torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda()
d_dig = torch.from_numpy(np.frombuffer(digests, dtype=np.uint8).copy()).cuda()
d_out = torch.zeros(66 * n, dtype=torch.uint8, device="cuda")
lib = sbv.load()
lib.sbv_secp256k1_sign_batch_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32] + [ctypes.c_void_p] * 4
lib.sbv_secp256k1_pubkeys.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
args = [d_keys.data_ptr(), nk, None, d_dig.data_ptr(), n, 1, d_out.data_ptr(), d_out.data_ptr() + 64 * n, d_out.data_ptr() + 65 * n, None]
print("before-init", lib.sbv_secp256k1_sign_batch_stream(*args), lib.sbv_secp256k1_pubkeys(keys, nk, ctypes.create_string_buffer(64 * nk), ctypes.create_string_buffer(nk)))
sbv.init(0)
st = torch.cuda.Stream()
torch.cuda.synchronize()
sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), nk, 0, d_dig.data_ptr(), n, d_out.data_ptr(), d_out.data_ptr() + 64 * n, d_out.data_ptr() + 65 * n,
                                low_s=True, stream=st.cuda_stream)
torch.cuda.synchronize()
print("out", d_out.cpu().numpy().tobytes().hex())
"""


def test_first_secp256k1_call_of_a_process_is_the_stream_signer(emul):
    """nothing has uploaded the comb of G before the _stream signer runs; before sbv_init the entries answer SBV_ENOTINIT"""
    n, nk = 300, 7
    keys = b"".join(cases.be32(d) for d in _keys(nk, b"k256-sign-first"))
    digests = _digests(n, 0xF157)
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL, ROOT, keys.hex(), digests.hex()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("before-init", "out")))
    assert lines["before-init"] == "%d %d" % (ENOTINIT, ENOTINIT)
    sigs, rid, ok = emul.sign(keys, digests, None, LOW_S)
    assert bytes.fromhex(lines["out"]) == sigs + rid + ok


# ---- the _stream entries under callers that do not synchronise --------------------------------------------------------------------
N_STREAM, KEYS_STREAM = 8229, 64


@pytest.fixture(scope="module")
def streams(emul):
    import torch
    from test_gpu_stream_order import DELAY_FACTOR, DELAY_MAX_MS, DELAY_MIN_MS, Delay

    class S:
        pass
    s = S()
    s.torch = torch
    keys = b"".join(cases.be32(d) for d in _keys(KEYS_STREAM, b"k256-sign-stream"))           # X and Y: the same keys, other digests
    rng = random.Random(0x8229)
    index = [rng.randrange(KEYS_STREAM) for _ in range(N_STREAM)]
    s.want, s.want_pubs, s.src = {}, b"".join(emul.pubkeys(keys)), {}
    for g, seed in (("x", 0x58), ("y", 0x59)):
        digests = _digests(N_STREAM, seed)
        s.want[g] = b"".join(emul.sign(keys, digests, index, LOW_S))
        s.src[g] = [_dev(torch, keys), _dev(torch, digests)]
    assert not any(_sig(s.want["x"], i) == _sig(s.want["y"], i) for i in range(N_STREAM))
    s.bufs = [torch.empty_like(a) for a in s.src["x"]]
    s.d_index = torch.from_numpy(np.array(index, dtype=np.uint32).view(np.int32)).cuda()
    s.outs = [torch.full((66 * N_STREAM,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.pubs = [torch.full((65 * KEYS_STREAM,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.hosts = [torch.zeros(66 * N_STREAM, dtype=torch.uint8).pin_memory() for _ in range(3)]
    s.hpubs = [torch.zeros(65 * KEYS_STREAM, dtype=torch.uint8).pin_memory() for _ in range(3)]
    s.stream = torch.cuda.Stream()
    torch.cuda.synchronize()                          # the fills above ran on the default stream

    def produce(g):
        for dst, a in zip(s.bufs, s.src[g]):
            dst.copy_(a, non_blocking=True)

    def call(k):
        """public keys and signatures from the input buffers, then the copies of the results into pinned memory: all on s.stream"""
        sp, o = s.stream.cuda_stream, s.outs[k].data_ptr()
        sbv.secp256k1_pubkeys_stream(s.bufs[0].data_ptr(), KEYS_STREAM, s.pubs[k].data_ptr(), s.pubs[k].data_ptr() + 64 * KEYS_STREAM, sp)
        sbv.secp256k1_sign_batch_stream(s.bufs[0].data_ptr(), KEYS_STREAM, s.d_index.data_ptr(), s.bufs[1].data_ptr(), N_STREAM, o, o + 64 * N_STREAM,
                                        o + 65 * N_STREAM, low_s=True, stream=sp)
        s.hosts[k].copy_(s.outs[k], non_blocking=True)
        s.hpubs[k].copy_(s.pubs[k], non_blocking=True)

    def check(k, g, what):
        got, want = s.hosts[k].numpy().tobytes(), s.want[g]
        if got != want:
            other = s.want["x" if g == "y" else "y"]
            a, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            kind = "the OTHER generation's" if got == other else "a mixture: %d bytes differ, first at %d" % (int((a != w).sum()), int(np.flatnonzero(a != w)[0]))
            raise AssertionError("%s: output %d is not generation %s's but %s" % (what, k, g.upper(), kind))
        assert s.hpubs[k].numpy().tobytes() == s.want_pubs, (what, k, "public keys")
    s.produce, s.call, s.check = produce, call, check
    s.delay = Delay(torch)
    with torch.cuda.stream(s.stream):
        produce("x")
        call(0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(0)
        b.record()
        torch.cuda.synchronize()
    s.call_ms = a.elapsed_time(b)
    s.delay_ms = min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * s.call_ms))
    check(0, "x", "warm call")
    print("\n[secp256k1 sign, stream order] one warm pubkeys + sign of %d: %.3f ms; delay %.1f ms" % (N_STREAM, s.call_ms, s.delay_ms))
    return s


def _held_back(s):
    """the delay on the current stream and an event behind it: still pending after the last enqueue = the GPU had everything queued first"""
    s.delay(s.delay_ms)
    gate = s.torch.cuda.Event()
    gate.record()
    return gate


@pytest.mark.parametrize("overwrite", [False, True], ids=["late_producer", "early_overwriter"])
def test_stream_late_producer_and_early_overwriter(streams, overwrite):
    s, torch = streams, streams.torch
    with torch.cuda.stream(s.stream):
        s.produce("x")
        torch.cuda.synchronize()
        gate = _held_back(s)
        s.produce("y")
        s.call(1)
        if overwrite:
            s.produce("x")
            s.hosts[1].copy_(s.outs[1], non_blocking=True)
        pending = not gate.query()
    torch.cuda.synchronize()
    assert pending, "the delay had run out before the last enqueue: the schedule proved nothing"
    s.check(1, "y", "early overwriter" if overwrite else "late producer")
    if overwrite:
        for dst, a in zip(s.bufs, s.src["x"]):
            assert torch.equal(dst, a)


def test_stream_x_y_x_back_to_back(streams):
    s, torch = streams, streams.torch
    with torch.cuda.stream(s.stream):
        gate = _held_back(s)
        for k, g in enumerate("xyx"):
            s.produce(g)
            s.call(k)
        pending = not gate.query()
    torch.cuda.synchronize()
    assert pending, "the delay had run out before the last enqueue: the schedule proved nothing"
    for k, g in enumerate("xyx"):
        s.check(k, g, "X-Y-X")


def test_host_sign_batch_equals_a_loop_of_sign():
    """Signer::SignBatch under Scheme::SECP256K1 with a device initialised: 70 messages of mixed length, the empty one among them"""
    host = hostlib.load()
    V, S = ctypes.c_void_p, ctypes.c_size_t
    host.sbvh_sign_batch.restype = S
    host.sbvh_sign_batch.argtypes = [V, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), S, ctypes.c_char_p, S]
    rng = random.Random(0x70)
    lens = [0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120, 1000] + [rng.randrange(300) for _ in range(58)]
    rng.shuffle(lens)
    msgs = [rng.randbytes(k) for k in lens]
    assert len(msgs) == 70 and b"" in msgs
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    offs = (ctypes.c_uint64 * 71)(*off)
    signer = host.sbvh_signer_new_scheme(2, 1, cases.be32(_keys(1, b"k256-sign-host")[0]))           # Scheme::SECP256K1
    try:
        out, one = ctypes.create_string_buffer(80 * 70), ctypes.create_string_buffer(80)
        assert host.sbvh_sign_batch(signer, b"".join(msgs) + b"\0", offs, 70, out, 80) == 70
        for i, m in enumerate(msgs):
            k = host.sbvh_sign(signer, m, len(m), one, 80)
            assert 8 <= k <= 72 and out.raw[80 * i:80 * i + k] == one.raw[:k] and out.raw[80 * i + k:80 * i + 80] == bytes(80 - k), i
    finally:
        host.sbvh_signer_free(signer)

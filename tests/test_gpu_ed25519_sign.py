"""GPU tier of the Ed25519 batch signer (include/sbv.h: sbv_ed25519_expand_keys, sbv_ed25519_sign_msgs and their _stream forms).

The signature is deterministic, so every byte the device writes is compared: with RFC 8032 section 7.1, and with the C oracle's
independent signer (sbvo_ed25519_sign, sbvo_ed25519_public_key) for every other message.  The unit operations run the operand lists
of the CPU tier (tests/ed_sign_cases.py) on the device; the two _stream entries run under callers that do not synchronise — the
schedules of tests/test_gpu_stream_order.py that apply to an entry without state: late producer, early overwriter, X-Y-X — with that
file's delay."""
import concurrent.futures
import ctypes
import os
import random
import sys
import time

import numpy as np
import pytest

import consensus_amd as sbv
import ed25519_py as ed
import ed_sign_cases as cases
import hostlib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(os.cpu_count() or 1, 16)
EINVAL = -2      # SBV_EINVAL


@pytest.fixture(scope="module", autouse=True)
def _init():
    sbv.init(0)
    yield


@pytest.fixture(scope="module")
def ref(oracle):
    """the oracle's signer and key derivation, spread over a few threads (the C calls release the interpreter lock)"""
    oracle.sbvo_ed25519_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    oracle.sbvo_ed25519_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]

    class Ref:
        @staticmethod
        def pks(seeds):
            out = []
            for s in seeds:
                pk = ctypes.create_string_buffer(32)
                oracle.sbvo_ed25519_public_key(s, pk)
                out.append(pk.raw)
            return out

        @staticmethod
        def sign(seeds, msgs, key_index=None):
            n, out = len(msgs), [None] * len(msgs)

            def work(t):
                sig = ctypes.create_string_buffer(64)
                for i in range(t, n, THREADS):
                    oracle.sbvo_ed25519_sign(seeds[key_index[i] if key_index is not None else i % len(seeds)], msgs[i], len(msgs[i]), sig)
                    out[i] = sig.raw
            with concurrent.futures.ThreadPoolExecutor(THREADS) as ex:
                list(ex.map(work, range(THREADS)))
            return out
    return Ref


def _lib():
    lib = sbv.load()
    V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.sbv_ed25519_expand_keys.argtypes = [V, S, V, V]
    lib.sbv_ed25519_sign_msgs.argtypes = [V, U, V, V, V, S, V, V]
    return lib


def test_rfc8032_vectors_byte_for_byte():
    vs = cases.rfc_vectors()
    expanded, pks = sbv.ed25519_expand_keys([v["seed"] for v in vs])
    assert pks == [v["pk"] for v in vs]
    for i, v in enumerate(vs):
        a, prefix = ed.secret_expand(v["seed"])
        assert expanded[96 * i:96 * i + 96] == cases.le32(a % ed.L) + prefix + v["pk"]
    sigs, ok = sbv.ed25519_sign_msgs(expanded, [v["msg"] for v in vs], list(range(len(vs))))
    assert ok == b"\x01" * len(vs) and sigs == [v["sig"] for v in vs]
    sigs, ok = sbv.ed25519_sign([v["seed"] for v in vs], [v["msg"] for v in vs])          # both steps, a null index: key i % 4
    assert ok == b"\x01" * len(vs) and sigs == [v["sig"] for v in vs]


def test_length_sweep_equals_the_oracle_and_verifies(ref):
    """4 099 signatures (sixteen workgroups and three lanes), 37 keys, a random index, every length of cases.LENGTHS among random ones"""
    n, seeds = 4099, cases.seeds(37)
    msgs = cases.mixed_messages(n, 0x4099)
    assert set(cases.LENGTHS) <= {len(m) for m in msgs}
    rng = random.Random(0x1D37)
    idx = [rng.randrange(37) for _ in range(n)]
    expanded, pks = sbv.ed25519_expand_keys(seeds)
    assert pks == ref.pks(seeds)
    sigs, ok = sbv.ed25519_sign_msgs(expanded, msgs, idx)
    want = ref.sign(seeds, msgs, idx)
    assert ok == b"\x01" * n
    bad = [i for i in range(n) if sigs[i] != want[i]]
    assert not bad, (len(bad), bad[:8], [len(msgs[i]) for i in bad[:8]])
    keys = [pks[k] for k in idx]
    bm = sbv.ed25519_verify_msgs(sigs, keys, msgs)
    assert sbv.bitmap_to_list(bm, n) == [True] * n
    flipped = [(bytes([m[0] ^ 1]) + m[1:]) if m else b"\x01" for m in msgs]              # one bit of each message (the empty ones gain a byte)
    bm = sbv.ed25519_verify_msgs(sigs, keys, flipped)
    assert sbv.bitmap_to_list(bm, n) == [False] * n


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_launch_geometry_with_a_null_index(ref, n):
    seeds = cases.seeds(max(n, 3), b"ed-sign-geometry")
    msgs = [b"geometry %d of %d" % (i, n) + bytes(i % 97) for i in range(n)]
    for nk in sorted({1, 3, n}):
        expanded, _ = sbv.ed25519_expand_keys(seeds[:nk])
        sigs, ok = sbv.ed25519_sign_msgs(expanded, msgs)
        assert ok == b"\x01" * n and sigs == ref.sign(seeds[:nk], msgs), (n, nk)


def test_rejected_lanes_and_errors(ref):
    import torch
    seeds = cases.seeds(5, b"ed-sign-reject")
    expanded, _ = sbv.ed25519_expand_keys(seeds)
    n = 300
    msgs = [b"reject %d" % i + bytes(i % 50) for i in range(n)]
    idx = [i % 5 for i in range(n)]
    bad = {0: 5, 63: 0xFFFFFFFF, 64: 5, 130: 0xFFFFFFFF, 255: 5, 256: 6, 299: 0xFFFFFFFF}
    for i, v in bad.items():
        idx[i] = v
    sigs, ok = sbv.ed25519_sign_msgs(expanded, msgs, idx)
    want = ref.sign(seeds, msgs, [k if k < 5 else 0 for k in idx])
    for i in range(n):
        assert (ok[i], sigs[i]) == ((0, bytes(64)) if i in bad else (1, want[i])), i
    # the _stream form cannot refuse a call: a decreasing offset pair is that lane's ok = 0, its neighbours sign what their offsets say
    payload, off = cases.pack_messages(msgs)
    off2 = list(off)
    off2[101] = off[100] - 3                               # pair (100, 101) decreases; lane 101 runs from the moved offset to its own end
    msgs2 = list(msgs)
    msgs2[101] = payload[off2[101]:off2[102]]
    want2 = ref.sign(seeds, msgs2, [i % 5 for i in range(n)])
    d_exp = torch.from_numpy(np.frombuffer(expanded, dtype=np.uint8).copy()).cuda()
    d_msgs = torch.from_numpy(np.frombuffer(payload, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.array(off2, dtype=np.uint64).view(np.int64)).cuda()
    d_sig = torch.full((64 * n,), 0x3C, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    sbv.ed25519_sign_msgs_stream(d_exp.data_ptr(), 5, 0, d_msgs.data_ptr(), d_off.data_ptr(), n, d_sig.data_ptr(), d_ok.data_ptr(), 0)
    torch.cuda.synchronize()
    got, gok = d_sig.cpu().numpy().tobytes(), d_ok.cpu().numpy().tobytes()
    for i in range(n):
        assert (gok[i], got[64 * i:64 * i + 64]) == ((0, bytes(64)) if i == 100 else (1, want2[i])), i
    # the host form refuses the whole call
    lib = _lib()
    offs = (ctypes.c_uint64 * 4)(0, 2, 4, 6)
    sig, okb = ctypes.create_string_buffer(b"\x3c" * 192, 192), ctypes.create_string_buffer(b"\x07" * 3, 3)
    exp3, body = ctypes.create_string_buffer(expanded, len(expanded)), ctypes.create_string_buffer(b"abcdef", 6)
    good = [exp3, 5, None, body, offs, 3, sig, okb]
    for pos in (0, 4, 6, 7):                                # expanded, offsets, sigs, ok
        args = list(good)
        args[pos] = None
        assert lib.sbv_ed25519_sign_msgs(*args) == EINVAL, pos
    assert lib.sbv_ed25519_sign_msgs(exp3, 5, None, None, offs, 3, sig, okb) == EINVAL          # bytes to read and no payload
    assert lib.sbv_ed25519_sign_msgs(exp3, 0, None, body, offs, 3, sig, okb) == EINVAL
    assert lib.sbv_ed25519_sign_msgs(exp3, 5, None, body, (ctypes.c_uint64 * 4)(1, 2, 4, 6), 3, sig, okb) == EINVAL
    assert lib.sbv_ed25519_sign_msgs(exp3, 5, None, body, (ctypes.c_uint64 * 4)(0, 4, 2, 6), 3, sig, okb) == EINVAL
    assert lib.sbv_ed25519_sign_msgs(exp3, 5, None, body, offs, (1 << 21) + 1, sig, okb) == EINVAL
    seeds3 = ctypes.create_string_buffer(b"".join(seeds[:3]), 96)
    out3 = ctypes.create_string_buffer(b"\x3c" * 288, 288)
    assert lib.sbv_ed25519_expand_keys(None, 3, out3, None) == EINVAL and lib.sbv_ed25519_expand_keys(seeds3, 3, None, None) == EINVAL
    assert lib.sbv_ed25519_sign_msgs(exp3, 5, None, body, offs, 0, sig, okb) == 0               # n = 0: nothing is written
    assert lib.sbv_ed25519_expand_keys(seeds3, 0, out3, None) == 0
    assert sig.raw == b"\x3c" * 192 and okb.raw == b"\x07" * 3 and out3.raw == b"\x3c" * 288
    assert lib.sbv_ed25519_expand_keys(seeds3, 3, out3, None) == 0 and out3.raw == expanded[:288]   # a null pks: the records alone
    assert lib.sbv_ed25519_sign_msgs(exp3, 5, None, body, offs, 3, sig, okb) == 0 and okb.raw == b"\x01" * 3
    assert [sig.raw[64 * i:64 * i + 64] for i in range(3)] == ref.sign(seeds, [b"ab", b"cd", b"ef"])
    with pytest.raises(sbv.SbvError):
        sbv.debug_ed25519_sign_op(3, [bytes(32)])


def test_unit_operations_on_the_device():
    for op, (blobs, want) in enumerate((cases.muladd_cases(), cases.reduce_cases(), cases.encode_cases())):
        got = sbv.debug_ed25519_sign_op(op, blobs)
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        assert not bad, (op, len(bad), bad[:8])


# ---- the _stream entries under callers that do not synchronise --------------------------------------------------------------------
N_STREAM, KEYS_STREAM = 8229, 64


class _Gen:
    """one generation of inputs: seeds, messages (packed), offsets — and what the oracle signs for them"""

    def __init__(self, ref, tag, index):
        self.seeds = cases.seeds(KEYS_STREAM, b"ed-sign-stream-" + tag)
        self.msgs = cases.mixed_messages(N_STREAM, 0x57 + tag[0], max_random=120)
        payload, off = cases.pack_messages(self.msgs)
        self.arrays = [np.frombuffer(b"".join(self.seeds), dtype=np.uint8), np.frombuffer(payload, dtype=np.uint8),
                       np.array(off, dtype=np.uint64).view(np.int64)]
        self.want = b"".join(ref.sign(self.seeds, self.msgs, index)) + b"\x01" * N_STREAM
        self.pks = b"".join(ref.pks(self.seeds))


@pytest.fixture(scope="module")
def streams(ref):
    import torch
    from test_gpu_stream_order import DELAY_FACTOR, DELAY_MAX_MS, DELAY_MIN_MS, Delay

    class S:
        pass
    s = S()
    s.torch = torch
    rng = random.Random(0x8229)
    s.index = [rng.randrange(KEYS_STREAM) for _ in range(N_STREAM)]
    s.gen = {"x": _Gen(ref, b"x", s.index), "y": _Gen(ref, b"y", s.index)}
    s.src = {g: [torch.from_numpy(a.copy()).cuda() for a in s.gen[g].arrays] for g in "xy"}
    size = max(s.src["x"][1].numel(), s.src["y"][1].numel())
    s.bufs = [torch.empty_like(s.src["x"][0]), torch.zeros(size, dtype=torch.uint8, device="cuda"), torch.empty_like(s.src["x"][2])]
    s.d_index = torch.from_numpy(np.array(s.index, dtype=np.uint32).view(np.int32)).cuda()
    s.exp = [torch.empty(96 * KEYS_STREAM, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.pks = [torch.empty(32 * KEYS_STREAM, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.outs = [torch.full((65 * N_STREAM,), 0x3C, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.hosts = [torch.zeros(65 * N_STREAM, dtype=torch.uint8).pin_memory() for _ in range(3)]
    s.hpks = [torch.zeros(32 * KEYS_STREAM, dtype=torch.uint8).pin_memory() for _ in range(3)]
    s.stream = torch.cuda.Stream()

    def produce(g):
        for dst, a in zip(s.bufs, s.src[g]):
            dst[:a.numel()].copy_(a, non_blocking=True)

    def call(k):
        """expand, then sign with the records just expanded, then the copies of the results into pinned memory: all on s.stream"""
        sp = s.stream.cuda_stream
        sbv.ed25519_expand_keys_stream(s.bufs[0].data_ptr(), KEYS_STREAM, s.exp[k].data_ptr(), s.pks[k].data_ptr(), sp)
        sbv.ed25519_sign_msgs_stream(s.exp[k].data_ptr(), KEYS_STREAM, s.d_index.data_ptr(), s.bufs[1].data_ptr(), s.bufs[2].data_ptr(), N_STREAM,
                                     s.outs[k].data_ptr(), s.outs[k].data_ptr() + 64 * N_STREAM, sp)
        s.hosts[k].copy_(s.outs[k], non_blocking=True)
        s.hpks[k].copy_(s.pks[k], non_blocking=True)

    def check(k, g, what):
        got, want = s.hosts[k].numpy().tobytes(), s.gen[g].want
        if got != want:
            other = s.gen["x" if g == "y" else "y"].want
            a, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            kind = "the OTHER generation's" if got == other else "a mixture: %d bytes differ, first at %d" % (int((a != w).sum()), int(np.flatnonzero(a != w)[0]))
            raise AssertionError("%s: output %d is not generation %s's but %s" % (what, k, g.upper(), kind))
        assert s.hpks[k].numpy().tobytes() == s.gen[g].pks, (what, k, "public keys")
    s.produce, s.call, s.check = produce, call, check
    # the delay: ten times one warm call, as tests/test_gpu_stream_order.py sizes it
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
    print("\n[ed25519 sign, stream order] one warm expand + sign of %d: %.3f ms; delay %.1f ms" % (N_STREAM, s.call_ms, s.delay_ms))
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
            assert torch.equal(dst[:a.numel()], a)


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


def test_round_trip_through_the_registry(ref):
    n, seeds = 2048, cases.seeds(16, b"ed-sign-registry")
    msgs = cases.mixed_messages(n, 0x2048, max_random=200)
    idx = [(5 * i + i // 16) % 16 for i in range(n)]
    expanded, pks = sbv.ed25519_expand_keys(seeds)
    sbv.ed25519_clear_keys()
    try:
        slots = sbv.ed25519_register_keys(pks)
        sigs, ok = sbv.ed25519_sign_msgs(expanded, msgs, idx)
        assert ok == b"\x01" * n
        bm = sbv.ed25519_verify_msgs_keyed(sigs, msgs, [slots[k] for k in idx])
        assert sbv.bitmap_to_list(bm, n) == [True] * n
    finally:
        sbv.ed25519_clear_keys()


def test_host_sign_batch_equals_a_loop_of_sign():
    host = hostlib.load()
    V, S = ctypes.c_void_p, ctypes.c_size_t
    host.sbvh_sign_batch.restype = S
    host.sbvh_sign_batch.argtypes = [V, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), S, ctypes.c_char_p, S]
    msgs = cases.mixed_messages(300, 0x300)
    payload, off = cases.pack_messages(msgs)
    offs = (ctypes.c_uint64 * 301)(*off)
    for scheme, seed in ((1, cases.seeds(1, b"ed-sign-host")[0]), (0, (7).to_bytes(32, "big"))):
        signer = host.sbvh_signer_new_scheme(scheme, 1, seed)
        try:
            out, one = ctypes.create_string_buffer(80 * 300), ctypes.create_string_buffer(80)
            assert host.sbvh_sign_batch(signer, payload + b"\0", offs, 300, out, 80) == 300
            for i, m in enumerate(msgs):
                k = host.sbvh_sign(signer, m, len(m), one, 80)
                assert out.raw[80 * i:80 * i + k] == one.raw[:k] and (scheme != 1 or k == 64), (scheme, i)
        finally:
            host.sbvh_signer_free(signer)


def test_signing_rate_is_reported(capsys):
    """Not a pass/fail bar: tools/bench_ed25519_sign.py's device measurements at 2^18 signatures, 64-byte messages, 1 024 keys"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_ed25519_sign as bench
    t0 = time.perf_counter()
    r = bench.device_rates(1 << 18, 1024)
    assert r["ok_all_ones"] and r["forms_agree"]
    with capsys.disabled():
        print("\n[ed25519 sign] 2^18 signatures, 64-byte messages, 1 024 keys: stream form %.3f ms (%.3f .. %.3f) = %.1f M signatures/s; "
              "host-pointer form %.3f ms (%.3f .. %.3f) = %.1f M signatures/s; expanding 1 024 keys %.3f ms = %.1f %% of expand + sign  [%.1f s]"
              % (r["stream_form"]["median_ms"], r["stream_form"]["min_ms"], r["stream_form"]["max_ms"], r["stream_form"]["signatures_per_s"] / 1e6,
                 r["host_pointer_form"]["median_ms"], r["host_pointer_form"]["min_ms"], r["host_pointer_form"]["max_ms"],
                 r["host_pointer_form"]["signatures_per_s"] / 1e6, r["expand_keys"]["median_ms"], 100 * r["expand_share_of_expand_plus_sign"],
                 time.perf_counter() - t0))

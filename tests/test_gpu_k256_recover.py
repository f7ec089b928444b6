"""GPU tier of the secp256k1 public-key recovery (include/sbv.h: sbv_secp256k1_recover, sbv_secp256k1_recover_stream,
sbv_secp256k1_recover_workspace, sbv_debug_secp256k1_recover_op), through the C-ABI and the Python wrapper.

Every byte the device writes is compared with the Python-integer model of tests/k256_recover_cases.py (the cases of the CPU tier,
tests/test_k256_recover_cpu.py).  Large batches tile the case set with a rotation, so their expected values are the model's too.  The
_stream entry runs under callers that do not synchronise — late producer, early overwriter, X-Y-X, two streams with two workspaces —
with the delay of tests/test_gpu_stream_order.py."""
import ctypes
import hashlib
import os
import random
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import consensus_amd as sbv
import hostlib
import k256_recover_cases as cases
import k256_sign_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LOW_S = cases.N, cases.LOW_S
EINVAL, ENOTINIT = -2, -5
SENTINEL = 0x3C
STRIP = 1536                                       # bytes of one lane's table strip (include/sbv.h)
TAIL = 4096                                        # sentinel bytes behind a workspace
LANES = int(re.search(r"#define SBV_K256_RECOVER_LANES (\d+)", open(os.path.join(ROOT, "include", "sbv.h")).read()).group(1))
T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def _init():
    sbv.init(0)
    yield
    print("\n[secp256k1 recover] wall time of this file: %.1f s" % (time.perf_counter() - T0))


@pytest.fixture(scope="module")
def model():
    """the expected values of every case, from the Python-integer model, once"""
    t = time.perf_counter()
    exp = cases.expected_all()
    print("\n[secp256k1 recover] the model of %d cases: %.1f s" % (len(exp), time.perf_counter() - t))
    return exp


def _dev(torch, data, dtype=np.uint8):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=dtype).copy()).cuda()


def _differ(idx, pubs, ok, exp):
    return [(i, cases.cases()[i][0]) for k, i in enumerate(idx) if (pubs[64 * k:64 * k + 64], ok[k]) != exp[i]]


@pytest.mark.parametrize("flags", [0, LOW_S])
def test_every_case_against_the_model(model, flags):
    idx, sigs, rid, digs = cases.by_flags(flags)
    pubs, ok = sbv.secp256k1_recover(sigs, rid, digs, low_s=bool(flags))
    bad = _differ(idx, pubs, ok, model)
    assert not bad, (flags, len(bad), bad[:8])
    assert min(ok) == 0 and max(ok) == 1


@pytest.mark.parametrize("op", [0, 1, 2])
def test_unit_operations_on_the_device(op):
    ins, want = cases.all_op_cases()[op]
    got = sbv.debug_secp256k1_recover_op(op, ins)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (op, len(bad), bad[:8])


def _stream_call(torch, n, sigs, rid, digs, flags, stream=0):
    """the _stream entry on fresh buffers with sentinels behind pubs, ok and the workspace: (pubs buffer, ok buffer, workspace)"""
    d_sig, d_rid, d_dig = _dev(torch, sigs), _dev(torch, rid), _dev(torch, digs)
    wb = sbv.secp256k1_recover_workspace(n)
    assert wb == min(n, LANES) * STRIP
    d_pub = torch.full((64 * (n + 2),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_work = torch.full((wb + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_work.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    sbv.secp256k1_recover_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_pub.data_ptr(), d_ok.data_ptr(), d_work.data_ptr(), wb,
                                 low_s=bool(flags), stream=stream)
    torch.cuda.synchronize()
    return d_pub, d_ok, d_work, wb


def _check_geometry(torch, n, flags, shift=0):
    sigs, rid, digs, want_pubs, want_ok = cases.tiled(flags, n, shift)
    d_pub, d_ok, d_work, wb = _stream_call(torch, n, sigs, rid, digs, flags)
    pubs, ok = d_pub.cpu().numpy().tobytes(), d_ok.cpu().numpy().tobytes()
    if pubs[:64 * n] != want_pubs or ok[:n] != want_ok:
        bad = [i for i in range(n) if pubs[64 * i:64 * i + 64] != want_pubs[64 * i:64 * i + 64] or ok[i] != want_ok[i]]
        raise AssertionError("n = %d, flags %d: %d items differ, first %s" % (n, flags, len(bad), bad[:8]))
    assert pubs[64 * n:] == bytes([SENTINEL]) * 128, (n, "bytes behind the last key were written")
    assert ok[n:] == bytes([SENTINEL]) * 64, (n, "bytes behind the last ok were written")
    assert bool((d_work[wb:] == SENTINEL).all()), (n, "bytes behind the workspace were written")
    return sigs, rid, digs, want_pubs, want_ok


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_launch_geometry_every_byte_and_nothing_behind_n(model, n):
    import torch
    for flags in (0, LOW_S):
        sigs, rid, digs, want_pubs, want_ok = _check_geometry(torch, n, flags, shift=n)
        assert sbv.secp256k1_recover(sigs, rid, digs, low_s=bool(flags)) == (want_pubs, want_ok), (n, flags)      # the host-pointer form


@pytest.mark.parametrize("n", [LANES - 1, LANES, LANES + 1, 2 * LANES + 3], ids=["lanes-1", "lanes", "lanes+1", "2lanes+3"])
def test_capped_grid_reuses_its_strips(model, n):
    """around the cap of the grid: the last lane idle, every lane once, lane 0 twice, every lane twice or three times"""
    import torch
    _check_geometry(torch, n, LOW_S if n == LANES + 1 else 0, shift=3)


def test_host_pointer_form_beyond_the_cap(model):
    n = LANES + 300
    sigs, rid, digs, want_pubs, want_ok = cases.tiled(0, n, 11)
    assert sbv.secp256k1_recover(sigs, rid, digs) == (want_pubs, want_ok)


def test_refused_calls():
    import torch
    lib = sbv.load()
    V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.sbv_secp256k1_recover.argtypes = [V, V, V, S, U, V, V]
    lib.sbv_secp256k1_recover_stream.argtypes = [V, V, V, S, U, V, V, V, S, V]
    lib.sbv_secp256k1_recover_workspace.argtypes = [S]
    lib.sbv_secp256k1_recover_workspace.restype = S
    assert [lib.sbv_secp256k1_recover_workspace(k) for k in (0, 1, 2, LANES, LANES + 1, 1 << 40)] == [0, STRIP, 2 * STRIP, LANES * STRIP, LANES * STRIP,
                                                                                                   LANES * STRIP]
    n = 3
    sigs, rid, digs, want_pubs, want_ok = cases.tiled(0, n)
    assert want_ok == b"\x01" * n
    b_sig, b_rid, b_dig = (ctypes.create_string_buffer(x, len(x)) for x in (sigs, rid, digs))
    pub, okb = (ctypes.create_string_buffer(bytes([SENTINEL]) * k, k) for k in (64 * n, n))
    good = [b_sig, b_rid, b_dig, n, 0, pub, okb]
    for pos in (0, 1, 2, 5, 6):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_recover(*args) == EINVAL, pos
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        args = list(good)
        args[4] = flags
        assert lib.sbv_secp256k1_recover(*args) == EINVAL, flags
    assert lib.sbv_secp256k1_recover(b_sig, b_rid, b_dig, 0, 0, pub, okb) == 0                      # n = 0: nothing is written
    assert lib.sbv_secp256k1_recover(None, None, None, 0, 0, None, None) == 0
    assert (pub.raw, okb.raw) == (bytes([SENTINEL]) * 64 * n, bytes([SENTINEL]) * n)
    assert lib.sbv_secp256k1_recover(*good) == 0 and (pub.raw, okb.raw) == (want_pubs, want_ok)
    # the _stream form: the same rules, the 4-byte alignment of sigs, digests and pubs, the workspace's 16 bytes and its size
    t = {k: torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda") for k in ("sig", "rid", "dig", "pub", "ok")}
    t["work"] = torch.full((n * STRIP + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    t["sig"][:64 * n] = _dev(torch, sigs)
    t["rid"][:n] = _dev(torch, rid)
    t["dig"][:32 * n] = _dev(torch, digs)
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in t.items()}
    good = [p["sig"], p["rid"], p["dig"], n, 0, p["pub"], p["ok"], p["work"], n * STRIP, None]
    for pos in (0, 1, 2, 5, 6, 7):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_recover_stream(*args) == EINVAL, pos
    for pos in (0, 2, 5):
        for off in (1, 2):
            args = list(good)
            args[pos] += off
            assert lib.sbv_secp256k1_recover_stream(*args) == EINVAL, (pos, off)
    for off in (1, 4, 8):
        args = list(good)
        args[7] += off
        args[8] += 64 - off
        assert lib.sbv_secp256k1_recover_stream(*args) == EINVAL, off
    for short in (0, STRIP, n * STRIP - 1):
        args = list(good)
        args[8] = short
        assert lib.sbv_secp256k1_recover_stream(*args) == EINVAL, short
    for flags in (2, 0x80000000):
        args = list(good)
        args[4] = flags
        assert lib.sbv_secp256k1_recover_stream(*args) == EINVAL, flags
    args = list(good)
    args[3] = 0
    assert lib.sbv_secp256k1_recover_stream(*args) == 0
    torch.cuda.synchronize()
    assert bool((t["pub"] == SENTINEL).all()) and bool((t["ok"] == SENTINEL).all()) and bool((t["work"] == SENTINEL).all())       # refused calls wrote nothing
    args = list(good)
    args[1] += 1                                                        # odd addresses for the byte arrays are fine
    args[6] += 3
    t["rid"][1:1 + n] = _dev(torch, rid)
    assert lib.sbv_secp256k1_recover_stream(*args) == 0
    torch.cuda.synchronize()
    assert t["pub"].cpu().numpy().tobytes()[:64 * n] == want_pubs and t["ok"].cpu().numpy().tobytes()[3:3 + n] == want_ok
    with pytest.raises(sbv.SbvError) as e:
        sbv.debug_secp256k1_recover_op(3, [bytes(cases.OP_IN)])
    assert e.value.code == EINVAL
    with pytest.raises(sbv.SbvError):
        sbv.debug_secp256k1_recover_op(-1, [bytes(cases.OP_IN)])
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_recover_stream(p["sig"], p["rid"], p["dig"], n, p["pub"], p["ok"], p["work"], n * STRIP, flags=4)


_FIRST_CALL = r"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
sigs, rid, digs = (bytes.fromhex(a) for a in sys.argv[2:5])
n = len(rid)
dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
d_sig, d_rid, d_dig = dev(sigs), dev(rid), dev(digs)
d_out = torch.zeros(65 * n, dtype=torch.uint8, device="cuda")
d_work = torch.zeros(1536 * n, dtype=torch.uint8, device="cuda")
lib = sbv.load()
lib.sbv_secp256k1_recover_stream.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_uint32] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
lib.sbv_secp256k1_recover.argtypes = [ctypes.c_char_p] * 3 + [ctypes.c_size_t, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
args = [d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, 0, d_out.data_ptr(), d_out.data_ptr() + 64 * n, d_work.data_ptr(), 1536 * n, None]
print("before-init", lib.sbv_secp256k1_recover_stream(*args), lib.sbv_secp256k1_recover(sigs, rid, digs, n, 0, ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)))
sbv.init(0)
st = torch.cuda.Stream()
torch.cuda.synchronize()
sbv.secp256k1_recover_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_out.data_ptr(), d_out.data_ptr() + 64 * n, d_work.data_ptr(), 1536 * n,
                             stream=st.cuda_stream)
torch.cuda.synchronize()
print("out", d_out.cpu().numpy().tobytes().hex())
"""


def test_first_secp256k1_call_of_a_process_is_the_stream_recovery(model):
    """nothing has uploaded the comb of G before the _stream entry runs; before sbv_init the entries answer SBV_ENOTINIT"""
    n = 300
    sigs, rid, digs, want_pubs, want_ok = cases.tiled(0, n, 5)
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL, ROOT, sigs.hex(), rid.hex(), digs.hex()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("before-init", "out")))
    assert lines["before-init"] == "%d %d" % (ENOTINIT, ENOTINIT)
    assert bytes.fromhex(lines["out"]) == want_pubs + want_ok


# ---- the _stream entry under callers that do not synchronise -----------------------------------------------------------------------
N_STREAM = 8229


@pytest.fixture(scope="module")
def streams(model):
    import torch
    from test_gpu_stream_order import DELAY_FACTOR, DELAY_MAX_MS, DELAY_MIN_MS, Delay

    class S:
        pass
    s = S()
    s.torch = torch
    s.want, s.src = {}, {}
    for g, shift in (("x", 0), ("y", 401)):                              # two generations: the same cases, rotated against each other
        sigs, rid, digs, pubs, ok = cases.tiled(0, N_STREAM, shift)
        s.want[g] = pubs + ok
        s.src[g] = [_dev(torch, sigs), _dev(torch, rid), _dev(torch, digs)]
    assert sum(s.want["x"][64 * i:64 * i + 64] == s.want["y"][64 * i:64 * i + 64] for i in range(N_STREAM)) < N_STREAM // 10
    s.bufs = [torch.empty_like(a) for a in s.src["x"]]
    s.wb = sbv.secp256k1_recover_workspace(N_STREAM)
    s.outs = [torch.full((65 * N_STREAM,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.works = [torch.full((s.wb + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    s.hosts = [torch.zeros(65 * N_STREAM, dtype=torch.uint8).pin_memory() for _ in range(3)]
    s.stream, s.stream2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()                          # the fills above ran on the default stream

    def produce(g, bufs=None):
        for dst, a in zip(bufs or s.bufs, s.src[g]):
            dst.copy_(a, non_blocking=True)

    def call(k, bufs=None, work=0, stream=None):
        """the recovery from the input buffers, then the copy of the result into pinned memory: all on one stream"""
        b, o = bufs or s.bufs, s.outs[k].data_ptr()
        sbv.secp256k1_recover_stream(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), N_STREAM, o, o + 64 * N_STREAM, s.works[work].data_ptr(), s.wb,
                                     stream=(stream or s.stream).cuda_stream)
        s.hosts[k].copy_(s.outs[k], non_blocking=True)

    def check(k, g, what):
        got, want = s.hosts[k].numpy().tobytes(), s.want[g]
        if got != want:
            other = s.want["x" if g == "y" else "y"]
            a, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            kind = "the OTHER generation's" if got == other else "a mixture: %d bytes differ, first at %d" % (int((a != w).sum()), int(np.flatnonzero(a != w)[0]))
            raise AssertionError("%s: output %d is not generation %s's but %s" % (what, k, g.upper(), kind))
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
    print("\n[secp256k1 recover, stream order] one warm recovery of %d: %.3f ms; delay %.1f ms" % (N_STREAM, s.call_ms, s.delay_ms))
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
    assert all(bool((w[s.wb:] == SENTINEL).all()) for w in s.works)


def test_two_streams_two_workspaces_at_once(streams):
    """two calls that overlap: each on its own stream, inputs and workspace, both queued behind a delay, one synchronise at the end"""
    s, torch = streams, streams.torch
    bufs2 = [torch.empty_like(a) for a in s.src["y"]]
    torch.cuda.synchronize()
    gates = []
    for st, g, k, bufs, work in ((s.stream, "x", 0, s.bufs, 0), (s.stream2, "y", 1, bufs2, 1)):
        with torch.cuda.stream(st):
            gates.append(_held_back(s))
            s.produce(g, bufs)
            s.call(k, bufs, work, st)
    pending = [not g.query() for g in gates]
    torch.cuda.synchronize()
    assert all(pending), "a delay had run out before the last enqueue: the schedule proved nothing"
    s.check(0, "x", "two streams")
    s.check(1, "y", "two streams")
    assert all(bool((w[s.wb:] == SENTINEL).all()) for w in s.works)


def test_round_trip_on_the_device():
    """sign -> recover -> compare with the public keys -> generic verify -> register the recovered keys -> keyed verify, 8 229 items; the
    signatures, ids, digests and keys stay on the device from the signer to the generic verifier"""
    import torch
    n, nk = N_STREAM, 37
    keys = b"".join(sc.be32(int.from_bytes(hashlib.sha256(b"k256-recover-roundtrip%d" % i).digest(), "big") % (N - 1) + 1) for i in range(nk))
    digests = random.Random(0x8229).randbytes(32 * n)
    idx = [(5 * i + i // nk) % nk for i in range(n)]
    d_keys, d_dig = _dev(torch, keys), _dev(torch, digests)
    d_idx = torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).cuda()
    d_sig, d_rid, d_sok = (torch.zeros(k, dtype=torch.uint8, device="cuda") for k in (64 * n, n, n))
    d_pub, d_rok = torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_kpub, d_kok = torch.zeros(64 * nk, dtype=torch.uint8, device="cuda"), torch.zeros(nk, dtype=torch.uint8, device="cuda")
    wb = sbv.secp256k1_recover_workspace(n)
    d_work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), nk, d_idx.data_ptr(), d_dig.data_ptr(), n, d_sig.data_ptr(), d_rid.data_ptr(), d_sok.data_ptr(),
                                        low_s=True, stream=sp)
        sbv.secp256k1_recover_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_pub.data_ptr(), d_rok.data_ptr(), d_work.data_ptr(), wb,
                                     low_s=True, stream=sp)
        sbv.secp256k1_pubkeys_stream(d_keys.data_ptr(), nk, d_kpub.data_ptr(), d_kok.data_ptr(), sp)
        # the 160-byte tuples r | s | digest | Qx | Qy of the generic verifier, assembled on the device from the recovered keys
        d_tup = torch.cat([d_sig.view(n, 64), d_dig.view(n, 32), d_pub.view(n, 64)], dim=1).contiguous()
        d_bm = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
        sbv.secp256k1_verify_batch_dev(d_tup.data_ptr(), n, d_bm.data_ptr(), sp)
    torch.cuda.synchronize()
    assert bool((d_sok == 1).all()) and bool((d_rok == 1).all()) and bool((d_kok == 1).all())
    assert torch.equal(d_pub.view(n, 64), d_kpub.view(nk, 64)[d_idx.long()]), "a recovered key is not its signer's"
    assert sbv.bitmap_to_list(d_bm.cpu().numpy().tobytes(), n) == [True] * n
    pubs, sigs = d_pub.cpu().numpy().tobytes(), d_sig.cpu().numpy().tobytes()
    sbv.secp256k1_clear_keys()
    try:
        slots = sbv.secp256k1_register_keys([pubs[64 * i:64 * i + 64] for i in range(n)])          # equal keys share a slot
        assert len(set(slots)) == nk
        rsh = b"".join(sigs[64 * i:64 * i + 64] + digests[32 * i:32 * i + 32] for i in range(n))
        assert sbv.bitmap_to_list(sbv.secp256k1_verify_batch_keyed(rsh, slots, n), n) == [True] * n
        wrong = slots[1:] + slots[:1]                                                              # the neighbour's key: another signer
        assert sbv.bitmap_to_list(sbv.secp256k1_verify_batch_keyed(rsh, wrong, n), n) == [slots[i] == wrong[i] for i in range(n)]
    finally:
        sbv.secp256k1_clear_keys()


def test_plus_n_keys_pass_the_generic_verifier(model):
    """the keys of the + n cases are accepted with their signatures: the verifier's `wraps` branch (R.x = r + n)"""
    tup = b"".join(rs + h + model[i][0] for i, (cat, rs, rid, h, _) in enumerate(cases.cases()) if cat == "plus_n")
    n = len(tup) // 160
    assert n >= 9 and sbv.bitmap_to_list(sbv.secp256k1_verify_batch(tup, n), n) == [True] * n


def test_host_recover_signers_on_the_gpu_backend_equals_the_cpu_backend(model):
    """Verifier::RecoverSigners: one device call on the GPU backend, a loop over the host form on the CPU backend, v as 27..30"""
    host = hostlib.load()
    host.sbvh_recover_signers.argtypes = [hostlib.V, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    idx, sigs, rid, digs = cases.by_flags(0)
    n = len(idx)
    blob = b"".join(sigs[64 * k:64 * k + 64] + bytes([rid[k] + 27 if rid[k] <= 3 else rid[k]]) for k in range(n))
    got = []
    for kind in (0, 1):                                                 # libsbv.so on device 0, then the callback backend
        h = host.sbvh_verifier_new_scheme(2, kind, 0, cb, None, 64, 50, 0)
        try:
            pubs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
            assert host.sbvh_recover_signers(h, blob, digs, n, pubs, ok) == hostlib.OK
            got.append((pubs.raw, ok.raw))
        finally:
            host.sbvh_verifier_free(h)
    assert got[0] == got[1]
    assert not _differ(idx, got[0][0], got[0][1], model)
